"""The get_final2 keypoints-only forward (include/esahrnet.h esahrnet_forward_keypoints_final2) against the composition it
replaces, esahrnet_forward into workspace scratch + esahrnet_keypoints_final2, graph-replayed.  Per workload: ms per step
(median of --reps windows of --steps replays) and workspace bytes per call of both, and whether kp / idx agree bit for bit.
One JSON line per workload.

    python tools/final2_kp_bench.py [--steps 30] [--reps 5] [--only NAME] [--form old|new|both]

--form narrows the run (for rocprofv3 --kernel-trace --stats of one path on its own)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {                   # name: (module, widths, crop size, batch, precision)
    "hrnet2_w32_256_b32_fp32": ("seg_hrnet2", (32, 64, 128, 256), 256, 32, "fp32"),     # the headline: VALU output layer
    "hrnet3_w32_256_b32_fp32": ("seg_hrnet3", (32, 64, 128, 256), 256, 32, "fp32"),
    "hrnet3_w48_384_b64_bf16": ("seg_hrnet3", (48, 96, 192, 384), 384, 64, "bf16"),
}


def _graph_ms(torch, fn, steps, reps):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            g.replay()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    out = tuple(t.clone() for t in out)
    del g
    return statistics.median(ms), [min(ms), max(ms)], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--form", choices=["old", "new", "both"], default="both")
    a = ap.parse_args()
    import torch
    from esa_pose_estimation_amd import _lib, config, seg_hrnet2, seg_hrnet3, synth
    if not torch.cuda.is_available():
        raise SystemExit("final2_kp_bench needs a GPU")
    lib = _lib.lib()
    mods = {"seg_hrnet2": seg_hrnet2, "seg_hrnet3": seg_hrnet3}
    for name, (mod, widths, hw, n, prec) in WORKLOADS.items():
        if a.only and a.only != name:
            continue
        net = mods[mod].get_seg_model(config.make_config(widths=widths), precision=prec)
        sd = synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval().freeze_weights()
        k = net.num_keypoints
        x = synth.make_crops(n, 1, hw, hw, seed=0).cuda()
        h = net._rt._handle_for(net, x.device)
        fw, f2, nw = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _lib.check(lib.esahrnet_workspace_bytes(h, n, hw, hw, C.byref(fw)))
        _lib.check(lib.esahrnet_keypoints_final2_workspace_bytes(n, k, hw, hw, C.byref(f2)))
        _lib.check(lib.esahrnet_keypoints_final2_forward_workspace_bytes(h, n, hw, hw, C.byref(nw)))
        hb = (n * k * hw * hw * 4 + 255) & ~255
        row = {"workload": name, "planes": n * k, "plane": [hw, hw],
               "old_bytes_per_call": fw.value + hb + f2.value, "new_bytes_per_call": nw.value}
        outs = {}
        with torch.no_grad():
            if a.form in ("old", "both"):
                ws = torch.empty(fw.value + hb + f2.value + 256, dtype=torch.uint8, device=x.device)
                wp = ws.data_ptr() + (-ws.data_ptr()) % 256

                def old():                          # hrnet.py's forward_final2 before esahrnet_forward_keypoints_final2
                    kp = torch.empty((n, k, 3), dtype=torch.float32, device=x.device)
                    idx = torch.empty((n, k), dtype=torch.int32, device=x.device)
                    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                    _lib.check(lib.esahrnet_forward(h, x.data_ptr(), n, hw, hw, wp + fw.value, wp, fw.value, st))
                    _lib.check(lib.esahrnet_keypoints_final2(wp + fw.value, n, k, hw, hw, kp.data_ptr(), idx.data_ptr(),
                                                             wp + fw.value + hb, f2.value, st))
                    return kp, idx
                row["old_ms"], row["old_spread"], outs["old"] = _graph_ms(torch, old, a.steps, a.reps)
                del ws
            if a.form in ("new", "both"):
                row["new_ms"], row["new_spread"], outs["new"] = _graph_ms(
                    torch, lambda: net(x, output="keypoints+index", refine="get_final2"), a.steps, a.reps)
            if a.form == "both":
                row["new_minus_old_ms"] = row["new_ms"] - row["old_ms"]
                (ko, io), (kn, i_n) = outs["old"], outs["new"]
                row["bit_identical"] = bool(torch.equal(ko.view(torch.int32), kn.view(torch.int32)) and torch.equal(io, i_n))
        print(json.dumps(row), flush=True)
        del net, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
