"""Keypoints from crops two ways, both graph-replayed: heatmaps_to_keypoints(net(x)) (heat-maps in caller memory, then the
finish or the sweep) against net(x, output="keypoints") (esahrnet_forward_keypoints: no heat-maps).  Prints one JSON line per
workload: ms per step (median of --reps windows of --steps replays), the peak memory torch allocates during one eager call of
each form after a warm-up, and whether the two forms give the same bits.

    python tools/kp_only_bench.py [--steps 50] [--reps 5] [--only NAME] [--form heat|kp|both]

--form narrows the run to one form (for rocprofv3 --kernel-trace --stats of each form on its own)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {                   # name: (module, widths, crop size, batch, precision)
    "hrnet2_w32_256_b32_fp32": ("seg_hrnet2", (32, 64, 128, 256), 256, 32, "fp32"),
    "hrnet3_w32_256_b32_fp32": ("seg_hrnet3", (32, 64, 128, 256), 256, 32, "fp32"),
    "hrnet3_w48_384_b64_bf16": ("seg_hrnet3", (48, 96, 192, 384), 384, 64, "bf16"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--form", choices=["heat", "kp", "both"], default="both")
    a = ap.parse_args()
    import torch
    from esa_pose_estimation_amd import config, inference, seg_hrnet2, seg_hrnet3, synth
    if not torch.cuda.is_available():
        raise SystemExit("kp_only_bench needs a GPU")
    mods = {"seg_hrnet2": seg_hrnet2, "seg_hrnet3": seg_hrnet3}
    forms = {"heat": lambda net, x: inference.heatmaps_to_keypoints(net(x)),
             "kp": lambda net, x: net(x, output="keypoints")}
    run = ["heat", "kp"] if a.form == "both" else [a.form]
    for name, (mod, widths, hw, n, prec) in WORKLOADS.items():
        if a.only and a.only != name:
            continue
        net = mods[mod].get_seg_model(config.make_config(widths=widths), precision=prec)
        sd = synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval().freeze_weights()
        x = synth.make_crops(n, 1, hw, hw, seed=0).cuda()
        row = {"workload": name, "k": net.num_keypoints, "heatmap_bytes": n * net.num_keypoints * hw * hw * 4}
        outs = {}
        with torch.no_grad():
            for f in run:
                fn = forms[f]
                fn(net, x)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn(net, x)
                torch.cuda.synchronize()
                row[f"{f}_peak_alloc_bytes"] = torch.cuda.max_memory_allocated() - base
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    fn(net, x)
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = fn(net, x)
                for _ in range(5):
                    g.replay()
                torch.cuda.synchronize()
                outs[f] = out.clone()
                ms = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        g.replay()
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1) / a.steps)
                row[f"{f}_ms_per_step"] = statistics.median(ms)
                row[f"{f}_ms_spread"] = [min(ms), max(ms)]
                del g
        if len(outs) == 2:
            h, k = outs["heat"], outs["kp"]
            row["bit_identical"] = bool(torch.equal(torch.isnan(h), torch.isnan(k)) and torch.equal(h.view(torch.int32),
                                                                                                     k.view(torch.int32)))
        print(json.dumps(row), flush=True)
        del net, x, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
