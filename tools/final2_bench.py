"""Cost of the get_final2 decoder (include/esahrnet.h esahrnet_keypoints_final2) against the default get_final, graph-replayed.
Per workload, ms per step (median of --reps windows of --steps replays) of:
  decode_default / decode_final2   heatmaps_to_keypoints(heat, refine=...) alone, on heat-maps of that workload's forward
  kp_default / kp_final2           the whole step: net(x, output="keypoints"[, refine="get_final2"])
and the added cost (final2 - default) of both.  One JSON line per workload.

    python tools/final2_bench.py [--steps 50] [--reps 5] [--only NAME] [--form decode|step|both]

--form narrows the run (for rocprofv3 --kernel-trace --stats of the decoders on their own)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {                   # name: (module, widths, crop size, batch, precision)
    "hrnet2_w32_256_b32_fp32": ("seg_hrnet2", (32, 64, 128, 256), 256, 32, "fp32"),     # the headline: 352 planes
    "hrnet3_w32_256_b32_fp32": ("seg_hrnet3", (32, 64, 128, 256), 256, 32, "fp32"),     # 960 planes
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
    for _ in range(5):
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
    out = out.clone()
    del g
    return statistics.median(ms), [min(ms), max(ms)], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--form", choices=["decode", "step", "both"], default="both")
    a = ap.parse_args()
    import torch
    from esa_pose_estimation_amd import config, inference, seg_hrnet2, seg_hrnet3, synth
    if not torch.cuda.is_available():
        raise SystemExit("final2_bench needs a GPU")
    mods = {"seg_hrnet2": seg_hrnet2, "seg_hrnet3": seg_hrnet3}
    for name, (mod, widths, hw, n, prec) in WORKLOADS.items():
        if a.only and a.only != name:
            continue
        net = mods[mod].get_seg_model(config.make_config(widths=widths), precision=prec)
        sd = synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval().freeze_weights()
        x = synth.make_crops(n, 1, hw, hw, seed=0).cuda()
        row = {"workload": name, "planes": n * net.num_keypoints, "plane": [hw, hw]}
        with torch.no_grad():
            if a.form in ("decode", "both"):
                heat = net(x).clone()               # a plain tensor: the default decoder sweeps it (no per-tile maxima note)
                for r in ("get_final", "get_final2"):
                    key = "decode_default" if r == "get_final" else "decode_final2"
                    row[f"{key}_ms"], row[f"{key}_spread"], _ = _graph_ms(
                        torch, lambda r=r: inference.heatmaps_to_keypoints(heat, refine=r), a.steps, a.reps)
                row["decode_added_ms"] = row["decode_final2_ms"] - row["decode_default_ms"]
                del heat
            if a.form in ("step", "both"):
                outs = {}
                for r in ("get_final", "get_final2"):
                    key = "kp_default" if r == "get_final" else "kp_final2"
                    row[f"{key}_ms"], row[f"{key}_spread"], outs[r] = _graph_ms(
                        torch, lambda r=r: net(x, output="keypoints", refine=r), a.steps, a.reps)
                row["step_added_ms"] = row["kp_final2_ms"] - row["kp_default_ms"]
                d = (outs["get_final2"][..., :2] - outs["get_final"][..., :2]).abs()
                row["mean_abs_dxy_vs_default_px"] = float(d.mean())
        print(json.dumps(row), flush=True)
        del net, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
