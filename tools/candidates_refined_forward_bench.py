"""Refined candidates from crops two ways, both graph-replayed, in one process and in alternating windows:
inference.heatmaps_to_candidates(net(x), M, r, refine=...) (esahrnet_forward, the heat-maps in caller memory, then
esahrnet_keypoints_candidates_refined as a second call) against net.candidates(x, M, r, refine=...)
(esahrnet_forward_keypoints_candidates_refined: one call, the heat-maps in the workspace).  Both forms write every output their decoder
has (get_final2: the Hessians; gaussfit: fit, status, Hessians, covariance and information).  One JSON line per workload and decoder:
ms per step (median and [min, max] of --reps windows of --steps replays), the workspace bytes of each form (the two-call form's
heat-map tensor and the stand-alone decoder's workspace counted beside the forward's) and whether the two forms give the same bits.

    python tools/candidates_refined_forward_bench.py [--steps 50] [--reps 9] [--candidates 3] [--radius 6] [--only NAME] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {                   # seg_hrnet2; name: (widths, crop size, batch, precision)
    "hrnet2_w32_256_b32_fp32": ((32, 64, 128, 256), 256, 32, "fp32"),
    "hrnet2_w32_256_b32_bf16x3": ((32, 64, 128, 256), 256, 32, "bf16x3"),
}
ASK = {"get_final2": dict(return_hessian=True), "gaussfit": dict(return_fit=True, return_hessian=True, return_cov=True)}


def _bits(a, b):
    import torch
    it = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool((not a.is_floating_point() or torch.equal(torch.isnan(a), torch.isnan(b))) and torch.equal(a.view(it), b.view(it)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--candidates", type=int, default=3)
    ap.add_argument("--radius", type=int, default=6)
    ap.add_argument("--only", default="hrnet2_w32_256_b32_fp32")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch
    from esa_pose_estimation_amd import _lib, config, inference, seg_hrnet2, synth
    if not torch.cuda.is_available():
        raise SystemExit("candidates_refined_forward_bench needs a GPU")
    M, r = a.candidates, a.radius
    for name, (widths, hw, n, prec) in WORKLOADS.items():
        if a.only and a.only != name:
            continue
        net = seg_hrnet2.get_seg_model(config.make_config(widths=widths), precision=prec)
        sd = synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval().freeze_weights()
        x = synth.make_crops(n, 1, hw, hw, seed=0).cuda()
        k = net.num_keypoints
        for decoder, refine in ((1, "get_final2"), (2, "gaussfit")):
            forms = {"two_calls": lambda: inference.heatmaps_to_candidates(net(x), M, r, return_index=True, refine=refine, **ASK[refine]),
                     "fused": lambda: net.candidates(x, M, r, return_index=True, refine=refine, **ASK[refine])}
            row = {"workload": name, "k": k, "candidates": M, "nms_radius": r, "decoder": decoder, "refine": refine, "steps": a.steps,
                   "reps": a.reps}
            graphs, outs = {}, {}
            with torch.no_grad():
                for f, fn in forms.items():
                    fn()
                    torch.cuda.synchronize()
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
                    graphs[f], outs[f] = g, out
                ms = {f: [] for f in forms}
                for _ in range(a.reps):
                    for f, g in graphs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.steps):
                            g.replay()
                        e1.record()
                        e1.synchronize()
                        ms[f].append(e0.elapsed_time(e1) / a.steps)
            h = net._rt._handle_for(net, x.device)
            fwd, at, fused = C.c_size_t(), C.c_size_t(), C.c_size_t()
            _lib.check(_lib.lib().esahrnet_workspace_bytes(h, n, hw, hw, C.byref(fwd)))
            _lib.check(_lib.lib().esahrnet_keypoints_at_workspace_bytes(n, k, hw, hw, decoder, C.byref(at)))
            _lib.check(_lib.lib().esahrnet_keypoints_candidates_refined_forward_workspace_bytes(h, n, hw, hw, decoder, C.byref(fused)))
            row["two_calls_workspace_bytes"], row["two_calls_heatmap_bytes"] = fwd.value + at.value, n * k * hw * hw * 4
            row["fused_workspace_bytes"] = fused.value
            for f, v in ms.items():
                row[f"{f}_ms_per_step"] = round(statistics.median(v), 4)
                row[f"{f}_ms_spread"] = [round(min(v), 4), round(max(v), 4)]
            row["fused_minus_two_calls_us"] = round(1e3 * (row["fused_ms_per_step"] - row["two_calls_ms_per_step"]), 1)
            row["bit_identical"] = len(outs["two_calls"]) == len(outs["fused"]) and all(
                _bits(p, q) for p, q in zip(outs["two_calls"], outs["fused"]))
            line = json.dumps(row)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del graphs, outs
        del net, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
