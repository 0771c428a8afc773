"""One step of pipeline.candidate_poses two ways, in one process and in alternating windows: candidates_path="loader" (the
candidates record to the host, then selection, back-projection, weights and the repairing solve there) against device_select=True
(esahrnet_correspondences_cand behind the loader's call, the record in image pixels to the host, the solve on it).  A step is the
whole call: the library calls, the one device->host copy and the native solve; it cannot be graph-replayed, so the windows are
wall-clock time around --steps calls with the device drained on both sides.  Frames are random bytes and the weights synthetic:
the solver's share of a step is that of images without a consensus, not of real ones.  One JSON line per (refine, weights): ms per
step (median and [min, max] of --reps windows), bytes copied per step on each path, and whether the two paths give the same poses.

    python tools/candidate_correspond_bench.py [--steps 20] [--reps 9] [--candidates 3] [--batch 32] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS, SCALE = (32, 64, 128, 256), 256
PAIRS = (("get_final2", "hessian"), ("gaussfit", "covariance"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--candidates", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import numpy as np
    import torch
    from esa_pose_estimation_amd import config, inference, pipeline, seg_hrnet2, synth
    if not torch.cuda.is_available():
        raise SystemExit("candidate_correspond_bench needs a GPU")
    n, M = a.batch, a.candidates
    net = seg_hrnet2.get_seg_model(config.make_config(widths=WIDTHS), precision="fp32")
    net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0), strict=True)
    net = net.cuda().eval().freeze_weights()
    k = net.num_keypoints
    frames = torch.randint(0, 256, (n, 600, 960), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    rng = np.random.default_rng(5)
    boxes = [[int(x), int(y), int(x) + 230, int(y) + 230] for x, y in zip(rng.integers(40, 600, n), rng.integers(40, 300, n))]
    kp3d = synth.make_scene(n, k, seed=0)["kp3d"]
    args = (net, frames, boxes, kp3d, synth.ESA_CAMERA)
    for refine, weights in PAIRS:
        kw = dict(candidates=M, refine=refine, weights=weights, scale=SCALE, thresh=0.0, min_k=8, on_fail="nan", threads=a.threads)
        forms = {"loader": lambda: pipeline.candidate_poses(*args, candidates_path="loader", **kw),
                 "device_select": lambda: pipeline.candidate_poses(*args, device_select=True, **kw)}
        poses = {}
        for f, fn in forms.items():
            for _ in range(3):
                poses[f] = fn()
        torch.cuda.synchronize()
        ms = {f: [] for f in forms}
        for _ in range(a.reps):
            for f, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                ms[f].append(1e3 * (time.perf_counter() - t0) / a.steps)
        gauss, cov = refine == "gaussfit", weights == "covariance"
        kind = "candidates" if refine == "get_final" else "candidates_refined"
        row = {"workload": f"hrnet2_w32_{SCALE}_b{n}_fp32", "k": k, "candidates": M, "refine": refine, "weights": weights,
               "steps": a.steps, "reps": a.reps,
               "loader_bytes_per_crop": sum(b for _, b in inference.record_fields(k, kind, gauss, cov, M)),
               "device_select_bytes_per_crop": sum(b for _, b in inference.record_fields(k, "candidate_correspondences", candidates=M))}
        for f, v in ms.items():
            row[f"{f}_ms_per_step"] = round(statistics.median(v), 4)
            row[f"{f}_ms_spread"] = [round(min(v), 4), round(max(v), 4)]
        row["device_select_minus_loader_us"] = round(1e3 * (row["device_select_ms_per_step"] - row["loader_ms_per_step"]), 1)
        same = lambda p, q: np.array_equal(np.asarray(p, np.float64).view(np.int64), np.asarray(q, np.float64).view(np.int64))   # noqa: E731
        row["bit_identical"] = all(same(qa, qb) and same(ta, tb) for (qa, ta), (qb, tb) in zip(poses["loader"], poses["device_select"]))
        row["poses_solved"] = int(sum(bool(np.isfinite(q).all()) for q, _ in poses["device_select"]))
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
