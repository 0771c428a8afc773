#!/usr/bin/env python
"""Cost of the decoders at caller-given pixels: `esahrnet_keypoints_at` per decoder at m = 1 and m = 3 beside the
arg-max decoder of the same kind (`esahrnet_keypoints_ex`, `esahrnet_keypoints_final2_hess`, `esahrnet_keypoints_gaussfit_cov`) on
the same planes: --images x --keypoints planes of --size^2 (32 x 11 x 256^2: one blob of amplitude 1, a second of 0.7, noise 0.01).
The pixels are the candidates `esahrnet_keypoints_candidates` finds (m = 1: the arg-max), so the at-decoders do the arg-max
decoders' refinement without their search.  The forms alternate window by window, so that they share whatever the machine is
doing; a window is --steps calls between two HIP events; per form the median window and the [min, max] spread, in microseconds per
call, and the ratio to the arg-max decoder of its kind.  One JSON line per form."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--keypoints", type=int, default=11)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--radius", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9, help="windows per form")
    a = ap.parse_args()
    import torch
    from esa_pose_estimation_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("refine_at_bench needs a GPU")
    n, k, s = a.images, a.keypoints, a.size
    heat = synth.make_gaussian_heatmaps(n, k, s, s, seed=0) + 0.7 * synth.make_gaussian_heatmaps(n, k, s, s, seed=1, noise=0.0)
    heat = heat.cuda().contiguous()
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    new = lambda dt, *shape: torch.empty(shape, dtype=dt, device="cuda")      # noqa: E731
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    need = C.c_size_t()
    _lib.check(lib.esahrnet_keypoints_at_workspace_bytes(n, k, s, s, 1, C.byref(need)))
    ws = new(torch.uint8, need.value + 256)
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    at = {}
    for m in (1, 3):
        cand, at[m] = new(f32, n, k, m, 3), new(i32, n, k, m)
        _lib.check(lib.esahrnet_keypoints_candidates(heat.data_ptr(), n, k, s, s, m, a.radius, cand.data_ptr(), at[m].data_ptr(), stream))
    kp, idx, hess, fit = new(f32, n, k, 3), new(i32, n, k), new(f64, n, k, 3), new(f64, n, k, 8)
    status, cov, info = new(i32, n, k), new(f64, n, k, 3), new(f64, n, k, 3)
    h = heat.data_ptr()
    forms = {"keypoints_ex": lambda: lib.esahrnet_keypoints_ex(h, n, k, s, s, kp.data_ptr(), idx.data_ptr(), stream),
             "final2_hess": lambda: lib.esahrnet_keypoints_final2_hess(h, n, k, s, s, kp.data_ptr(), idx.data_ptr(), hess.data_ptr(),
                                                                       ws_ptr, need.value, stream),
             "gaussfit_cov": lambda: lib.esahrnet_keypoints_gaussfit_cov(h, n, k, s, s, kp.data_ptr(), idx.data_ptr(), fit.data_ptr(),
                                                                         status.data_ptr(), hess.data_ptr(), cov.data_ptr(),
                                                                         info.data_ptr(), 1e-6, stream)}
    outs = {}
    for m in (1, 3):
        o = outs[m] = dict(kp=new(f32, n, k, m, 3), hess=new(f64, n, k, m, 3), fit=new(f64, n, k, m, 8), status=new(i32, n, k, m),
                           cov=new(f64, n, k, m, 3), info=new(f64, n, k, m, 3))
        p = {name: t.data_ptr() for name, t in o.items()}
        forms[f"at_final_m{m}"] = lambda m=m, p=p: lib.esahrnet_keypoints_at(h, n, k, s, s, at[m].data_ptr(), m, 0, p["kp"], None, None,
                                                                             None, None, None, 1e-6, None, 0, stream)
        forms[f"at_final2_m{m}"] = lambda m=m, p=p: lib.esahrnet_keypoints_at(h, n, k, s, s, at[m].data_ptr(), m, 1, p["kp"], p["hess"], None,
                                                                              None, None, None, 1e-6, ws_ptr, need.value, stream)
        forms[f"at_gaussfit_m{m}"] = lambda m=m, p=p: lib.esahrnet_keypoints_at(h, n, k, s, s, at[m].data_ptr(), m, 2, p["kp"], p["hess"],
                                                                                p["fit"], p["status"], p["cov"], p["info"], 1e-6, None,
                                                                                0, stream)
    for f in forms.values():                              # warm-up: code objects loaded, the planes in the caches as in the windows
        for _ in range(3):
            _lib.check(f())
    torch.cuda.synchronize()
    assert torch.equal(outs[1]["fit"].view(torch.int64).reshape(-1), fit.view(torch.int64).reshape(-1)), "m = 1 is not the arg-max decoder"
    us = {name: [] for name in forms}
    for _ in range(a.reps):
        for name, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                f()
            e1.record()
            e1.synchronize()
            us[name].append(1e3 * e0.elapsed_time(e1) / a.steps)
    base = {"final": "keypoints_ex", "final2": "final2_hess", "gaussfit": "gaussfit_cov"}
    for name, v in us.items():
        row = {"form": name, "planes": n * k, "plane": [s, s], "steps": a.steps, "reps": a.reps,
               "us_per_call": round(statistics.median(v), 2), "spread_us": [round(min(v), 2), round(max(v), 2)]}
        if name.startswith("at_"):
            kind, m = name[3:].split("_m")
            row["slots"] = n * k * int(m)
            row["pixels_inside"] = int((at[int(m)] >= 0).sum())
            row["ratio_to_" + base[kind]] = round(statistics.median(v) / statistics.median(us[base[kind]]), 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
