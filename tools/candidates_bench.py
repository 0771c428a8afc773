#!/usr/bin/env python
"""Cost of the candidate decoder and of the solve on candidates.

Decoder (default): `esahrnet_keypoints_candidates` at M = 1..4 against `esahrnet_keypoints_ex` of the same library, on
--images x --keypoints planes of --size^2 (32 x 11 x 256^2: one blob of amplitude 1, a second of 0.7, noise 0.01).  The forms
alternate window by window, so that they share whatever the machine is doing; a window is --steps calls between two HIP events;
per form the median window and the [min, max] spread, in microseconds per call, and the ratio to M times the existing decoder
(the M sweeps it logically is).  One JSON line per form.

--form 0,1 (any of 0, 1, -1): the kernels of `esahrnet_keypoints_candidates_form` against each other instead — 0 the multi-sweep
kernel, 1 the one-sweep kernel, -1 what the fused paths launch — at M = 1..4 on the same planes, the same alternating windows;
one JSON line per (form, M), with the ratio to `esahrnet_keypoints_ex` and whether the form's bits are those of form 0.

--host: host poses/s of `esahrnet_pnp_batch_cand` (M = 1 and M = 3) against `esahrnet_pnp_batch_ex` on candidate 0, on one
synthetic record of --poses images (11 keypoints, sigma 0.5 px, --bad wrong primaries per image whose true place is candidate
1), alternating windows as tools/pnp_report_bench.py's.  Needs no GPU.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def decoder(a):
    import torch
    from esa_pose_estimation_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("candidates_bench needs a GPU (--host runs without one)")
    n, k, s = a.images, a.keypoints, a.size
    heat = synth.make_gaussian_heatmaps(n, k, s, s, seed=0) + 0.7 * synth.make_gaussian_heatmaps(n, k, s, s, seed=1, noise=0.0)
    heat = heat.cuda().contiguous()
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kp = torch.empty((n, k, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    cand = torch.empty((n, k, _lib.MAX_CANDIDATES, 3), dtype=torch.float32, device="cuda")
    cidx = torch.empty((n, k, _lib.MAX_CANDIDATES), dtype=torch.int32, device="cuda")
    forms = {"keypoints_ex": lambda: lib.esahrnet_keypoints_ex(heat.data_ptr(), n, k, s, s, kp.data_ptr(), idx.data_ptr(), stream)}
    for M in range(1, _lib.MAX_CANDIDATES + 1):
        forms[f"candidates_M{M}"] = lambda M=M: lib.esahrnet_keypoints_candidates(heat.data_ptr(), n, k, s, s, M, a.radius,
                                                                                   cand.data_ptr(), cidx.data_ptr(), stream)
    for f in forms.values():                              # warm-up: code objects loaded, the planes in the caches as in the windows
        for _ in range(3):
            _lib.check(f())
    torch.cuda.synchronize()
    assert torch.equal(cand[:, :, 0].view(torch.int32), kp.view(torch.int32)), "candidate 0 is not esahrnet_keypoints_ex's row"
    found = int((cidx >= 0).sum())
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
    base = statistics.median(us["keypoints_ex"])
    for name, v in us.items():
        M = int(name[-1]) if name.startswith("candidates") else 1
        print(json.dumps({"form": name, "planes": n * k, "plane": [s, s], "nms_radius": a.radius, "steps": a.steps, "reps": a.reps,
                          "us_per_call": round(statistics.median(v), 2), "spread_us": [round(min(v), 2), round(max(v), 2)],
                          "ratio_to_M_x_keypoints_ex": round(statistics.median(v) / (M * base), 3),
                          "candidates_found_at_M4": found}), flush=True)


def kernels(a):
    import torch
    from esa_pose_estimation_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("candidates_bench needs a GPU (--host runs without one)")
    kinds = [int(f) for f in a.form.split(",")]
    n, k, s = a.images, a.keypoints, a.size
    heat = synth.make_gaussian_heatmaps(n, k, s, s, seed=0) + 0.7 * synth.make_gaussian_heatmaps(n, k, s, s, seed=1, noise=0.0)
    heat = heat.cuda().contiguous()
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kp = torch.empty((n, k, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    outs = {(f, M): (torch.empty((n, k, M, 3), dtype=torch.float32, device="cuda"), torch.empty((n, k, M), dtype=torch.int32, device="cuda"))
            for f in set(kinds) | {0} for M in range(1, _lib.MAX_CANDIDATES + 1)}
    forms = {"keypoints_ex": lambda: lib.esahrnet_keypoints_ex(heat.data_ptr(), n, k, s, s, kp.data_ptr(), idx.data_ptr(), stream)}
    call = lambda f, M: lib.esahrnet_keypoints_candidates_form(heat.data_ptr(), n, k, s, s, M, a.radius, f,               # noqa: E731
                                                               outs[f, M][0].data_ptr(), outs[f, M][1].data_ptr(), stream)
    for M in range(1, _lib.MAX_CANDIDATES + 1):
        _lib.check(call(0, M))                            # the bits every form is held to
        for f in kinds:
            forms[f"form{f}_M{M}"] = lambda f=f, M=M: call(f, M)
    for f in forms.values():                              # warm-up: code objects loaded, the planes in the caches as in the windows
        for _ in range(3):
            _lib.check(f())
    torch.cuda.synchronize()
    same = {(f, M): bool(torch.equal(outs[f, M][0].view(torch.int32), outs[0, M][0].view(torch.int32)) and
                         torch.equal(outs[f, M][1], outs[0, M][1])) for f in kinds for M in range(1, _lib.MAX_CANDIDATES + 1)}
    found = int((outs[0, _lib.MAX_CANDIDATES][1] >= 0).sum())
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
    base = statistics.median(us["keypoints_ex"])
    for name, v in us.items():
        row = {"form": name, "planes": n * k, "plane": [s, s], "nms_radius": a.radius, "steps": a.steps, "reps": a.reps,
               "us_per_call": round(statistics.median(v), 2), "spread_us": [round(min(v), 2), round(max(v), 2)],
               "ratio_to_keypoints_ex": round(statistics.median(v) / base, 3), "candidates_found_at_M4": found}
        if name != "keypoints_ex":
            f, M = name[4:].split("_M")
            row["bits_of_form0"] = same[int(f), int(M)]
        print(json.dumps(row), flush=True)


def host(a):
    from esa_pose_estimation_amd import _lib, synth
    m, k, M = a.poses, 11, 3
    rng = np.random.default_rng(0)
    scene = synth.make_scene(m, k, seed=0)
    uv = scene["uv"] + rng.normal(0, 0.5, scene["uv"].shape)
    cand = np.full((m, k, M, 3), np.nan, np.float32)
    cand[:, :, 0, :2] = uv
    cand[:, :, 0, 2] = rng.uniform(0.5, 1.0, (m, k))
    for i in range(m):
        bad = rng.choice(k, a.bad, replace=False)
        cand[i, bad, 1] = cand[i, bad, 0] * [1, 1, 0.7]
        cand[i, bad, 0, :2] += rng.uniform(30, 120, (a.bad, 2)) * rng.choice([-1, 1], (a.bad, 2))
    first = np.ascontiguousarray(cand[:, :, 0])
    one = np.ascontiguousarray(cand[:, :, :1])
    kp3d = np.ascontiguousarray(scene["kp3d"])
    K9 = np.ascontiguousarray(np.asarray(synth.ESA_CAMERA, np.float64).reshape(9))
    boxes = np.zeros((m, 2), np.int32)                    # image pixels as they are: origin 0, rate 1
    rates = np.ones(m)
    q, t, rep, used = np.empty((m, 4)), np.empty((m, 3)), np.empty((m, _lib.POSE_REPORT_DOUBLES)), np.empty((m, k), np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)                       # noqa: E731
    lib = _lib.lib()
    tail = (p(kp3d), p(K9), p(boxes), p(rates), 0.0, k)
    forms = {"pnp_batch_ex": lambda: lib.esahrnet_pnp_batch_ex(p(first), m, k, *tail, a.threads, p(q), p(t), p(rep)),
             "cand_M1": lambda: lib.esahrnet_pnp_batch_cand(p(one), m, k, 1, *tail, 0.3, a.threads, p(q), p(t), p(rep), p(used)),
             "cand_M3": lambda: lib.esahrnet_pnp_batch_cand(p(cand), m, k, M, *tail, 0.3, a.threads, p(q), p(t), p(rep), p(used))}
    poses = {}
    for name, f in forms.items():
        assert f() == 0
        poses[name] = (q.copy(), t.copy())
    assert np.array_equal(poses["pnp_batch_ex"][0], poses["cand_M1"][0], equal_nan=True)
    rescued = int((used > 0).any(1).sum())
    rate = {name: [] for name in forms}
    for _ in range(a.reps):
        for name, f in forms.items():
            t0 = time.perf_counter()
            f()
            rate[name].append(m / (time.perf_counter() - t0))
    row = {"images": m, "keypoints": k, "bad_per_image": a.bad, "threads": a.threads, "reps": a.reps,
           "cpus": len(os.sched_getaffinity(0)), "rescued_images": rescued}
    for name, r in rate.items():
        row[f"{name}_poses_per_s"] = round(statistics.median(r))
        row[f"{name}_spread"] = [round(min(r)), round(max(r))]
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--form", default=None, help="comma-separated kernels of esahrnet_keypoints_candidates_form to compare, e.g. 0,1")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--keypoints", type=int, default=11)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--radius", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9, help="windows per form")
    ap.add_argument("--poses", type=int, default=12000)
    ap.add_argument("--bad", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    host(a) if a.host else kernels(a) if a.form else decoder(a)


if __name__ == "__main__":
    main()
