#!/usr/bin/env python
"""What the pose report costs the host solve (DESIGN.md §5.4 "What the solve reports").

Host poses/s of esahrnet_pnp_batch_w_ex without and with a report buffer, and, with --parent, of esahrnet_pnp_batch_w of
another build of the library (the parent commit's), on one synthetic record of --images images (11 keypoints, sigma 0.5 px,
random symmetric 2x2 weights) and --threads threads.  The forms alternate window by window, as tools/precision_bench.py's do,
so that they share whatever the machine is doing; per form the median window and the [min, max] spread.  Needs no GPU.
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=12000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=15, help="windows per form (one window = one call on the whole record)")
    ap.add_argument("--parent", default=None, help="libesahrnet.so of the parent commit: adds its esahrnet_pnp_batch_w")
    a = ap.parse_args()
    from esa_pose_estimation_amd import _lib, synth
    m, k = a.images, 11
    rng = np.random.default_rng(0)
    scene = synth.make_scene(m, k, seed=0)
    pts = np.ascontiguousarray(scene["uv"] + rng.normal(0, 0.5, scene["uv"].shape))
    w = np.ascontiguousarray(np.stack([rng.uniform(0.5, 2, (m, k)), rng.uniform(-0.3, 0.3, (m, k)), rng.uniform(0.5, 2, (m, k))], 2))
    count = np.full(m, k, np.int32)
    order = np.ascontiguousarray(np.tile(np.arange(k, dtype=np.int32), (m, 1)))
    kp3d = np.ascontiguousarray(scene["kp3d"])
    K9 = np.ascontiguousarray(np.asarray(synth.ESA_CAMERA, np.float64).reshape(9))
    q, t = np.empty((m, 4)), np.empty((m, 3))
    rep = np.empty((m, _lib.POSE_REPORT_DOUBLES))
    p = lambda x: x.ctypes.data_as(C.c_void_p)                       # noqa: E731
    head = (p(pts), p(w), p(count), m, k, p(kp3d), p(order), p(K9), a.threads, p(q), p(t))
    lib = _lib.lib()
    forms = {"ex_null": lambda: lib.esahrnet_pnp_batch_w_ex(*head, None), "ex_report": lambda: lib.esahrnet_pnp_batch_w_ex(*head, p(rep))}
    if a.parent:
        parent = _lib.load_other(a.parent)
        forms = {"parent": lambda: parent.esahrnet_pnp_batch_w(*head), **forms}
    poses = {}
    for name, f in forms.items():                                    # warm-up, and the poses must be the same bits
        assert f() == 0
        poses[name] = (q.copy(), t.copy())
    first = next(iter(poses.values()))
    assert all(np.array_equal(v[0], first[0], equal_nan=True) and np.array_equal(v[1], first[1], equal_nan=True) for v in poses.values())
    rate = {name: [] for name in forms}
    for _ in range(a.reps):
        for name, f in forms.items():
            t0 = time.perf_counter()
            f()
            rate[name].append(m / (time.perf_counter() - t0))
    row = {"images": m, "keypoints": k, "threads": a.threads, "reps": a.reps, "cpus": len(os.sched_getaffinity(0)),
           "same_poses": True}
    for name, r in rate.items():
        row[f"{name}_poses_per_s"] = round(statistics.median(r))
        row[f"{name}_spread"] = [round(min(r)), round(max(r))]
    print(json.dumps(row))


if __name__ == "__main__":
    main()
