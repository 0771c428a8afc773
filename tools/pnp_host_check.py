#!/usr/bin/env python
"""Build tools/pnp_host_check.cpp with the host solver under host sanitizers and run it on the batches of
tests/test_pose_report_host.py (the 64-image batch of its tests 1 and 2, as a correspondence record and as keypoint rows; the
same record with all but two weights zero; the six random points without a consensus) and, for esahrnet_pnp_batch_cand, on the
scenes of tests/test_candidates_host.py (its three cases at their seeds, with 3 and with 4 candidate rows, and three-keypoint
images without a pose); the program also runs those scenes through esahrnet_pnp_batch_cand_w with a Hessian per candidate row
that it makes up itself, and through esahrnet_pnp_batch_cand_pts as the records in image pixels it makes of them (all candidates
and one, count = 0 images, NaN slots, the refused arguments).  CPU only; nothing is loaded into Python.  --sanitize "" builds it plain."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def record(f, pts, w, count, order, kp3d, K, kp=None, boxes=None, rates=None, thresh=0.5, min_k=0):
    m, k = pts.shape[:2]
    np.array([m, k, kp is not None], np.int32).tofile(f)
    for a, dt in ((pts, np.float64), (w, np.float64), (count, np.int32), (order, np.int32), (kp3d, np.float64), (K, np.float64)):
        np.ascontiguousarray(a, dt).tofile(f)
    if kp is not None:
        for a, dt in ((kp, np.float32), (boxes, np.int32), (rates, np.float64), ([thresh, min_k], np.float64)):
            np.ascontiguousarray(a, dt).tofile(f)


def candidate_record(f, cand, kp3d, K, boxes, rates, thresh, min_k, min_ratio=0.3):
    m, k, M = cand.shape[:3]
    np.array([m, k, M], np.int32).tofile(f)
    for a, dt in ((cand, np.float32), (kp3d, np.float64), (K, np.float64), (boxes, np.int32), (rates, np.float64),
                  ([thresh, min_k, min_ratio], np.float64)):
        np.ascontiguousarray(a, dt).tofile(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", default="address,undefined")
    ap.add_argument("--keep", default=None, help="directory for the program and the record file (default: a temporary one)")
    a = ap.parse_args()
    import test_pose_report_host as T
    from esa_pose_estimation_amd.build import _hipcc
    out = a.keep or tempfile.mkdtemp(prefix="pnp_host_check_")
    os.makedirs(out, exist_ok=True)
    b = T._batch()
    with open(os.path.join(out, "records.bin"), "wb") as f:
        record(f, b["pts"], b["w"], b["count"], b["order"], b["kp3d"], T.K, b["kp"], b["boxes_xy"], b["rates"])
        w2 = b["w"].copy()
        w2[:, 2:] = 0.0
        record(f, b["pts"], w2, b["count"], b["order"], b["kp3d"], T.K)
        rng = np.random.default_rng(T.FALLBACK_SEED)
        kp3d = rng.uniform(-0.5, 0.5, (6, 3))
        pts = rng.uniform([200, 100], [1700, 1100], (6, 2))
        record(f, pts[None], np.tile([1.0, 0.0, 1.0], (1, 6, 1)), [6], np.arange(6)[None], kp3d, T.K)
    import test_candidates_host as TC
    with open(os.path.join(out, "candidates.bin"), "wb") as f:
        for k, nbad in TC.CASES:
            for M in (3, 4):
                kp3d, cand, boxes, rates, _, _ = TC.scene(np.random.default_rng(TC.seed_of(k, nbad)), TC.N, k, nbad, M=M)
                candidate_record(f, cand, kp3d, TC.K, boxes, rates, 0.0, k)
        kp3d, cand, boxes, rates, _, _ = TC.scene(np.random.default_rng(15), 3, 3, 1)
        candidate_record(f, cand, kp3d, TC.K, boxes, rates, 0.0, 3)
    san = [x for s in ([f"-fsanitize={a.sanitize}", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if a.sanitize else [])
           for x in ("-Xarch_host", s)]
    exe = os.path.join(out, "pnp_host_check")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san, os.path.join(ROOT, "tools", "pnp_host_check.cpp"),
           os.path.join(ROOT, "esa-pose-estimation_amd", "csrc", "pnp_host.hip"), *([f"-fsanitize={a.sanitize}"] if a.sanitize else []),
           "-o", exe]
    print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return subprocess.run([exe, os.path.join(out, "records.bin"), os.path.join(out, "candidates.bin")]).returncode


if __name__ == "__main__":
    sys.exit(main())
