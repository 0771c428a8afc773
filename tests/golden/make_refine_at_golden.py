#!/usr/bin/env python3
"""Generate tests/golden/refine_at_*.npz by running the REAL reference's get_final (inference.py:136-152) and get_final2
(inference.py:154-169) at coordinates that are NOT the arg-max of their planes.

Run where a checkout of the reference exists:   python tests/golden/make_refine_at_golden.py REFERENCE_DIR

The cv2 shim is make_final2_golden.py's (an independent cv2.GaussianBlur(dr, (11, 11), 0): OpenCV's getGaussianKernel weights
along x, then along y, in f64).  Each fixture stores the heat-maps hm [1,K,H,W], the integer-valued coords [K,2] = (x, y) handed
to the reference, and the outputs [K,2] of get_final (`final`) and get_final2 (`final2`) at those coords -- data, never
reference source.  Both functions refine in place the coords they are given and blur (get_final2) the heat-maps they are given:
each gets copies.  The cases:
  second_blob  two blobs per plane, amplitudes 1.0 and 0.7: the coords are the integer peak of the LOWER one
  slope        pixels 2-4 px off a blob's centre: left of / above it my_taylor's offset is >= 1 and get_final takes no step, right
               of / below it the (negative) offset is taken; get_final2's Newton step is taken either way
  guard        pixels with px <= 1, px >= W - 2, py <= 1 or py >= H - 2: no step in either decoder
  det0         negative planes (every blurred value clamps to 1e-10: the Hessian is zero, det == 0) at pixels off the arg-max
  nonsquare    48 x 80 planes, coords on the second blob and on slopes
Under NumPy 2 (NEP 50) the reference's taylor runs in f32 where the restatement follows the NumPy 1.x promotion in f64: the tests
compare them with make_final2_golden.py's tolerance.
"""
import math
import os
import sys
import types

import numpy as np
from scipy import ndimage

if len(sys.argv) != 2:
    raise SystemExit("usage: make_refine_at_golden.py REFERENCE_DIR")
REF = sys.argv[1]
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import final2_ref as F  # noqa: E402  (only for its Gaussian-plane helper)


def _gaussian_blur(src, ksize, sigma):
    assert tuple(ksize) == (11, 11) and sigma == 0 and src.dtype == np.float64
    n = ksize[0]
    sig = 0.3 * ((n - 1) * 0.5 - 1) + 0.8
    t = np.array([math.exp(-((i - (n - 1) * 0.5) ** 2) / (2 * sig * sig)) for i in range(n)])
    w = t * (1.0 / t.sum())
    out = ndimage.correlate1d(src, w, axis=1, mode="constant", cval=0.0)
    return ndimage.correlate1d(out, w, axis=0, mode="constant", cval=0.0)


cv2 = types.ModuleType("cv2")
cv2.GaussianBlur = _gaussian_blur
sys.modules["cv2"] = cv2
sys.modules.setdefault("transforms", types.ModuleType("transforms")).transform_preds = None
sys.path.insert(0, REF)
import inference as ref  # noqa: E402  (reference)


def _two(h, w, first, second, sigma=2.0):
    """Planes with a blob of amplitude 1.0 at first[i] and one of 0.7 at second[i]."""
    g = F.gaussian_planes
    return (g(h, w, first, sigma) + np.float32(0.7) * g(h, w, second, sigma)).astype(np.float32)


def _cases():
    g = F.gaussian_planes
    c = {}
    first = [(12.3, 14.6), (50.7, 20.2), (30.4, 48.8), (9.6, 52.1)]
    second = [(44.6, 40.3), (15.2, 45.7), (51.3, 12.4), (40.8, 22.5)]
    c["second_blob"] = (_two(64, 64, first, second), [(round(x), round(y)) for x, y in second])
    cen = [(20.3, 18.6)] * 6
    c["slope"] = (g(40, 40, cen, 2.0), [(17, 19), (20, 15), (23, 19), (20, 22), (17, 16), (23, 21)])
    cen = [(6.4, 7.7), (25.3, 24.1), (15.6, 3.2), (4.1, 27.4), (16.0, 16.0), (28.7, 8.8), (3.3, 3.9), (14.2, 29.1)]
    c["guard"] = (g(32, 32, cen, 2.5), [(1, 8), (30, 24), (16, 1), (4, 30), (0, 0), (31, 9), (2, 1), (14, 31)])
    neg = g(40, 40, [(19.3, 21.6), (11.2, 9.9), (25.5, 25.5)], 2.0) - 2.0
    neg[1, 30, 12] = -1.2
    c["det0"] = (neg.astype(np.float32), [(10, 12), (12, 30), (25, 20)])
    first = [(10.3, 7.8), (70.6, 40.2), (41.1, 23.7), (5.4, 44.9)]
    second = [(60.2, 35.5), (20.7, 10.4), (12.5, 30.6), (66.3, 12.8)]
    c["nonsquare"] = (_two(48, 80, first, second, 2.5), [(60, 36), (21, 10), (43, 22), (64, 14)])
    return c


def main():
    for name, (planes, coords) in _cases().items():
        hm = np.ascontiguousarray(planes[None], np.float32)
        coords = np.asarray(coords, np.float32)
        k, h, w = hm.shape[1:]
        assert coords.shape == (k, 2) and (coords[:, 0] < w).all() and (coords[:, 1] < h).all()
        peaks, _ = ref.get_max_preds(hm.copy())
        assert not (peaks[0] == coords).all(1).any(), name            # none of the coords is its plane's arg-max
        final = ref.get_final(hm.copy(), coords.copy())
        final2 = ref.get_final2(hm.copy(), coords.copy())
        path = os.path.join(OUT, f"refine_at_{name}.npz")
        np.savez_compressed(path, hm=hm, coords=coords, final=np.asarray(final, np.float32), final2=np.asarray(final2, np.float32))
        print(path, hm.shape, os.path.getsize(path), "bytes")
        print("  final  - coords:", (np.asarray(final) - coords).round(3).tolist())
        print("  final2 - coords:", (np.asarray(final2) - coords).round(3).tolist())


if __name__ == "__main__":
    main()
