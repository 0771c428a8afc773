#!/usr/bin/env python3
"""Generate tests/golden/final2_*.npz by running the REAL reference's get_final2 (inference.py:154-169).

Run where a checkout of the reference exists:   python tests/golden/make_final2_golden.py REFERENCE_DIR

inference.py imports cv2 for gaussian_blur's cv2.GaussianBlur(dr, (11, 11), 0) alone; cv2 is replaced by a shim whose
GaussianBlur is an independent implementation of that call: OpenCV's getGaussianKernel(11, sigma 0) weights (sigma
0.3 * ((11 - 1) * 0.5 - 1) + 0.8 = 2) applied along x, then along y, with scipy.ndimage.correlate1d in f64.  The border mode
does not matter: gaussian_blur pads by the radius and keeps the interior.  Each fixture stores the heat-maps hm [1,K,H,W],
the arg-max coords [K,2] the reference's callers pass in, and get_final2's output [K,2] — data, never reference source.
Under NumPy 2 (NEP 50) the reference's taylor runs in f32 and inverts the Hessian with LAPACK, where the restatement
(tests/final2_ref.py) follows the NumPy 1.x promotion in f64: the tests compare them with a tolerance.
"""
import math
import os
import sys
import types

import numpy as np
from scipy import ndimage

if len(sys.argv) != 2:
    raise SystemExit("usage: make_final2_golden.py REFERENCE_DIR")
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


def _cases(rng):
    g = F.gaussian_planes
    c = {}
    cen = [(20 + rng.uniform(-0.5, 0.5) + 4 * i, 30 + rng.uniform(-0.5, 0.5) - 3 * i) for i in range(6)]
    c["sigma2"] = (g(64, 64, cen, 2.0), dict(centres=np.array(cen)))
    cen = [(32 + rng.uniform(-0.5, 0.5), 32 + rng.uniform(-0.5, 0.5)) for _ in range(8)]
    th = np.linspace(0.2, 2.9, 8)
    c["rotated"] = (g(64, 64, cen, 4.0, 1.5, th), dict(centres=np.array(cen), theta=th))
    cen = [(10.3, 7.8), (70.6, 40.2), (41.1, 23.7), (5.4, 44.9)]
    c["nonsquare"] = (g(48, 80, cen, 2.5, 1.8, 0.6), dict(centres=np.array(cen)))
    cen = [(2.0, 20.3), (29.0, 11.2), (13.4, 2.0), (17.6, 29.0), (1.0, 16.0), (30.0, 15.0)]
    c["guard"] = (g(32, 32, cen, 2.0), dict(centres=np.array(cen)))
    neg = g(40, 40, [(19.3, 21.6), (11.2, 9.9)], 2.0) - 2.0
    neg[1, 30, 12] = -1.2                              # a lone less-negative pixel: every blurred value clamps, det = 0
    c["negative"] = (neg, {})
    c["constant"] = (np.full((2, 24, 24), 0.5, np.float32), {})
    cen = [(16.4 + 3 * i, 20.7 - 2 * i) for i in range(4)]
    noisy = g(48, 48, cen, 2.0) + rng.uniform(0, 0.15, (4, 48, 48)).astype(np.float32)
    c["noisy"] = (noisy.astype(np.float32), dict(centres=np.array(cen)))
    return c


def main():
    rng = np.random.default_rng(20261016)
    for name, (planes, extra) in _cases(rng).items():
        hm = np.ascontiguousarray(planes[None], np.float32)
        preds, _ = ref.get_max_preds(hm.copy())
        coords = preds[0].copy()
        out = ref.get_final2(hm.copy(), coords.copy())            # the reference blurs its argument in place
        path = os.path.join(OUT, f"final2_{name}.npz")
        np.savez_compressed(path, hm=hm, coords=coords, out=np.asarray(out, np.float32), **extra)
        print(path, hm.shape, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
