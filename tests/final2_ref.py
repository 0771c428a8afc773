"""Host restatement of get_final2 (the reference's inference.py:154-169: gaussian_blur :96-111, taylor :54-73) in the exact
arithmetic the GPU kernel (csrc/keypoints_final2.hip, refine.h) is held to.  Test infrastructure only: the product never
imports it.

The contract, per plane of f32 heat-maps:
  * arg-max: the first row-major maximum of the RAW plane, NaN counting as the maximum (np.argmax); peak = raw value there.
  * blur: the plane zero-padded by 5 in f64, an 11-tap Gaussian (sigma 2: t_i = exp(-(i - 5)^2 / 8) times 1 / sum t, the
    weights of OpenCV's getGaussianKernel(11, 0)) along x, then along y, each sum in tap order -5 .. +5 in plain f64 (no
    fma), rounded to f32.
  * rescale: s = f32(origin_max / max(blurred)) with origin_max the raw maximum; every value f32(v * s) (gaussian_blur).
  * np.maximum(., 1e-10) (NaN-propagating), then log as f32(log(f64(.))) (NumPy's f32 log may differ by one ulp).
  * taylor, with the scalar promotion of NumPy 1.x (the reference ran on Python 3.6): the difference of two f32 values is
    f32, the first product with a Python number and everything after it is f64; the inverse Hessian in closed form.
  * the step is applied when 1 < px < W-2, 1 < py < H-2, det != 0, and origin_max, max(blurred), s and the offset are all
    finite (otherwise the reference writes NaN or raises in np.linalg: here the integer coordinates stay); the result is
    f32(f64(coordinate) + offset).
"""
from __future__ import annotations

import math

import numpy as np

_T = [math.exp(-0.125 * (i - 5.0) ** 2) for i in range(11)]
_S = 0.0
for _t in _T:
    _S += _t
_S = 1.0 / _S
GAUSS = [t * _S for t in _T]
R = 5


def blur(plane: np.ndarray) -> np.ndarray:
    """f32 [H,W] -> f32 [H,W]: the zero-padded separable 11-tap blur, f64 sums in tap order."""
    h, w = plane.shape
    p = np.zeros((h + 2 * R, w + 2 * R), np.float64)
    p[R:R + h, R:R + w] = plane
    with np.errstate(invalid="ignore", over="ignore"):
        row = GAUSS[0] * p[:, 0:w]
        for t in range(1, 11):
            row = row + GAUSS[t] * p[:, t:t + w]
        col = GAUSS[0] * row[0:h]
        for t in range(1, 11):
            col = col + GAUSS[t] * row[t:t + h]
    return col.astype(np.float32)


def _log(v: np.float32, s: np.float32) -> np.float32:
    v = np.float32(np.float64(v) * np.float64(s))
    v = np.maximum(v, np.float32(1e-10))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(np.log(np.float64(v)))


def newton(h, px: int, py: int):
    """h(dy, dx) -> f32 log values around the peak.  -> (ox, oy) in f64, or None when no step is taken."""
    f = np.float32
    with np.errstate(all="ignore"):
        dx = 0.5 * float(f(h(0, 1) - h(0, -1)))
        dy = 0.5 * float(f(h(1, 0) - h(-1, 0)))
        c2 = 2 * float(h(0, 0))
        dxx = 0.25 * ((float(h(0, 2)) - c2) + float(h(0, -2)))
        dyy = 0.25 * ((float(h(2, 0)) - c2) + float(h(-2, 0)))
        dxy = 0.25 * float(f(f(f(h(1, 1) - h(-1, 1)) - h(1, -1)) + h(-1, -1)))
    det = dxx * dyy - dxy * dxy
    if det == 0:
        return None
    try:
        i00, i01, i11 = dyy / det, -dxy / det, dxx / det
        ox, oy = -(i00 * dx + i01 * dy), -(i01 * dx + i11 * dy)
    except (OverflowError, ZeroDivisionError):
        return None
    if not (math.isfinite(ox) and math.isfinite(oy)):
        return None
    return ox, oy


def decode_plane(plane: np.ndarray):
    """f32 [H,W] -> (x, y, peak) as f32, the flat arg-max index, whether the Newton step was applied."""
    plane = np.asarray(plane, np.float32)
    hh, ww = plane.shape
    bi = int(np.argmax(plane.reshape(-1)))
    px, py = bi % ww, bi // ww
    peak = plane.reshape(-1)[bi]
    fx, fy = np.float32(px), np.float32(py)
    applied = False
    if 1 < px < ww - 2 and 1 < py < hh - 2:
        origin_max = np.max(plane)
        b = blur(plane)
        bmax = np.max(b)
        with np.errstate(all="ignore"):
            s = np.float32(np.float64(origin_max) / np.float64(bmax))
        if np.isfinite(origin_max) and np.isfinite(bmax) and np.isfinite(s):
            off = newton(lambda dy, dx: _log(b[py + dy, px + dx], s), px, py)
            if off is not None:
                fx = np.float32(px + off[0])
                fy = np.float32(py + off[1])
                applied = True
    return np.array([fx, fy, peak], np.float32), bi, applied


def decode(hm: np.ndarray):
    """f32 [N,K,H,W] -> (kp f32 [N,K,3], idx int32 [N,K], applied bool [N,K])."""
    hm = np.asarray(hm, np.float32)
    n, k = hm.shape[:2]
    kp = np.zeros((n, k, 3), np.float32)
    idx = np.zeros((n, k), np.int32)
    ap = np.zeros((n, k), bool)
    for i in range(n):
        for j in range(k):
            kp[i, j], idx[i, j], ap[i, j] = decode_plane(hm[i, j])
    return kp, idx, ap


def gaussian_planes(h, w, centres, sx, sy=None, theta=0.0, amp=1.0):
    """f32 [len(centres), h, w]: anisotropic Gaussians (sigmas sx, sy, rotated by theta) at sub-pixel (x, y) centres."""
    sy = sx if sy is None else sy
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for (cx, cy), th in zip(centres, np.broadcast_to(theta, (len(centres),))):
        c, s = math.cos(th), math.sin(th)
        u = c * (xx - cx) + s * (yy - cy)
        v = -s * (xx - cx) + c * (yy - cy)
        out.append(amp * np.exp(-0.5 * ((u / sx) ** 2 + (v / sy) ** 2)))
    return np.asarray(out, np.float32)
