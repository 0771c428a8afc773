"""Host restatements for the correspondence stage's GPU tests (test infrastructure only: the product never imports it).

  * hessian_plane: the Hessian (dxx, dxy, dyy) get_final2 uses at a plane's peak, in f64, built from final2_ref.blur / _log
    and the formulas of final2_ref.newton (same promotion rules: the cross difference in f32, everything else f64).
  * gaussian_hessian: the analytic Hessian of the log of a rotated Gaussian blob after the sigma-2 blur, -(Sigma + 4 I)^-1.
  * hessian_weight: csrc/correspond.h corr_hessian_weight in numpy scalars, operation for operation.
  * record: what esahrnet_correspondences writes, from inference.select_keypoints and inference.crop_to_image.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import final2_ref as F  # noqa: E402


def hessian_plane(plane: np.ndarray):
    """f32 [H,W] -> ((dxx, dxy, dyy) f64, applied): NaN x 3 when final2_ref.decode_plane takes no step."""
    plane = np.asarray(plane, np.float32)
    hh, ww = plane.shape
    _, bi, applied = F.decode_plane(plane)
    nan3 = np.full(3, np.nan)
    if not applied:
        return nan3, False
    px, py = bi % ww, bi // ww
    b = F.blur(plane)
    with np.errstate(all="ignore"):
        s = np.float32(np.float64(np.max(plane)) / np.float64(np.max(b)))
    f = np.float32

    def h(dy, dx):
        return F._log(b[py + dy, px + dx], s)

    with np.errstate(all="ignore"):
        c2 = 2 * float(h(0, 0))
        dxx = 0.25 * ((float(h(0, 2)) - c2) + float(h(0, -2)))
        dyy = 0.25 * ((float(h(2, 0)) - c2) + float(h(-2, 0)))
        dxy = 0.25 * float(f(f(f(h(1, 1) - h(-1, 1)) - h(1, -1)) + h(-1, -1)))
    return np.array([dxx, dxy, dyy]), True


def hessian(hm: np.ndarray):
    """f32 [N,K,H,W] -> (hess f64 [N,K,3], applied bool [N,K])."""
    n, k = hm.shape[:2]
    out = np.empty((n, k, 3))
    ap = np.zeros((n, k), bool)
    for i in range(n):
        for j in range(k):
            out[i, j], ap[i, j] = hessian_plane(hm[i, j])
    return out, ap


def gaussian_hessian(sx: float, sy: float, theta: float, blur_sigma: float = 2.0):
    """(dxx, dxy, dyy) of log(Gaussian(Sigma) * Gaussian(blur_sigma^2 I)) = -(Sigma + blur_sigma^2 I)^-1, Sigma the covariance
    of final2_ref.gaussian_planes(sx, sy, theta): u along (cos, sin), v along (-sin, cos)."""
    c, s = math.cos(theta), math.sin(theta)
    a, b = sx * sx + blur_sigma ** 2, sy * sy + blur_sigma ** 2
    cov = np.array([[a * c * c + b * s * s, (a - b) * c * s], [(a - b) * c * s, a * s * s + b * c * c]])
    inv = np.linalg.inv(cov)
    return np.array([-inv[0, 0], -inv[0, 1], -inv[1, 1]])


def hessian_weight(H, rate):
    """corr_hessian_weight: rate * (-H)^(1/2) as (wxx, wxy, wyy), zeros when -H is not positive definite or not finite."""
    f = np.float64
    a, b, c = -f(H[0]), -f(H[1]), -f(H[2])
    rate = f(rate)
    with np.errstate(all="ignore"):
        det = a * c - b * b
        if not (a > 0.0 and det > 0.0):
            return np.zeros(3)
        s = np.sqrt(det)
        t = np.sqrt((a + c) + f(2.0) * s)
        w = np.array([rate * ((a + s) / t), rate * (b / t), rate * ((c + s) / t)])
    return w if np.isfinite(w).all() else np.zeros(3)


def record(kp, crop_boxes, rates, valid, thresh, min_k, hess=None):
    """kp f32 [m,K,3] ... -> (count int32 [m], order int32 [m,K], pts f64 [m,K,2], w f64 [m,K,3]) by the host rule:
    inference.select_keypoints over the peaks that are numbers, inference.crop_to_image; hess given: mode 1 weights."""
    from esa_pose_estimation_amd import inference
    m, k = kp.shape[:2]
    count = np.zeros(m, np.int32)
    order = np.full((m, k), -1, np.int32)
    pts = np.zeros((m, k, 2))
    w = np.zeros((m, k, 3))
    for i in range(m):
        if not valid[i]:
            continue
        live = [j for j in range(k) if not np.isnan(kp[i, j, 2])]
        sel = inference.select_keypoints(kp[i, live, 2], thresh, min_k)          # at most len(live) of them
        idxs = [live[j] for j in sel]
        c = len(idxs)
        count[i] = c
        order[i, :c] = idxs
        ori = inference.crop_to_image(kp[i, :, :2].astype(np.float64), float(rates[i]), int(crop_boxes[i][0]), int(crop_boxes[i][1]))
        pts[i, :c] = ori[idxs]
        if hess is None:
            w[i, :c, 0] = w[i, :c, 2] = kp[i, idxs, 2]
        else:
            for r, j in enumerate(idxs):
                w[i, r] = hessian_weight(hess[i, j], rates[i])
    return count, order, pts, w
