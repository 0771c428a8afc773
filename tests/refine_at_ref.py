"""Host restatements of the decoders at caller-given pixels (include/esahrnet.h esahrnet_keypoints_at), in numpy.  Test
infrastructure only: the product never imports it.  Nothing is restated twice: every piece is the restatement the arg-max decoder
is already held to, handed the pixel instead of np.argmax.

  decoder 0  oracle.keypoints_ref.refine_keypoints(hm, coords): the reference's get_final(hm, coords), plus the raw value.
  decoder 1  final2_ref.blur / _log / newton at the pixel.  The rescale factor stays the whole plane's (raw maximum over blurred
             maximum); the Hessian is correspond_ref.hessian_plane's three lines at the pixel.
  decoder 2  gaussfit_ref.fit_plane(plane, idx) and gaussfit_cov_ref.cov_plane(plane, idx) on decoder 0's row.
A pixel outside the plane: NaN rows and status -1.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import final2_ref as F  # noqa: E402
import gaussfit_cov_ref as V  # noqa: E402
import gaussfit_ref as G  # noqa: E402
from oracle import keypoints_ref  # noqa: E402

NAN3 = np.full(3, np.nan)


def _inside(idx, plane):
    return 0 <= int(idx) < plane.size


def final_at(plane, idx):
    """f32 [H,W], pixel index -> (x, y, raw value) f32: a row of the reference's get_final at that pixel."""
    plane = np.asarray(plane, np.float32)
    if not _inside(idx, plane):
        return np.full(3, np.nan, np.float32)
    w = plane.shape[1]
    coords = np.array([[[idx % w, idx // w]]], np.float32)
    with np.errstate(all="ignore"):
        xy = keypoints_ref.refine_keypoints(plane[None, None], coords)[0, 0]
    return np.array([xy[0], xy[1], plane.reshape(-1)[idx]], np.float32)


def final2_at(plane, idx):
    """f32 [H,W], pixel index -> ((x, y, raw value) f32, (dxx, dxy, dyy) f64 or NaN x 3, whether the step was taken):
    final2_ref.decode_plane and correspond_ref.hessian_plane with the pixel given."""
    plane = np.asarray(plane, np.float32)
    if not _inside(idx, plane):
        return np.full(3, np.nan, np.float32), NAN3.copy(), False
    hh, ww = plane.shape
    px, py = idx % ww, idx // ww
    fx, fy = np.float32(px), np.float32(py)
    hess, applied = NAN3.copy(), False
    if 1 < px < ww - 2 and 1 < py < hh - 2:
        origin_max = np.max(plane)
        b = F.blur(plane)
        bmax = np.max(b)
        with np.errstate(all="ignore"):
            s = np.float32(np.float64(origin_max) / np.float64(bmax))
        if np.isfinite(origin_max) and np.isfinite(bmax) and np.isfinite(s):
            h = lambda dy, dx: F._log(b[py + dy, px + dx], s)            # noqa: E731
            off = F.newton(h, px, py)
            if off is not None:
                fx, fy, applied = np.float32(px + off[0]), np.float32(py + off[1]), True
                f = np.float32
                with np.errstate(all="ignore"):
                    c2 = 2 * float(h(0, 0))
                    dxx = 0.25 * ((float(h(0, 2)) - c2) + float(h(0, -2)))
                    dyy = 0.25 * ((float(h(2, 0)) - c2) + float(h(-2, 0)))
                    dxy = 0.25 * float(f(f(f(h(1, 1) - h(-1, 1)) - h(1, -1)) + h(-1, -1)))
                hess = np.array([dxx, dxy, dyy])
    return np.array([fx, fy, plane.reshape(-1)[idx]], np.float32), hess, applied


def gaussfit_at(plane, idx, cov_floor=V.COV_FLOOR):
    """f32 [H,W], pixel index -> dict(kp f32 (3,), fit (8,), status, hess (3,), cov (3,), info (3,)) as decoder 2 writes them."""
    plane = np.asarray(plane, np.float32)
    if not _inside(idx, plane):
        return dict(kp=np.full(3, np.nan, np.float32), fit=np.full(8, np.nan), status=-1, hess=NAN3.copy(), cov=NAN3.copy(),
                    info=NAN3.copy())
    kp = final_at(plane, idx)
    out = G.fit_plane(plane, idx)
    c = V.cov_plane(plane, idx, cov_floor)
    assert c["status"] == out["status"]
    if out["status"] == 0:
        kp[0], kp[1] = np.float32(out["fit"][1]), np.float32(out["fit"][2])
    return dict(kp=kp, fit=out["fit"], status=out["status"], hess=-2.0 * out["fit"][3:6], cov=c["cov"], info=c["info"])


def decode_at(hm, at, decoder, cov_floor=V.COV_FLOOR):
    """hm f32 [n,k,H,W], at int [n,k,m] -> dict of arrays [n,k,m,...]: kp, status, and per decoder hess / applied (1) or fit, hess,
    cov, info (2)."""
    hm = np.asarray(hm, np.float32)
    at = np.asarray(at)
    n, k, m = at.shape
    o = dict(kp=np.empty((n, k, m, 3), np.float32), status=np.zeros((n, k, m), np.int32), hess=np.full((n, k, m, 3), np.nan),
             fit=np.full((n, k, m, 8), np.nan), cov=np.full((n, k, m, 3), np.nan), info=np.full((n, k, m, 3), np.nan),
             applied=np.zeros((n, k, m), bool))
    for i in range(n):
        for j in range(k):
            for s in range(m):
                a = int(at[i, j, s])
                if not _inside(a, hm[i, j]):
                    o["kp"][i, j, s], o["status"][i, j, s] = np.nan, -1
                elif decoder == 0:
                    o["kp"][i, j, s] = final_at(hm[i, j], a)
                elif decoder == 1:
                    o["kp"][i, j, s], o["hess"][i, j, s], o["applied"][i, j, s] = final2_at(hm[i, j], a)
                else:
                    r = gaussfit_at(hm[i, j], a, cov_floor)
                    for name in ("kp", "fit", "status", "hess", "cov", "info"):
                        o[name][i, j, s] = r[name]
    return o
