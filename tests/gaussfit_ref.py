"""numpy f64 restatement of csrc/keypoints_gaussfit.hip (include/esahrnet.h esahrnet_keypoints_gaussfit), step for step: the
window, the start values, the lane / slot layout of the sums and their butterfly order, the Levenberg-Marquardt schedule, the
unrolled Cholesky and the acceptance rules.  Every sum is formed in the kernel's order, so the two differ in `exp` alone.
Written from the decoder's specification; nothing here calls the library."""
import numpy as np

R = 6                    # window radius
P = 7                    # A, x0, y0, a, b, c, off (x0, y0 relative to the arg-max inside the solver)
LANES = 64
SLOTS = 3
_LANE = np.arange(LANES)


def wave_sum(v):
    """[..., 64] per-lane values -> the sum every lane holds after the xor butterfly, offsets 32 .. 1."""
    v = np.asarray(v, np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ off]
    return v[..., 0]


def window(plane, idx):
    """-> (z, u, v, m) as [SLOTS, 64] arrays (pixel j of the row-major window: lane j % 64, slot j // 64; u, v relative to the
    arg-max), and the window's bounds (xlo, xhi, ylo, yhi)."""
    H, W = plane.shape
    px, py = idx % W, idx // W
    xlo, xhi, ylo, yhi = max(px - R, 0), min(px + R, W - 1), max(py - R, 0), min(py + R, H - 1)
    ww = xhi - xlo + 1
    npx = ww * (yhi - ylo + 1)
    j = np.arange(SLOTS * LANES).reshape(SLOTS, LANES)
    m = j < npx
    wy, wx = np.where(m, j // ww, 0), np.where(m, j % ww, 0)
    z = np.where(m, plane[ylo + wy, xlo + wx].astype(np.float64), 0.0)
    return z, (xlo + wx - px).astype(np.float64), (ylo + wy - py).astype(np.float64), m, (xlo, xhi, ylo, yhi)


def _residual(p, z, u, v):
    du, dv = u - p[1], v - p[2]
    q = (p[3] * du) * du + ((2.0 * p[4]) * du) * dv + (p[5] * dv) * dv
    e = np.exp(-q)
    return (p[6] + p[0] * e) - z, du, dv, e


def _lane_sum(t):
    """[..., SLOTS, 64] -> [..., 64]: slot 0, + slot 1, + slot 2."""
    acc = t[..., 0, :]
    for s in range(1, SLOTS):
        acc = acc + t[..., s, :]
    return acc


def _cost(p, z, u, v, m):
    with np.errstate(all="ignore"):
        r = _residual(p, z, u, v)[0]
        return float(wave_sum(_lane_sum(np.where(m, r * r, 0.0))))


def _tri(i, j):
    return i * (i + 1) // 2 + j


def _solve_damped(Hm, g, lam):
    """(H + lam diag(diag(H) + 1e-12)) d = -g by the kernel's Cholesky, scalar by scalar in its order; (ok, d)."""
    L = [0.0] * (P * (P + 1) // 2)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(P):
            s = Hm[_tri(j, j)] + lam * (Hm[_tri(j, j)] + 1e-12)
            for k in range(j):
                s = s - L[_tri(j, k)] * L[_tri(j, k)]
            ok = ok and bool(s > 0.0)
            dj = np.sqrt(s)
            L[_tri(j, j)] = dj
            for i in range(j + 1, P):
                t = Hm[_tri(i, j)]
                for k in range(j):
                    t = t - L[_tri(i, k)] * L[_tri(j, k)]
                L[_tri(i, j)] = t / dj
        y = [0.0] * P
        for i in range(P):
            t = -g[i]
            for k in range(i):
                t = t - L[_tri(i, k)] * y[k]
            y[i] = t / L[_tri(i, i)]
        d = [0.0] * P
        for i in range(P - 1, -1, -1):
            t = y[i]
            for k in range(i + 1, P):
                t = t - L[_tri(k, i)] * d[k]
            d[i] = t / L[_tri(i, i)]
    return ok, np.array(d, np.float64)


def fit_plane(plane, idx=None):
    """One f32 plane -> dict(status, idx, fit = (A, x0, y0, a, b, c, off, cost) or NaN x 8, iterations, raw): raw is what the
    solver ended on, (A, x0, y0, a, b, c, off) with the centre in plane coordinates, also for a plane the rules then reject
    (None for status 3)."""
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    if idx is None:
        idx = int(np.argmax(plane))                      # first maximum; a NaN is the maximum (its first occurrence)
    px, py = idx % W, idx // W
    z, u, v, m, (xlo, xhi, ylo, yhi) = window(plane, idx)
    nan8 = np.full(8, np.nan)
    if not np.isfinite(z).all():
        return dict(status=3, idx=idx, fit=nan8, iterations=0, raw=None)
    lo = float(z[m].min())
    p = np.array([float(plane[py, px]) - lo, 0.0, 0.0, 0.125, 0.0, 0.125, lo], np.float64)
    cost = _cost(p, z, u, v, m)
    lam = 1e-3
    its = 0
    for _ in range(50):
        its += 1
        with np.errstate(all="ignore"):
            r, du, dv, e = _residual(p, z, u, v)
            ae = p[0] * e
            J = np.stack([e,
                          ae * ((2.0 * p[3]) * du + (2.0 * p[4]) * dv),
                          ae * ((2.0 * p[4]) * du + (2.0 * p[5]) * dv),
                          -(ae * (du * du)),
                          -(ae * ((2.0 * du) * dv)),
                          -(ae * (dv * dv)),
                          np.ones_like(e)])
            J = np.where(m, J, 0.0)
            r = np.where(m, r, 0.0)
            Hm = np.empty(P * (P + 1) // 2)
            for i in range(P):
                for k in range(i + 1):
                    Hm[_tri(i, k)] = wave_sum(_lane_sum(J[i] * J[k]))
            g = np.array([wave_sum(_lane_sum(J[i] * r)) for i in range(P)])
        improved = done = False
        for _t in range(10):
            ok, d = _solve_damped(Hm, g, lam)
            if ok:
                pn = p + d
                cn = _cost(pn, z, u, v, m)
                if np.isfinite(cn) and cn < cost:
                    p = pn
                    lam = max(lam / 3.0, 1e-9)
                    improved = True
                    done = cost - cn < 1e-14 * max(cost, 1e-30)
                    cost = cn
                    break
            lam = lam * 4.0
        if not improved or done:
            break
    raw = np.array([p[0], px + p[1], py + p[2], p[3], p[4], p[5], p[6]])
    if not (np.isfinite(p).all() and np.isfinite(cost)):
        return dict(status=1, idx=idx, fit=nan8, iterations=its, raw=raw)
    inside = (xlo - px) <= p[1] <= (xhi - px) and (ylo - py) <= p[2] <= (yhi - py)
    if not (p[0] > 0.0 and p[3] > 0.0 and p[3] * p[5] - p[4] * p[4] > 0.0 and inside):
        return dict(status=2, idx=idx, fit=nan8, iterations=its, raw=raw)
    fit = np.array([p[0], px + p[1], py + p[2], p[3], p[4], p[5], p[6], cost])
    return dict(status=0, idx=idx, fit=fit, iterations=its, raw=raw)


def gaussfit(heat, kp_rows):
    """heat f32 [n, k, H, W], kp_rows f32 [n, k, 3] the rows of esahrnet_keypoints_ex -> (kp f32 [n, k, 3], idx int32 [n, k],
    fit f64 [n, k, 8], status int32 [n, k], hess f64 [n, k, 3]) as esahrnet_keypoints_gaussfit writes them."""
    heat = np.asarray(heat, np.float32)
    n, k = heat.shape[:2]
    kp = np.array(kp_rows, np.float32, copy=True)
    idx = np.empty((n, k), np.int32)
    fit = np.empty((n, k, 8))
    status = np.empty((n, k), np.int32)
    for i in range(n):
        for j in range(k):
            out = fit_plane(heat[i, j])
            idx[i, j], status[i, j], fit[i, j] = out["idx"], out["status"], out["fit"]
            if out["status"] == 0:
                kp[i, j, 0], kp[i, j, 1] = np.float32(out["fit"][1]), np.float32(out["fit"][2])
    return kp, idx, fit, status, -2.0 * fit[..., 3:6]


def model_residuals(params, plane, idx):
    """The residuals of (A, x0, y0, a, b, c, off), x0 / y0 in plane coordinates, over the window of `idx`, for an independent
    optimiser: plain numpy, no lane layout."""
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    px, py = idx % W, idx // W
    ys, xs = np.mgrid[max(py - R, 0):min(py + R, H - 1) + 1, max(px - R, 0):min(px + R, W - 1) + 1]
    A, x0, y0, a, b, c, off = params
    dx, dy = xs - x0, ys - y0
    return (off + A * np.exp(-(a * dx * dx + 2 * b * dx * dy + c * dy * dy)) - plane[ys, xs].astype(np.float64)).ravel()


def start_values(plane, idx):
    """The kernel's start, in plane coordinates."""
    plane = np.asarray(plane, np.float32)
    W = plane.shape[1]
    z, _, _, m, _ = window(plane, idx)
    lo = float(z[m].min())
    return np.array([float(plane.flat[idx]) - lo, idx % W, idx // W, 0.125, 0.0, 0.125, lo])


def blob(H, W, cx, cy, sx, sy, theta, amp=1.0, off=0.0):
    """f32 [H, W]: off + amp exp(-0.5 d^T Sigma^-1 d), Sigma = Rot(theta) diag(sx^2, sy^2) Rot(theta)^T; with its (a, b, c)."""
    a, b, c = abc_of(sx, sy, theta)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = xs - cx, ys - cy
    return (off + amp * np.exp(-(a * dx * dx + 2 * b * dx * dy + c * dy * dy))).astype(np.float32), (a, b, c)


def abc_of(sx, sy, theta):
    """(a, b, c) with [[a, b], [b, c]] = 0.5 Sigma^-1 of the blob with axes sx (along theta) and sy."""
    ct, st = np.cos(theta), np.sin(theta)
    ix, iy = 0.5 / sx ** 2, 0.5 / sy ** 2
    return ix * ct * ct + iy * st * st, (ix - iy) * ct * st, ix * st * st + iy * ct * ct


# ---- the fixtures the host and the GPU tests share ------------------------------------------------------------------------------
H, W = 32, 40
# name -> (cx, cy, sx, sy, theta, amp, off): noise-free blobs with a known centre
BLOBS = {
    "isotropic": (17.3, 12.6, 2.0, 2.0, 0.0, 1.0, 0.0),                    # sigma 2 at a sub-pixel centre
    "rotated": (20.25, 15.7, 3.5, 1.5, 0.6, 1.0, 0.0),                     # 1.5 x 3.5, theta 0.6
    "rotated+offset": (20.25, 15.7, 3.5, 1.5, 0.6, 0.8, 0.15),
    "border": (3.2, 14.4, 2.0, 2.0, 0.0, 1.0, 0.0),                        # peak 3 px from the left border: 10 x 13 window
    "corner": (0.3, 0.4, 2.0, 2.5, 0.3, 1.0, 0.0),                         # peak in the corner: 7 x 7 window
    "isotropic-2": (30.55, 24.45, 2.0, 2.0, 0.0, 0.7, 0.0),
    "rotated-neg": (12.8, 20.1, 1.5, 3.5, -0.9, 1.2, 0.05),
}
SMALL = [(7.6, 8.2, 2.0, 1.6, 1.0, 1.0, 0.0), (3.4, 11.7, 2.0, 2.0, 0.0, 1.0, 0.0), (12.1, 4.9, 1.5, 2.5, 0.4, 0.9, 0.1),
         (8.0, 8.0, 2.0, 2.0, 0.0, 1.0, 0.0), (14.6, 14.2, 2.0, 2.0, 0.0, 1.0, 0.0), (5.5, 5.5, 3.0, 1.2, 2.2, 1.0, 0.0)]


def fixture_batches():
    """-> {"a": ..., "b": ..., "c": ...} f32 [2, 3, 32, 40] and "small" f32 [2, 3, 16, 16], with names[batch] the plane names
    and truth[batch][i] = (cx, cy, sx, sy, theta, amp, off) or None."""
    rng = np.random.default_rng(20250)
    pl = {k: blob(H, W, *v[:5], amp=v[5], off=v[6])[0] for k, v in BLOBS.items()}
    pl["noise"] = (blob(H, W, 17.3, 12.6, 2.2, 1.8, 0.4)[0] + rng.normal(0.0, 0.02, (H, W))).astype(np.float32)   # 2 % of A
    pl["noise+offset"] = (blob(H, W, 24.7, 9.2, 1.7, 2.6, 1.9, 0.9, 0.2)[0] + rng.normal(0.0, 0.018, (H, W))).astype(np.float32)
    pl["constant"] = np.full((H, W), 0.25, np.float32)
    pl["nan"] = pl["isotropic"].copy()
    pl["nan"][9, 19] = np.nan
    pl["two-peaks"] = blob(H, W, 15.0, 12.0, 2.0, 2.0, 0.0)[0] + blob(H, W, 20.0, 12.0, 2.0, 2.0, 0.0)[0]   # equal, 5 px apart
    # rejected by the rules other than A > 0.  A blob whose centre lies outside the plane: the peak sits on the border, the fit
    # finds the true centre, which is outside the window.  A saddle (a ridge along x that RISES away from the centre, capped
    # beyond the window) with one higher pixel on it: the window's best fit has a = -7e-3 or so, far from zero on both sides
    pl["outside-x"] = blob(H, W, -3.0, 12.4, 2.5, 2.5, 0.0)[0]
    pl["outside-corner"] = blob(H, W, -2.5, -1.5, 3.0, 3.0, 0.0)[0]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    for name, spike in (("saddle", 1.0), ("saddle-2", 0.75)):
        pl[name] = (0.5 * np.exp(-(ys - 15.0) ** 2 / 8.0) * np.minimum(1.0 + 0.01 * (xs - 20.0) ** 2, 1.49)).astype(np.float32)
        pl[name][15, 20] = spike
    pl["isotropic-3"] = blob(H, W, 8.45, 25.3, 2.0, 2.0, 0.0, 0.9, 0.0)[0]
    pl["rotated-3"] = blob(H, W, 28.6, 7.75, 2.8, 1.7, 2.4, 1.1, 0.1)[0]
    names = {"a": ["isotropic", "rotated", "rotated+offset", "noise", "border", "corner"],
             "b": ["constant", "nan", "two-peaks", "isotropic-2", "rotated-neg", "noise+offset"],
             "c": ["outside-x", "outside-corner", "saddle", "saddle-2", "isotropic-3", "rotated-3"],
             "small": [f"small-{i}" for i in range(6)]}
    heat = {b: np.stack([pl[n] for n in names[b]]).reshape(2, 3, H, W) for b in ("a", "b", "c")}
    heat["small"] = np.stack([blob(16, 16, *v[:5], amp=v[5], off=v[6])[0] for v in SMALL]).reshape(2, 3, 16, 16)
    truth = {b: [BLOBS.get(n) for n in names[b]] for b in ("a", "b", "c")}
    truth["c"][4:] = [(8.45, 25.3, 2.0, 2.0, 0.0, 0.9, 0.0), (28.6, 7.75, 2.8, 1.7, 2.4, 1.1, 0.1)]
    truth["small"] = list(SMALL)
    return heat, names, truth


def scipy_fit(plane, idx):
    """scipy's trust-region least squares on the same residuals from the same start -> (params, cost, jac)."""
    from scipy.optimize import least_squares
    sol = least_squares(model_residuals, start_values(plane, idx), args=(plane, idx), method="trf", xtol=1e-15, ftol=1e-15,
                        gtol=1e-15, x_scale="jac", max_nfev=2000)
    return sol.x, float(sol.fun @ sol.fun), sol.jac


def sigma_of(a, b, c):
    """(a, b, c) -> Sigma = (2 [[a, b], [b, c]])^-1 as (sxx, sxy, syy)."""
    det = 4.0 * (a * c - b * b)
    return 2.0 * c / det, -2.0 * b / det, 2.0 * a / det


ANISO = [(17.3, 15.6, 1.5, 1.0, 0.3), (20.7, 14.2, 2.5, 1.5, 1.1), (19.5, 16.5, 3.0, 2.0, 2.0), (21.25, 13.75, 2.0, 3.5, 0.7),
         (15.0, 15.0, 3.0, 1.0, 2.6), (22.9, 17.1, 2.0, 2.0, 0.0), (18.4, 16.3, 3.5, 1.5, 1.5708), (21.0, 15.5, 1.0, 3.0, 0.9),
         (16.6, 14.4, 2.2, 1.2, 0.5), (23.3, 16.7, 1.3, 2.8, 2.9), (19.1, 13.2, 2.6, 2.4, 1.3), (20.2, 17.9, 1.8, 3.2, 0.1)]


def aniso_planes():
    """f32 [4, 3, 32, 40]: rotated anisotropic blobs of known Sigma, not blurred; and Sigma as [12, 3] = (sxx, sxy, syy)."""
    planes = np.stack([blob(H, W, cx, cy, sx, sy, th)[0] for cx, cy, sx, sy, th in ANISO]).reshape(4, 3, H, W)
    return planes, np.array([sigma_of(*abc_of(sx, sy, th)) for _, _, sx, sy, th in ANISO])


def sigma_error(est, true):
    """Frobenius distance of symmetric 2x2 matrices given as [..., 3] = (xx, xy, yy), relative to the true one's norm."""
    w = np.array([1.0, 2.0, 1.0])
    return np.sqrt((((est - true) ** 2) * w).sum(-1)) / np.sqrt(((true ** 2) * w).sum(-1))
