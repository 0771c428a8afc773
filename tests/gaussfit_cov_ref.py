"""numpy f64 restatement of the covariance pass of csrc/gaussfit.h (gaussfit_plane<COV>; include/esahrnet.h
esahrnet_keypoints_gaussfit_cov), step for step behind tests/gaussfit_ref.py's fit: one more Jacobian pass at the returned
parameters, N = J^T J in the kernel's slot and butterfly order, the iteration's Cholesky with lambda = 0 for the x0 and the y0
column of N^-1, cov = cost / (n - 7) * that block, info = -cov^-1 in the header's three lines.  gaussfit_ref supplies the window,
the lane layout, the sums, the solver and the fit; fit_plane_rel runs gaussfit_ref.fit_plane's loop once more only because that
function returns the centre in plane coordinates and the pass needs the solver's own parameters, bit for bit (the host test
holds the two to the same fit).  Written from the specification; nothing here calls the library."""
import numpy as np

import gaussfit_ref as G

P = G.P
COV_FLOOR = 1e-6                 # the reference's guard: covar[0, 0] < 1e-6 -> weight zero


def jacobian(p, z, u, v, m):
    """-> (J [7, SLOTS, 64], r [SLOTS, 64]) of the model at p (centre relative to the arg-max); an empty slot holds 0.0."""
    with np.errstate(all="ignore"):
        r, du, dv, e = G._residual(p, z, u, v)
        ae = p[0] * e
        J = np.stack([e,
                      ae * ((2.0 * p[3]) * du + (2.0 * p[4]) * dv),
                      ae * ((2.0 * p[4]) * du + (2.0 * p[5]) * dv),
                      -(ae * (du * du)),
                      -(ae * ((2.0 * du) * dv)),
                      -(ae * (dv * dv)),
                      np.ones_like(e)])
        return np.where(m, J, 0.0), np.where(m, r, 0.0)


def normal_matrix(J):
    """J^T J, lower triangle packed: every lane its slots in slot order, then the butterfly."""
    with np.errstate(all="ignore"):
        N = np.empty(P * (P + 1) // 2)
        for i in range(P):
            for k in range(i + 1):
                N[G._tri(i, k)] = G.wave_sum(G._lane_sum(J[i] * J[k]))
    return N


def fit_plane_rel(plane, idx=None):
    """gaussfit_ref.fit_plane's loop -> (status, idx, p, cost, window): p = (A, x0, y0, a, b, c, off) with the centre relative to
    the arg-max, as the solver holds it (None for status 3)."""
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    if idx is None:
        idx = int(np.argmax(plane))
    px, py = idx % W, idx // W
    win = G.window(plane, idx)
    z, u, v, m, (xlo, xhi, ylo, yhi) = win
    if not np.isfinite(z).all():
        return 3, idx, None, None, win
    lo = float(z[m].min())
    p = np.array([float(plane[py, px]) - lo, 0.0, 0.0, 0.125, 0.0, 0.125, lo], np.float64)
    cost = G._cost(p, z, u, v, m)
    lam = 1e-3
    for _ in range(50):
        J, r = jacobian(p, z, u, v, m)
        Hm = normal_matrix(J)
        with np.errstate(all="ignore"):
            g = np.array([G.wave_sum(G._lane_sum(J[i] * r)) for i in range(P)])
        improved = done = False
        for _t in range(10):
            ok, d = G._solve_damped(Hm, g, lam)
            if ok:
                pn = p + d
                cn = G._cost(pn, z, u, v, m)
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
    if not (np.isfinite(p).all() and np.isfinite(cost)):
        return 1, idx, p, cost, win
    inside = (xlo - px) <= p[1] <= (xhi - px) and (ylo - py) <= p[2] <= (yhi - py)
    if not (p[0] > 0.0 and p[3] > 0.0 and p[3] * p[5] - p[4] * p[4] > 0.0 and inside):
        return 2, idx, p, cost, win
    return 0, idx, p, cost, win


def info_of(cov, cov_floor=COV_FLOOR):
    """cov [..., 3] = (cxx, cxy, cyy) -> info = -cov^-1, the header's three lines; NaN x 3 where cov is NaN, det is not positive
    or cxx < cov_floor."""
    cov = np.asarray(cov, np.float64)
    cxx, cxy, cyy = cov[..., 0], cov[..., 1], cov[..., 2]
    with np.errstate(all="ignore"):
        det = cxx * cyy - cxy * cxy
        keep = (det > 0.0) & ~(cxx < cov_floor)
        out = np.stack([-(cyy / det), cxy / det, -(cxx / det)], -1)
    return np.where(keep[..., None], out, np.nan)


def cov_plane(plane, idx=None, cov_floor=COV_FLOOR):
    """One f32 plane -> dict(status, idx, fit (as gaussfit_ref.fit_plane's), cov (cxx, cxy, cyy), info)."""
    plane = np.asarray(plane, np.float32)
    W = plane.shape[1]
    st, idx, p, cost, (z, u, v, m, _) = fit_plane_rel(plane, idx)
    nan3 = np.full(3, np.nan)
    fit = np.full(8, np.nan)
    cov = nan3.copy()
    if st == 0:
        fit = np.array([p[0], idx % W + p[1], idx // W + p[2], p[3], p[4], p[5], p[6], cost])
        N = normal_matrix(jacobian(p, z, u, v, m)[0])
        e = np.eye(P)
        ok1, c1 = G._solve_damped(N, -e[1], 0.0)                    # N d = e1: the x0 column of N^-1
        ok2, c2 = G._solve_damped(N, -e[2], 0.0)
        dof = int(m.sum()) - P
        if ok1 and ok2 and dof > 0:
            with np.errstate(all="ignore"):
                s2 = cost / float(dof)
                c = np.array([s2 * c1[1], s2 * c1[2], s2 * c2[2]])
            if np.isfinite(c).all():
                cov = c
    return dict(status=st, idx=idx, fit=fit, cov=cov, info=info_of(cov, cov_floor))


def gaussfit_cov(heat, cov_floor=COV_FLOOR):
    """heat f32 [n, k, H, W] -> (status int32 [n, k], fit f64 [n, k, 8], cov f64 [n, k, 3], info f64 [n, k, 3])."""
    heat = np.asarray(heat, np.float32)
    n, k = heat.shape[:2]
    status, fit = np.empty((n, k), np.int32), np.empty((n, k, 8))
    cov, info = np.empty((n, k, 3)), np.empty((n, k, 3))
    for i in range(n):
        for j in range(k):
            out = cov_plane(heat[i, j], None, cov_floor)
            status[i, j], fit[i, j], cov[i, j], info[i, j] = out["status"], out["fit"], out["cov"], out["info"]
    return status, fit, cov, info


# ---- two independent references, both scipy ---------------------------------------------------------------------------------------
def lsq_pcov(plane, idx):
    """scipy.optimize.least_squares on the (a, b, c) model from the kernel's start -> the centre block (cxx, cxy, cyy) of
    cost / (n - 7) (J^T J)^-1 with scipy's own Jacobian at its own solution."""
    x, cost, jac = G.scipy_fit(plane, idx)
    pc = np.linalg.inv(jac.T @ jac) * cost / (jac.shape[0] - P)
    return np.array([pc[1, 1], pc[1, 2], pc[2, 2]])


def _two_d_gaussian(xy, amplitude, xo, yo, sigma_x, sigma_y, theta, offset):
    """The model of the reference's test.py, restated: the (sigma_x, sigma_y, theta) parametrisation."""
    x, y = xy
    a = np.cos(theta) ** 2 / (2 * sigma_x ** 2) + np.sin(theta) ** 2 / (2 * sigma_y ** 2)
    b = -np.sin(2 * theta) / (4 * sigma_x ** 2) + np.sin(2 * theta) / (4 * sigma_y ** 2)
    c = np.sin(theta) ** 2 / (2 * sigma_x ** 2) + np.cos(theta) ** 2 / (2 * sigma_y ** 2)
    return (offset + amplitude * np.exp(-(a * (x - xo) ** 2 + 2 * b * (x - xo) * (y - yo) + c * (y - yo) ** 2))).ravel()


def curve_fit_pcov(plane, idx, sx, sy):
    """scipy.optimize.curve_fit on test.py's (sigma_x, sigma_y, theta) model over the same window -> pcov[1:3, 1:3] as (cxx, cxy,
    cyy).  (sx, sy) only start the search."""
    from scipy.optimize import curve_fit
    plane = np.asarray(plane, np.float32)
    H, W = plane.shape
    px, py = idx % W, idx // W
    ys, xs = np.mgrid[max(py - G.R, 0):min(py + G.R, H - 1) + 1, max(px - G.R, 0):min(px + G.R, W - 1) + 1]
    data = plane[ys, xs].astype(np.float64).ravel()
    _, pcov = curve_fit(_two_d_gaussian, (xs.astype(np.float64), ys.astype(np.float64)), data,
                        p0=(float(plane[py, px]), px, py, sx, sy, 0.1, 0.0), xtol=1e-14, ftol=1e-14, gtol=1e-14, maxfev=20000)
    return np.array([pcov[1, 1], pcov[1, 2], pcov[2, 2]])


def deviation(c, ref):
    """Largest component difference of two (cxx, cxy, cyy), relative to sqrt(cxx cyy) of the reference."""
    return float(np.max(np.abs(np.asarray(c) - np.asarray(ref))) / np.sqrt(ref[0] * ref[2]))


# ---- the fixtures the host and the GPU tests share ------------------------------------------------------------------------------------
# name -> (H, W, cx, cy, sx, sy, theta, amp, off, noise sigma, seed): noisy blobs the restatement accepts
NOISY = {
    "n-aniso": (16, 16, 7.6, 8.2, 2.0, 1.4, 1.0, 1.0, 0.0, 0.02, 11),                 # 2 % noise, sigma_x != sigma_y, rotated
    "n-aniso+offset": (16, 16, 8.3, 7.4, 1.3, 2.2, 0.4, 0.9, 0.2, 0.03, 12),         # with an offset, 3 %
    "n-sharp": (16, 16, 7.2, 8.7, 1.0, 1.4, 2.2, 1.0, 0.0, 0.01, 13),                 # sigma 1, 1 %
    "n-wide": (40, 40, 19.6, 20.3, 3.0, 2.2, 0.7, 1.0, 0.05, 0.05, 14),               # sigma 3 needs room, 5 %
    "n-border": (16, 16, 3.3, 8.4, 2.0, 1.5, 0.3, 1.0, 0.0, 0.02, 15),                # window clipped to 10 x 13
    "n-corner": (16, 16, 0.4, 0.3, 2.2, 1.8, 0.3, 1.0, 0.0, 0.01, 16),                # 7 x 7 window, n = 49
}


def noisy_plane(name):
    H, W, cx, cy, sx, sy, th, amp, off, sd, seed = NOISY[name]
    rng = np.random.default_rng(seed)
    return (G.blob(H, W, cx, cy, sx, sy, th, amp, off)[0] + rng.normal(0.0, sd * amp, (H, W))).astype(np.float32)


def guard_planes():
    """16 x 16 planes of the guard cases: name -> plane."""
    pl = {"clean": G.blob(16, 16, 7.6, 8.2, 2.0, 1.6, 1.0)[0],                        # noise-free: cov finite, below the floor
          "constant": np.full((16, 16), 0.25, np.float32),                             # status 2
          "outside": G.blob(16, 16, -3.0, 8.4, 2.5, 2.5, 0.0)[0]}                      # status 2: the centre outside the window
    pl["nan"] = pl["clean"].copy()
    pl["nan"][8, 7] = np.nan                                                           # status 3
    return pl
