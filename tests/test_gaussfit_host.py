"""The Gaussian-fit decoder without a GPU (include/esahrnet.h esahrnet_keypoints_gaussfit): the symbol, its argument errors
(reported before anything is enqueued, so they need no device), the Python entry points' checks, and the numpy restatement
tests/gaussfit_ref.py — which the GPU tests hold the kernel to — against two unrelated optimisers: scipy's trust-region least
squares on the same residuals, and curve_fit on the (sigma_x, sigma_y, theta) model of the reference's test.py."""
import ctypes as C
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correspond_ref as R  # noqa: E402
import gaussfit_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED = ["isotropic", "rotated", "rotated+offset", "noise", "border", "corner", "isotropic-2", "rotated-neg", "noise+offset",
            "isotropic-3", "rotated-3"]


@pytest.fixture(scope="module")
def fitted():
    """Every fixture plane through the restatement, once: {name: (plane, fit_plane's dict)}."""
    heat, names, _ = G.fixture_batches()
    out = {}
    for b in heat:
        for pl, name in zip(heat[b].reshape((-1,) + heat[b].shape[2:]), names[b]):
            out[name] = (pl, G.fit_plane(pl))
    return out


# ---- 1. the symbol and its argument checks -----------------------------------------------------------------------------------
def test_header_declares_and_lib_exports_the_entry():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esahrnet.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+esahrnet_keypoints_gaussfit\s*\(", header)
    from esa_pose_estimation_amd import _lib as L
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == L.ABI_VERSION
    assert "esahrnet_keypoints_gaussfit" in L.exported_symbols()
    assert hasattr(C.CDLL(L.LIB_PATH), "esahrnet_keypoints_gaussfit")
    lib = L.lib()
    assert lib.esahrnet_abi_version() == 6
    assert len(lib.esahrnet_keypoints_gaussfit.argtypes) == 11


def test_argument_errors_are_reported_before_anything_is_enqueued():
    """None of these calls reaches a launch: they return non-zero on a machine without a GPU, on pointers that are only numbers."""
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    p = 0x10000                                          # never dereferenced
    good = dict(heat=p, n=2, k=3, h=32, w=40, kp=p, idx=p, fit=p, status=p, hess=p)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.esahrnet_keypoints_gaussfit(a["heat"], a["n"], a["k"], a["h"], a["w"], a["kp"], a["idx"], a["fit"], a["status"],
                                             a["hess"], None)
        return rc, lib.esahrnet_last_error()

    for name in ("heat", "kp", "status"):
        rc, msg = call(**{name: None})
        assert rc != 0 and b"null" in msg, name
    for kw in (dict(n=0), dict(k=-1), dict(h=0), dict(w=0), dict(h=65536, w=65536), dict(n=65536, k=65536)):
        rc, msg = call(**kw)
        assert rc != 0 and b"bad shape" in msg, kw
    for name in ("heat", "kp", "idx", "status"):
        rc, msg = call(**{name: p + 2})
        assert rc != 0 and b"4-byte aligned" in msg, name
    for name in ("fit", "hess"):
        rc, msg = call(**{name: p + 4})
        assert rc != 0 and b"8-byte aligned" in msg, name


def test_the_kernel_keeps_its_arrays_in_registers():
    """The 7 x 7 system, its factor and the window live in arrays indexed by constants: no scratch memory, no spill, no LDS;
    two waves per SIMD is what 28 + 28 + 7 + 7 f64 values and three f64 pixel triples leave (build/resource_usage.json)."""
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    usage = json.load(open(b.USAGE))
    hits = [k for k in usage if k.startswith("keypoints_gaussfit.hip:") and "gaussfit_kernel" in k]
    assert len(hits) == 1, hits
    u = usage[hits[0]]
    print(hits[0], u)
    assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["lds"] == 0
    assert u["waves_per_simd"] >= 2


def test_python_argument_checks_need_no_gpu():
    import torch
    from esa_pose_estimation_amd import inference
    with pytest.raises(ValueError, match="4-D"):
        inference.gaussfit_keypoints(torch.zeros(3, 32, 40))
    with pytest.raises(RuntimeError, match="GPU only"):
        inference.gaussfit_keypoints(torch.zeros(1, 3, 32, 40))
    from esa_pose_estimation_amd import hrnet
    assert callable(hrnet.HighResolutionNet.keypoints_gaussfit)


def _testpy_abc(sigma_x, sigma_y, theta):
    """(a, b, c) of the reference's test.py, restated (the same three lines as in _two_d_gaussian below)."""
    a = np.cos(theta) ** 2 / (2 * sigma_x ** 2) + np.sin(theta) ** 2 / (2 * sigma_y ** 2)
    b = -np.sin(2 * theta) / (4 * sigma_x ** 2) + np.sin(2 * theta) / (4 * sigma_y ** 2)
    c = np.sin(theta) ** 2 / (2 * sigma_x ** 2) + np.cos(theta) ** 2 / (2 * sigma_y ** 2)
    return a, b, c


def test_sigma_theta_round_trips_through_the_reference_model():
    """(sigma_x, sigma_y, theta) -> test.py's (a, b, c) -> gaussfit_sigma_theta gives the triple back (modulo pi, the long axis
    first), and the triple it returns, put into test.py's model, is the function the (a, b, c) stand for."""
    from esa_pose_estimation_amd import inference
    triples = [(3.5, 1.5, 0.6), (3.5, 1.5, -1.2), (3.0, 1.0, 1.5), (1.5, 3.5, 0.6), (2.5, 2.0, 0.0), (3.0, 1.0, np.pi / 2),
               (1.2, 2.9, 2.8), (2.0, 1.9, -0.3)]
    rows, want = [], []
    for sx, sy, th in triples:
        f = np.array([0.8, 6.3, 5.6, 0.0, 0.0, 0.0, 0.1, 0.0])
        f[3:6] = _testpy_abc(sx, sy, th)
        rows.append(f)
        if sx < sy:                                       # the long axis is reported as sigma_x
            sx, sy, th = sy, sx, th + np.pi / 2
        want.append((sx, sy, th))
    rows, want = np.array(rows), np.array(want)
    sx, sy, th = inference.gaussfit_sigma_theta(rows)
    assert np.allclose(sx, want[:, 0], rtol=1e-12) and np.allclose(sy, want[:, 1], rtol=1e-12)
    dth = (th - want[:, 2] + np.pi / 2) % np.pi - np.pi / 2          # angles of an axis: modulo pi
    assert np.all(np.abs(dth) < 1e-9), dth
    assert np.all(th > -np.pi / 2) and np.all(th <= np.pi / 2) and np.all(sx >= sy)
    ys, xs = np.mgrid[0:13, 0:13].astype(np.float64)
    for f, x, y, t in zip(rows, sx, sy, th):
        A, x0, y0, a, b, c, off = f[:7]
        direct = off + A * np.exp(-(a * (xs - x0) ** 2 + 2 * b * (xs - x0) * (ys - y0) + c * (ys - y0) ** 2))
        assert np.allclose(_two_d_gaussian((xs, ys), A, x0, y0, x, y, t, off), direct.ravel(), rtol=1e-12, atol=1e-15)
    # the sign: test.py's theta is minus the geometric angle of the long axis, the angle of tests/gaussfit_ref.abc_of
    f = np.zeros(8)
    f[3:6] = G.abc_of(3.5, 1.5, 0.6)
    assert abs(float(inference.gaussfit_sigma_theta(f)[2]) + 0.6) < 1e-12
    f[3:6] = G.abc_of(2.0, 2.0, 0.0)
    sx, sy, th = inference.gaussfit_sigma_theta(f)
    assert sx == sy == 2.0 and np.isfinite(th)
    assert all(np.isnan(v) for v in inference.gaussfit_sigma_theta(np.full(8, np.nan)))


# ---- 2. the restatement against scipy on the same residuals -----------------------------------------------------------------
def test_statuses_of_the_fixtures(fitted):
    for name in ACCEPTED + [f"small-{i}" for i in range(6)]:
        assert fitted[name][1]["status"] == 0, name
    assert fitted["constant"][1]["status"] == 2 and np.isnan(fitted["constant"][1]["fit"]).all()
    assert fitted["nan"][1]["status"] == 3
    # the other rules: a finite fit with A > 0 whose centre is outside the window, or whose quadratic form is not positive
    for name in ("outside-x", "outside-corner"):
        out = fitted[name][1]
        A, x0, y0, a, b, c, _ = out["raw"]
        assert out["status"] == 2 and A > 0 and a > 0 and a * c - b * b > 0 and (x0 < -1 or y0 < -1), (name, out["raw"])
        assert np.isnan(out["fit"]).all()
    for name in ("saddle", "saddle-2"):
        out = fitted[name][1]
        A, x0, y0, a, b, c, _ = out["raw"]
        assert out["status"] == 2 and A > 0 and a < -1e-3 and a * c - b * b < -1e-4, (name, out["raw"])
        assert abs(x0 - 20) < 1 and abs(y0 - 15) < 1                         # the centre is inside: this rule alone rejects it
    two = fitted["two-peaks"]
    assert two[1]["idx"] == 12 * G.W + 15 and two[1]["status"] in (0, 2)       # starts at the first of the equal maxima
    print("two-peaks: status", two[1]["status"], "fit", two[1]["fit"])


def test_restatement_reaches_scipys_minimum(fitted):
    for name, (pl, out) in fitted.items():
        if out["status"] != 0:
            continue
        x_ref, c_ref, _ = G.scipy_fit(pl, out["idx"])
        r = G.model_residuals(out["fit"][:7], pl, out["idx"])
        c = float(r @ r)
        print(f"{name}: cost {c:.6e} (kernel order {out['fit'][7]:.6e}), scipy {c_ref:.6e}, iterations {out['iterations']}")
        assert c <= c_ref * (1 + 1e-6) + 1e-12, (name, c, c_ref)             # as deep a minimum as scipy's
        assert abs(out["fit"][7] - c) <= 1e-9 * c + 1e-20, name               # the cost it reports is that cost


def test_noise_free_centres_are_the_truth(fitted):
    _, names, truth = G.fixture_batches()
    for b in names:
        for name, tr in zip(names[b], truth[b]):
            if tr is None:
                continue
            out = fitted[name][1]
            x_ref = G.scipy_fit(fitted[name][0], out["idx"])[0]
            e = np.hypot(out["fit"][1] - tr[0], out["fit"][2] - tr[1])
            e_ref = np.hypot(x_ref[1] - tr[0], x_ref[2] - tr[1])
            print(f"{name}: centre error {e:.3e} px, scipy {e_ref:.3e} px")
            assert e <= 2 * e_ref + 1e-6, name


# ---- 3. the restatement against curve_fit on test.py's own model ------------------------------------------------------------
def _two_d_gaussian(xy, amplitude, xo, yo, sigma_x, sigma_y, theta, offset):
    """The model of the reference's test.py, restated: the (sigma_x, sigma_y, theta) parametrisation."""
    x, y = xy
    a = np.cos(theta) ** 2 / (2 * sigma_x ** 2) + np.sin(theta) ** 2 / (2 * sigma_y ** 2)
    b = -np.sin(2 * theta) / (4 * sigma_x ** 2) + np.sin(2 * theta) / (4 * sigma_y ** 2)
    c = np.sin(theta) ** 2 / (2 * sigma_x ** 2) + np.cos(theta) ** 2 / (2 * sigma_y ** 2)
    return (offset + amplitude * np.exp(-(a * (x - xo) ** 2 + 2 * b * (x - xo) * (y - yo) + c * (y - yo) ** 2))).ravel()


def _sigmas(abc):
    a, b, c = abc
    half, rad = 0.5 * (a + c), np.hypot(0.5 * (a - c), b)
    return np.array([np.sqrt(0.5 / (half - rad)), np.sqrt(0.5 / (half + rad))])      # long axis first


@pytest.mark.parametrize("cx,cy,sx,sy,theta,seed", [(17.3, 12.6, 3.0, 1.5, 0.6, 1), (22.8, 18.4, 1.4, 2.6, 2.0, 2),
                                                    (14.5, 15.5, 2.4, 1.8, -0.4, 3)])
def test_restatement_agrees_with_curve_fit_on_the_reference_model(cx, cy, sx, sy, theta, seed):
    """Blobs with sigma_x != sigma_y and 2 % noise, the 13 x 13 window of test.py.  Both fits minimise the same sum over the
    same family, so they must agree far inside their own uncertainty: the tolerance of each quantity is the sum of the two
    fits' standard errors, from curve_fit's pcov and from s^2 (J^T J)^-1 at the restatement's solution (the formula behind
    curve_fit's pcov), propagated to the sigmas through the numerical Jacobian of (a, b, c) -> (sigma_long, sigma_short)."""
    from scipy.optimize import curve_fit
    rng = np.random.default_rng(seed)
    plane = (G.blob(G.H, G.W, cx, cy, sx, sy, theta)[0] + rng.normal(0.0, 0.02, (G.H, G.W))).astype(np.float32)
    out = G.fit_plane(plane)
    assert out["status"] == 0
    idx = out["idx"]
    px, py = idx % G.W, idx // G.W
    ys, xs = np.mgrid[py - 6:py + 7, px - 6:px + 7]
    data = plane[ys, xs].astype(np.float64).ravel()
    popt, pcov = curve_fit(_two_d_gaussian, (xs.astype(np.float64), ys.astype(np.float64)), data,
                           p0=(float(plane[py, px]), px, py, max(sx, sy), min(sx, sy), 0.0, 0.0), xtol=1e-14, ftol=1e-14, gtol=1e-14)
    se_cf = np.sqrt(np.diag(pcov))
    # the restatement's covariance: s^2 (J^T J)^-1 with scipy's Jacobian of the (a, b, c) model at its solution
    fit = out["fit"]
    r = G.model_residuals(fit[:7], plane, idx)
    eps = 1e-7
    J = np.stack([(G.model_residuals(fit[:7] + eps * np.eye(7)[i], plane, idx) - r) / eps for i in range(7)], 1)
    cov = np.linalg.inv(J.T @ J) * (r @ r) / (len(r) - 7)
    se = np.sqrt(np.diag(cov))
    dS = np.stack([(_sigmas(fit[3:6] + eps * np.eye(3)[i]) - _sigmas(fit[3:6])) / eps for i in range(3)], 1)     # [2, 3]
    se_sig = np.sqrt(np.diag(dS @ cov[3:6, 3:6] @ dS.T))
    sig_cf = np.sort(np.abs(popt[3:5]))[::-1]
    se_sig_cf = se_cf[3:5][np.argsort(np.abs(popt[3:5]))[::-1]]
    print(f"centre: restatement ({fit[1]:.6f}, {fit[2]:.6f}) curve_fit ({popt[1]:.6f}, {popt[2]:.6f}) tolerance "
          f"({se[1] + se_cf[1]:.2e}, {se[2] + se_cf[2]:.2e}); sigmas {_sigmas(fit[3:6])} / {sig_cf} tolerance {se_sig + se_sig_cf}")
    assert abs(fit[1] - popt[1]) <= se[1] + se_cf[1] and abs(fit[2] - popt[2]) <= se[2] + se_cf[2]
    assert np.all(np.abs(_sigmas(fit[3:6]) - sig_cf) <= se_sig + se_sig_cf)
    assert np.hypot(fit[1] - cx, fit[2] - cy) < 0.1                              # and both sit on the blob


# ---- 4. the statistical property, on the CPU first ---------------------------------------------------------------------------
def test_fitted_sigma_is_closer_to_the_truth_than_the_final2_hessian():
    """Un-blurred anisotropic blobs of known Sigma: the fit's (2 [[a, b], [b, c]])^-1 against get_final2's -H^-1 - 4 I (the
    Hessian of the blurred log heat-map, its blur taken off again).  Measured with the restatements (12 blobs): median relative
    Frobenius error printed below; only the ordering of the two medians is asserted."""
    planes, true = G.aniso_planes()
    fit = np.stack([G.fit_plane(p)["fit"] for p in planes.reshape(-1, G.H, G.W)])
    assert np.isfinite(fit).all()
    e_fit = G.sigma_error(np.stack(G.sigma_of(fit[:, 3], fit[:, 4], fit[:, 5]), 1), true)
    hess, applied = R.hessian(planes)
    assert applied.all()
    h = hess.reshape(-1, 3)
    det = h[:, 0] * h[:, 2] - h[:, 1] ** 2
    est = np.stack([-h[:, 2] / det - 4.0, h[:, 1] / det, -h[:, 0] / det - 4.0], 1)       # -H^-1 - 4 I
    e_f2 = G.sigma_error(est, true)
    print(f"median relative error of Sigma: fit {np.median(e_fit):.3e}, get_final2 Hessian {np.median(e_f2):.3e}")
    assert np.median(e_fit) <= np.median(e_f2)
