"""The covariance of the Gaussian fit's centre without a GPU (include/esahrnet.h esahrnet_keypoints_gaussfit_cov and its two
siblings): the symbols, their argument errors (reported before anything is enqueued, so they need no device), the resource
figures of the new kernels, the Python entry points' checks, and the numpy restatement tests/gaussfit_cov_ref.py — which the GPU
tests hold the kernels to — against two scipy references that calibrate each other: least_squares on the (a, b, c) model and
curve_fit on the (sigma_x, sigma_y, theta) model of the reference's test.py."""
import ctypes as C
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussfit_cov_ref as V  # noqa: E402
import gaussfit_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"esahrnet_keypoints_gaussfit_cov": 14, "esahrnet_forward_keypoints_gaussfit_cov": 16,
           "esahrnet_frames_keypoints_gaussfit_cov": 27}
SIBLINGS = {"esahrnet_keypoints_gaussfit_cov": "esahrnet_keypoints_gaussfit",
            "esahrnet_forward_keypoints_gaussfit_cov": "esahrnet_forward_keypoints_gaussfit",
            "esahrnet_frames_keypoints_gaussfit_cov": "esahrnet_frames_keypoints_gaussfit"}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


# ---- 1. the symbols and their argument checks ------------------------------------------------------------------------------------
def test_header_declares_lib_exports_and_binds_the_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esahrnet.h")).read(), flags=re.S)
    from esa_pose_estimation_amd import _lib as L
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == L.ABI_VERSION
    lib, raw = L.lib(), C.CDLL(L.LIB_PATH)
    assert lib.esahrnet_abi_version() == 6

    def params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    for name, nargs in ENTRIES.items():
        got, sib = params(name), params(SIBLINGS[name])
        assert len(got) == nargs == len(sib) + 3, name
        assert name in L.exported_symbols() and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
        # the sibling's declaration with three additions before the workspace arguments / the stream
        add = ["void* cov_dev", "void* info_dev", "double cov_floor"]
        at = got.index(add[0])
        assert got[at:at + 3] == add and got[:at] + got[at + 3:] == sib, name
        assert got[at + 3].split()[-1] in ("stream", "ws_dev"), name
        assert getattr(lib, name).argtypes[at:at + 3] == [C.c_void_p, C.c_void_p, C.c_double], name


def _handle(lib, L, variant=0, cin=1, k=11):
    from esa_pose_estimation_amd import config, hrnet
    widths = (16, 16, 32, 64) if variant else (16, 32, 64, 128)
    cfg = hrnet._cfg_struct(config.make_config(widths=widths), cin, k, variant, "fp32")
    h = C.c_void_p()
    L.check(lib.esahrnet_create(C.byref(cfg), 0, C.byref(h)))
    return h


def test_argument_errors_are_reported_before_anything_is_enqueued():
    """None of these calls reaches a launch: they return non-zero on a machine without a GPU, on pointers that are only numbers.
    The siblings' refusals with the siblings' words, then the three additions: a misaligned cov_dev / info_dev, a negative or
    NaN cov_floor.  NULL for cov_dev and info_dev is no error."""
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    err = lib.esahrnet_last_error
    p = 0x10000                                          # never dereferenced
    nan = float("nan")

    def kg(heat=p, n=2, k=3, h=32, w=40, kp=p, idx=p, fit=p, status=p, hess=p, cov=p, info=p, floor=1e-6):
        return lib.esahrnet_keypoints_gaussfit_cov(heat, n, k, h, w, kp, idx, fit, status, hess, cov, info, floor, None)

    for name in ("heat", "kp", "status"):
        assert kg(**{name: None}) != 0 and b"null" in err(), name
    for kw in (dict(n=0), dict(k=-1), dict(h=0), dict(w=0), dict(h=65536, w=65536), dict(n=65536, k=65536)):
        assert kg(**kw) != 0 and b"bad shape" in err(), kw
    for name in ("heat", "kp", "idx", "status"):
        assert kg(**{name: p + 2}) != 0 and b"4-byte aligned" in err(), name
    for name in ("fit", "hess", "cov", "info"):
        assert kg(**{name: p + 4}) != 0 and b"8-byte aligned" in err(), name
    for bad in (-1e-6, -1.0, nan, float("-inf")):
        assert kg(floor=bad) != 0 and b"cov_floor" in err(), bad
        assert kg(floor=bad, cov=None, info=None) != 0 and b"cov_floor" in err(), bad

    h = _handle(lib, L)
    try:
        def fwd(hh=h, x=p, n=2, kp=p, idx=p, fit=p, status=p, hess=p, cov=p, info=p, floor=1e-6, ws=p, wsb=1 << 40):
            return lib.esahrnet_forward_keypoints_gaussfit_cov(hh, x, n, 48, 80, kp, idx, fit, status, hess, cov, info, floor, ws, wsb,
                                                               None)
        for name in ("hh", "x", "kp", "status", "ws"):
            assert fwd(**{name: None}) != 0 and b"null" in err(), name
        for name in ("kp", "idx", "status"):
            assert fwd(**{name: p + 2}) != 0 and b"4-byte aligned" in err(), name
        for name in ("fit", "hess", "cov", "info"):
            assert fwd(**{name: p + 4}) != 0 and b"8-byte aligned" in err(), name
        for bad in (-1e-6, nan):
            assert fwd(floor=bad) != 0 and b"cov_floor" in err(), bad
        assert fwd() != 0 and b"commit" in err()                                  # the handle has no weights
        assert fwd(cov=None, info=None) != 0 and b"commit" in err()
        assert fwd(n=0) != 0

        def fr(hh=h, m=1, nframes=1, fmt=0, rule=0, std=0.229, kp=p, status=p, fit=p, cov=p, info=p, floor=1e-6, ws=p, wsb=1 << 40):
            return lib.esahrnet_frames_keypoints_gaussfit_cov(hh, p, nframes, 1200, 1920, fmt, p, None, m, 256, rule, 0.485, std, kp,
                                                              None, fit, status, None, p, p, p, cov, info, floor, ws, wsb, None)
        for name in ("hh", "kp", "status", "ws"):
            assert fr(**{name: None}) != 0 and b"null" in err(), name
        assert fr(m=0) != 0 and fr(m=-1) != 0
        assert fr(rule=3) != 0 and b"rule" in err()
        assert fr(fmt=5) != 0 and b"pixel_format" in err()
        assert fr(std=-1.0) != 0 and b"stdv" in err()
        assert fr(m=2) != 0 and b"frame index" in err()
        for name in ("cov", "info"):
            assert fr(**{name: p + 4}) != 0 and b"8-byte aligned" in err(), name
        for bad in (-1e-6, nan):
            assert fr(floor=bad) != 0 and b"cov_floor" in err(), bad
        assert fr() != 0 and b"commit" in err()
    finally:
        lib.esahrnet_destroy(h)


def test_new_kernels_stay_in_registers():
    """The covariance pass adds no scratch memory, no spill and no LDS: the two kernels of keypoints_gaussfit_cov.hip (three
    instantiations) have none at all; the VALU finish keeps the LDS of its sibling (the staged inputs and the window, which the
    solver only reads) and not a byte more.  Two waves per SIMD, as the fit without the pass."""
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    assert "keypoints_gaussfit_cov.hip" in b.SOURCES
    usage = json.load(open(b.USAGE))
    new = [k for k in usage if "gfcov" in k]
    assert len(new) == 5, new                   # NCHW, NHWC f32 and split-bf16, the VALU finish, the loader's NaN rows
    for k in new:
        u = usage[k]
        print(k, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, k
    plain = [k for k in new if k.startswith("keypoints_gaussfit_cov.hip:")]
    assert len(plain) == 3
    for k in plain:
        assert usage[k]["lds"] == 0 and usage[k]["waves_per_simd"] >= 2, k
    fin = [k for k in new if "final_gfcov_finish_kernel" in k]
    sib = [k for k in usage if "final_gf_finish_kernel" in k]
    assert len(fin) == 1 and len(sib) == 1
    assert usage[fin[0]]["lds"] == usage[sib[0]]["lds"] and usage[fin[0]]["waves_per_simd"] >= 2
    inv = [k for k in new if "mark_invalid_gfcov_kernel" in k]
    assert len(inv) == 1 and usage[inv[0]]["lds"] == 0


# ---- 2. Python ----------------------------------------------------------------------------------------------------------------------
def test_python_argument_checks_need_no_gpu():
    from esa_pose_estimation_amd import config, inference, pipeline, seg_hrnet2
    assert inference.check_weights("covariance", "gaussfit") == 1                  # the mode of esahrnet_correspondences
    for refine in ("get_final", "get_final2"):
        with pytest.raises(ValueError, match="gaussfit"):
            inference.check_weights("covariance", refine)
    with pytest.raises(ValueError, match="gaussfit"):
        inference.check_weights("covariance")
    assert inference.check_weights("peak", "gaussfit") == 0 and inference.check_weights("hessian", "gaussfit") == 1
    with pytest.raises(ValueError, match="4-D"):
        inference.gaussfit_keypoints(torch.zeros(3, 32, 40), return_cov=True)
    for bad in (-1.0, float("nan"), "x", None):
        with pytest.raises(ValueError, match="cov_floor"):
            inference.gaussfit_keypoints(torch.zeros(1, 3, 32, 40), return_cov=True, cov_floor=bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        inference.gaussfit_keypoints(torch.zeros(1, 3, 32, 40), return_cov=True)
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64))).eval()
    with pytest.raises(ValueError, match="cov_floor"):
        net.keypoints_gaussfit(torch.zeros(1, 1, 32, 32), return_cov=True, cov_floor=-1e-9)
    with pytest.raises(ValueError, match="device_select"):
        pipeline.estimate_poses(net, None, None, None, None, refine="gaussfit", weights="covariance")
    with pytest.raises(ValueError, match="gaussfit"):
        pipeline.estimate_poses(net, None, None, None, None, refine="get_final2", weights="covariance", device_select=True)
    with pytest.raises(ValueError, match="gaussfit"):
        net.frames_to_correspondences(torch.zeros(1, 64, 64, dtype=torch.uint8), [[0, 0, 9, 9]], refine="get_final2",
                                      weights="covariance")
    with pytest.raises(ValueError, match="cov_floor"):
        net.frames_to_correspondences(torch.zeros(1, 64, 64, dtype=torch.uint8), [[0, 0, 9, 9]], refine="gaussfit",
                                      weights="covariance", cov_floor=float("nan"))
    # the packed record: existing callers get the layout they got; with cov the two f64 parts follow hess, nothing overlaps
    for m, k in ((1, 11), (5, 11), (3, 30)):
        assert inference.packed_layout(m, k, True, cov=False) == inference.packed_layout(m, k, True)
        assert inference.packed_layout(m, k, False, cov=False) == inference.packed_layout(m, k)
        lay = inference.packed_layout(m, k, True, cov=True)
        end = 0
        for name, size in (("rates", 8), ("fit", 8), ("hess", 8), ("cov", 8), ("info", 8), ("kp", 4), ("boxes", 4), ("valid", 4),
                           ("idx", 4), ("status", 4)):
            off, nbytes = lay[name]
            assert off == end and off % size == 0 and nbytes > 0, name
            end = off + nbytes
        assert lay["total"] == (0, end) and lay["cov"][1] == lay["info"][1] == 24 * m * k
    with pytest.raises(ValueError, match="gaussfit"):
        inference.packed_layout(1, 11, False, cov=True)


# ---- 3. the restatement against scipy ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy():
    """Every noisy fixture through the restatement, once: {name: (plane, cov_plane's dict)}."""
    return {name: (pl, V.cov_plane(pl)) for name, pl in ((n, V.noisy_plane(n)) for n in V.NOISY)}


def test_restatement_accepts_every_fixture_with_the_fit_of_gaussfit_ref(noisy):
    """No plane may be skipped below: every fixture is accepted, with the parameters and the cost gaussfit_ref.fit_plane returns,
    bit for bit (the pass starts from the same fit), a finite covariance above the reference's floor, and a finite info."""
    shapes = set()
    for name, (pl, out) in noisy.items():
        ref = G.fit_plane(pl)
        assert out["status"] == 0 == ref["status"], name
        assert out["idx"] == ref["idx"] and out["fit"].tobytes() == ref["fit"].tobytes(), name
        assert np.isfinite(out["cov"]).all() and out["cov"][0] > V.COV_FLOOR and out["cov"][2] > V.COV_FLOOR, (name, out["cov"])
        assert np.isfinite(out["info"]).all(), name
        shapes.add(int(G.window(pl, out["idx"])[3].sum()))
    assert {169, 49} <= shapes and any(s not in (169, 49) for s in shapes), shapes      # full, corner (7 x 7), clipped at a border
    sd = sorted(V.NOISY[n][9] for n in V.NOISY)
    assert sd[0] == 0.01 and sd[-1] == 0.05


@pytest.mark.parametrize("name", list(V.NOISY))
def test_restatement_lies_between_the_two_scipy_references(noisy, name):
    """least_squares on the (a, b, c) model and curve_fit on test.py's (sigma_x, sigma_y, theta) model minimise the same sum, so
    their centre blocks of pcov differ by their own convergence and rounding alone: that distance is the yardstick.  The
    restatement may lie no further from least_squares' than curve_fit's does (plus 1e-12 relative), and within twice that
    distance of curve_fit's.  Deviations relative to sqrt(cxx cyy)."""
    pl, out = noisy[name]
    cfg = V.NOISY[name]
    lsq = V.lsq_pcov(pl, out["idx"])
    cf = V.curve_fit_pcov(pl, out["idx"], cfg[4], cfg[5])
    d_ref, d_lsq, d_cf = V.deviation(cf, lsq), V.deviation(out["cov"], lsq), V.deviation(out["cov"], cf)
    print(f"{name}: cov {out['cov']}  restatement - least_squares {d_lsq:.2e}, restatement - curve_fit {d_cf:.2e}, "
          f"curve_fit - least_squares {d_ref:.2e}")
    assert d_lsq <= d_ref + 1e-12, (d_lsq, d_ref)
    assert d_cf <= 2 * d_ref + 1e-12, (d_cf, d_ref)


def test_predicted_covariance_is_calibrated():
    """One blob, M = 200 independent noise draws: the empirical covariance of the fitted centres against the mean predicted cov.
    Each diagonal ratio within 1 +- 4 sqrt(2 / (M - 1)) = +- 0.40, four standard errors of a variance estimated from M
    Gaussian samples."""
    M = 200
    rng = np.random.default_rng(777)
    clean = G.blob(16, 16, 7.6, 8.2, 2.0, 1.4, 1.0)[0].astype(np.float64)
    centres, covs = [], []
    for _ in range(M):
        out = V.cov_plane((clean + rng.normal(0.0, 0.03, clean.shape)).astype(np.float32))
        assert out["status"] == 0
        centres.append(out["fit"][1:3])
        covs.append(out["cov"])
    emp = np.cov(np.array(centres).T)
    pred = np.mean(covs, 0)
    tol = 4 * np.sqrt(2.0 / (M - 1))
    rx, ry = emp[0, 0] / pred[0], emp[1, 1] / pred[2]
    print(f"empirical {emp[0, 0]:.4e} {emp[0, 1]:.4e} {emp[1, 1]:.4e}  predicted {pred}  ratios {rx:.3f} {ry:.3f} (1 +- {tol:.2f})")
    assert abs(rx - 1) <= tol and abs(ry - 1) <= tol


# ---- 4. the guards -----------------------------------------------------------------------------------------------------------------------
def test_guard_cases():
    pl = V.guard_planes()
    clean = V.cov_plane(pl["clean"])
    assert clean["status"] == 0 and np.isfinite(clean["cov"]).all()
    assert 0 < clean["cov"][0] < 1e-6 and 0 < clean["cov"][2] < 1e-6, clean["cov"]           # f32 rounding is all the noise there is
    assert np.isnan(clean["info"]).all()                                                  # below the reference's floor
    assert np.isfinite(V.cov_plane(pl["clean"], cov_floor=0.0)["info"]).all()
    for name, st in (("constant", 2), ("outside", 2), ("nan", 3)):
        out = V.cov_plane(pl[name])
        assert out["status"] == st and np.isnan(out["cov"]).all() and np.isnan(out["info"]).all(), name
    # n = 6 pixels, 7 parameters: dof <= 0, whatever the fit's status
    out = V.cov_plane(G.blob(2, 3, 1.2, 0.6, 1.0, 1.0, 0.0)[0])
    assert np.isnan(out["cov"]).all() and np.isnan(out["info"]).all()
    # the floor acts on cxx alone, and info is -cov^-1
    c = np.array([[2e-6, 0.0, 5e-7], [5e-7, 0.0, 2e-6], [4e-4, 1e-4, 9e-4], [1e-4, 2e-4, 1e-4], [np.nan, 0.0, 1.0]])
    i = V.info_of(c)
    assert np.isfinite(i[0]).all() and np.isnan(i[1]).all() and np.isnan(i[3]).all() and np.isnan(i[4]).all()
    m = -np.linalg.inv(np.array([[4e-4, 1e-4], [1e-4, 9e-4]]))
    assert np.allclose(i[2], [m[0, 0], m[0, 1], m[1, 1]], rtol=1e-13, atol=0)
