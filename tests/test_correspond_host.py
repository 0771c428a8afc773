"""The host side of the correspondence stage (include/esahrnet.h esahrnet_pnp_batch_w, pnp.cpnp_m with 2x2 weights): the
full-weight refinement with (peak, 0, peak) rows is the scalar path bit for bit, with random SPD weights it reaches the minimum
an unrelated optimiser finds, both weight modes recover noise-free poses, and on anisotropic keypoint noise the information-
matrix weight is measured against the peak weight.  Pure host code: runs without a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_pnp_native as TPN  # noqa: E402  (its scene, its seeds and its independent checker's pattern)

from esa_pose_estimation_amd import inference, pnp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = TPN.K
ENTRIES = ["esahrnet_keypoints_final2_hess", "esahrnet_forward_keypoints_final2_hess", "esahrnet_correspondences",
           "esahrnet_frames_correspondences_workspace_bytes", "esahrnet_frames_correspondences", "esahrnet_pnp_batch_w"]
NATIVE_CASES = [(11, 0.0, 0, 0.0, 11), (11, 0.5, 0, 0.0, 11), (30, 0.7, 4, 0.3, 12), (11, 0.5, 2, 0.0, 11), (6, 0.3, 0, 0.0, 24)]


def host_record(kp, boxes, rates, thresh, min_k):
    """What esahrnet_correspondences writes in mode 0, from the host rule: inference.select_keypoints + crop_to_image."""
    n, k = kp.shape[:2]
    count = np.zeros(n, np.int32)
    order = np.full((n, k), -1, np.int32)
    pts = np.zeros((n, k, 2))
    w = np.zeros((n, k, 3))
    for i in range(n):
        idxs = inference.select_keypoints(kp[i, :, 2], thresh, min_k)
        c = len(idxs)
        count[i] = c
        order[i, :c] = idxs
        pts[i, :c] = inference.crop_to_image(kp[i, :, :2].astype(np.float64), rates[i], boxes[i][0], boxes[i][1])[idxs]
        w[i, :c, 0] = w[i, :c, 2] = kp[i, idxs, 2]
    return count, order, pts, w


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- 1. (peak, 0, peak) is the scalar path, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("k,noise,outliers,thresh,min_k", NATIVE_CASES)
def test_peak_rows_equal_the_scalar_path_bit_for_bit(k, noise, outliers, thresh, min_k):
    rng = np.random.default_rng(k * 100 + outliers)                         # test_pnp_native's seeds
    n = 12
    kp3d, kp, boxes, rates, _ = TPN._scene(rng, n, k, noise, outliers)
    q0, t0 = pnp.keypoints_to_pose_batch(kp, kp3d, K, boxes, rates, thresh=thresh, min_k=min_k, threads=3)
    count, order, pts, w = host_record(kp, boxes, rates, thresh, min_k)
    assert count.tolist() == [min(k, max(int((kp[i, :, 2] > thresh).sum()), min_k)) for i in range(n)]
    q1, t1 = pnp.correspondences_to_pose_batch(pts, w, count, order, kp3d, K, threads=2)
    assert np.isfinite(q0).all() and np.isfinite(t0).all()
    assert np.array_equal(_bits(q0), _bits(q1)) and np.array_equal(_bits(t0), _bits(t1))
    # the numpy LM: weights [n, 3] = (peak, 0, peak) against weights [n]
    for i in range(0, n, 4):
        c = count[i]
        p3d, p2d, mav = kp3d[order[i, :c]], pts[i, :c], w[i, :c, 0]
        Rt = pnp.pnp(p3d, p2d, K)
        cam = np.concatenate([pnp.rodrigues_inv(Rt[:, :3]), Rt[:, 3]])
        a = pnp.cpnp_m(p3d, p2d, mav, K, cam)
        b = pnp.cpnp_m(p3d, p2d, w[i, :c], K, cam)
        assert np.array_equal(_bits(a), _bits(b)), i


def test_pnp_batch_w_argument_checks_and_short_rows():
    from esa_pose_estimation_amd import _lib
    rng = np.random.default_rng(5)
    kp3d, kp, boxes, rates, _ = TPN._scene(rng, 3, 8, 0.0, 0)
    count, order, pts, w = host_record(kp, boxes, rates, 0.0, 8)
    count[1] = 3                                                             # fewer than 4 points: NaN, not a crash
    q, t = pnp.correspondences_to_pose_batch(pts, w, count, order, kp3d, K)
    assert np.isnan(q[1]).all() and np.isnan(t[1]).all() and np.isfinite(q[[0, 2]]).all()
    count[1] = 9
    with pytest.raises(_lib.EsaHrnetError, match="count"):
        pnp.correspondences_to_pose_batch(pts, w, count, order, kp3d, K)
    count[1] = 8
    order[2, 5] = 8
    with pytest.raises(_lib.EsaHrnetError, match="order"):
        pnp.correspondences_to_pose_batch(pts, w, count, order, kp3d, K)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        pnp.cpnp_m(kp3d, pts[0], np.ones((8, 2)), K, np.zeros(6))


# ---- 2. random SPD weights: an unrelated optimiser on the same residuals ------------------------------------------------------
def _spd(rng, n, lo=0.3, hi=1.5):
    """n random symmetric positive definite 2x2 matrices as rows (wxx, wxy, wyy)."""
    th = rng.uniform(0, np.pi, n)
    l1, l2 = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    c, s = np.cos(th), np.sin(th)
    return np.stack([l1 * c * c + l2 * s * s, (l1 - l2) * c * s, l1 * s * s + l2 * c * c], 1)


def _full_residuals(x, p3d, p2d, w):
    """uncertainty_pnp.cpp:17-31, built from scipy's Rotation: no line of pnp.py or pnp_host.hip is involved."""
    from scipy.spatial.transform import Rotation
    pc = Rotation.from_rotvec(x[:3]).apply(p3d) + x[3:]
    dx = K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2] - p2d[:, 0]
    dy = K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2] - p2d[:, 1]
    return np.stack([w[:, 0] * dx + w[:, 1] * dy, w[:, 1] * dx + w[:, 2] * dy], 1).ravel()


@pytest.mark.parametrize("k,noise", [(11, 0.0), (11, 0.7), (30, 1.5)])
def test_full_weight_refinement_reaches_scipys_minimum(k, noise):
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(900 + k)
    n = 8
    kp3d, kp, boxes, rates, poses = TPN._scene(rng, n, k, noise, 0)
    count, order, pts, _ = host_record(kp, boxes, rates, 0.0, k)
    w = np.stack([_spd(rng, k) for _ in range(n)])
    q_nat, t_nat = pnp.correspondences_to_pose_batch(pts, w, count, order, kp3d, K, threads=2)
    for i in range(n):
        p3d = kp3d[order[i]]
        Rt, tt = poses[i]
        cam0 = np.concatenate([Rotation.from_matrix(Rt).as_rotvec() + rng.normal(0, 0.01, 3), tt * (1 + rng.normal(0, 0.01, 3))])
        sol = least_squares(_full_residuals, cam0, args=(p3d, pts[i], w[i]), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                            x_scale="jac", max_nfev=2000)
        x_ref, cost_ref = sol.x, float(sol.fun @ sol.fun)
        Rt0 = pnp.pnp(p3d, pts[i], K)
        cam = pnp.cpnp_m(p3d, pts[i], w[i], K, np.concatenate([pnp.rodrigues_inv(Rt0[:, :3]), Rt0[:, 3]]))
        q_np, t_np = pnp.rotation_to_quat_wxyz(pnp.rodrigues(cam[:3])), cam[3:]
        q_ref = Rotation.from_rotvec(x_ref[:3]).as_quat()                               # [x, y, z, w]
        q_ref = np.array([q_ref[3], q_ref[0], q_ref[1], q_ref[2]])
        for name, (q, t) in (("native", (q_nat[i], t_nat[i])), ("numpy", (q_np, t_np))):
            rv = Rotation.from_quat([q[1], q[2], q[3], q[0]]).as_rotvec()
            r = _full_residuals(np.concatenate([rv, t]), p3d, pts[i], w[i])
            c = float(r @ r)
            assert c <= cost_ref * (1 + 1e-6) + 1e-12, (name, i, c, cost_ref)           # as deep a minimum as scipy's
            s = pnp.speed_score(q, t, q_ref, x_ref[3:])[0]
            assert s < (1e-6 if noise == 0 else 2e-4), (name, i, s)                     # and the same pose


# ---- 3. noise-free poses are recovered in both modes --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["peak", "hessian"])
def test_noise_free_poses_are_recovered(mode):
    rng = np.random.default_rng(31)
    n, k = 12, 11
    kp3d, kp, boxes, rates, poses = TPN._scene(rng, n, k, 0.0, 0)
    count, order, pts, w = host_record(kp, boxes, rates, 0.0, k)
    if mode == "hessian":
        w = np.stack([_spd(rng, k, 0.05, 2.0) for _ in range(n)])
        w[:, 3] = 0.0                                        # a keypoint whose Hessian was unusable: no weight, still a point
    q, t = pnp.correspondences_to_pose_batch(pts, w, count, order, kp3d, K)
    for i in range(n):
        Rt, tt = poses[i]
        assert pnp.speed_score(q[i], t[i], pnp.rotation_to_quat_wxyz(Rt), tt)[0] < 1e-6, i


# ---- 4. anisotropic keypoint noise: information-matrix weights against peak weights -------------------------------------------
def anisotropic_scores(seed=2024, n=200, k=11):
    """n seeded poses, every keypoint displaced by a draw from its OWN covariance (sigma 0.2 .. 4 px along a random axis, 0.2
    .. 0.6 px across it).  "hessian": w = Sigma^(-1/2), the weight the get_final2 Hessian stands for; "peak": the scalar peak
    (here uninformative: uniform 0.3 .. 1, as in test_pnp_native's scene).  -> the two arrays of SPEED scores."""
    rng = np.random.default_rng(seed)
    kp3d = rng.uniform(-0.6, 0.6, (k, 3))
    pts, wp, wh, truth = np.empty((n, k, 2)), np.zeros((n, k, 3)), np.empty((n, k, 3)), []
    for i in range(n):
        R = pnp.rodrigues(rng.uniform(-1.2, 1.2, 3))
        t = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(4.0, 14.0)])
        th, s1, s2 = rng.uniform(0, np.pi, k), rng.uniform(0.2, 4.0, k), rng.uniform(0.2, 0.6, k)
        c, s = np.cos(th), np.sin(th)
        z = rng.standard_normal((k, 2))
        e1, e2 = s1 * z[:, 0], s2 * z[:, 1]                                   # along / across the axis
        pts[i] = pnp.project(kp3d, R, t, K) + np.stack([c * e1 - s * e2, s * e1 + c * e2], 1)
        i1, i2 = 1 / s1, 1 / s2                                               # Sigma^(-1/2) = U diag(1 / sigma) U^T
        wh[i] = np.stack([i1 * c * c + i2 * s * s, (i1 - i2) * c * s, i1 * s * s + i2 * c * c], 1)
        wp[i, :, 0] = wp[i, :, 2] = rng.uniform(0.3, 1.0, k)
        truth.append((pnp.rotation_to_quat_wxyz(R), t))
    count = np.full(n, k, np.int32)
    order = np.tile(np.arange(k, dtype=np.int32), (n, 1))
    out = {}
    for name, w in (("peak", wp), ("hessian", wh)):
        q, t = pnp.correspondences_to_pose_batch(pts, w, count, order, kp3d, K)
        out[name] = np.array([pnp.speed_score(q[i], t[i], *truth[i])[0] for i in range(n)])
    return out


def test_information_weights_beat_peak_weights_on_anisotropic_noise():
    """Measured on the CPU (seed 2024, 200 poses, 11 keypoints): median SPEED score 0.00864 with the peak weight, 0.00265 with
    w = Sigma^(-1/2) — a factor 3.3, and the per-pose score is lower in 96 % of the poses: a clear margin on this seed set, so
    the assertion stands: the anisotropic weight must not be worse than the scalar one."""
    s = anisotropic_scores()
    mp, mh = float(np.median(s["peak"])), float(np.median(s["hessian"]))
    print(f"median SPEED score: peak {mp:.5f}, hessian {mh:.5f}; hessian lower in {np.mean(s['hessian'] < s['peak']):.0%}")
    assert np.isfinite(s["peak"]).all() and np.isfinite(s["hessian"]).all()
    assert mh <= mp


# ---- 5. symbols and ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_exports_the_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esahrnet.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    from esa_pose_estimation_amd import _lib as L
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == L.ABI_VERSION
    assert set(ENTRIES) <= set(L.exported_symbols())
    raw = C.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
    lib = L.lib()
    assert lib.esahrnet_abi_version() == 6
    assert len(lib.esahrnet_frames_correspondences.argtypes) == 29 and len(lib.esahrnet_correspondences.argtypes) == 15
    assert len(lib.esahrnet_pnp_batch_w.argtypes) == 11


def test_python_argument_checks_need_no_gpu():
    with pytest.raises(ValueError, match="get_final2"):
        inference.check_weights("hessian", "get_final")
    with pytest.raises(ValueError, match="weights must be"):
        inference.check_weights("variance")
    assert inference.check_weights("peak", "get_final") == 0 and inference.check_weights("hessian") == 1
