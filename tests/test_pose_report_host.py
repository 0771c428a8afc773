"""What the native pose solve reports (include/esahrnet.h: enum esahrnet_pose_report, esahrnet_pnp_batch_ex,
esahrnet_pnp_batch_w_ex; pnp.PoseReport), without a GPU: the report takes no part in the solve; its fields against the numpy
statement pnp.pose_report and the RANSAC bookkeeping of pnp.solve_pnp_ransac; that statement's Jacobian against scipy's finite
differences; the covariance against the scatter of 4000 noisy solves; its two scale conventions; the statuses and flags; the
gates of pipeline.estimate_poses; the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from esa_pose_estimation_amd import _lib as L
from esa_pose_estimation_amd import inference, pipeline, pnp, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.asarray(synth.ESA_CAMERA, np.float64)              # fx = fy = 3003.41297, cx = 960, cy = 600
EPS = np.finfo(np.float64).eps
REAL = ("cost", "rms_px", "max_px", "min_depth", "s2")
SHORT = (5, 17, 40)                                       # images of the batch that have 3 points


# ---- the seeded batch of tests 1 and 2: 64 images, 11 keypoints, sigma 0.5 px, three images with 3 points -----------------
def _batch(m=64, k=11, sigma=0.5, seed=0):
    """-> kp3d [k,3], the correspondence record (pts, w, count, order: a random rank order per image, random symmetric 2x2
    weights with an off-diagonal term) and the same scene as keypoint rows (kp f32 [m,k,3], boxes_xy, rates)."""
    rng = np.random.default_rng(seed)
    scene = synth.make_scene(m, k, seed=seed)
    uv = scene["uv"] + rng.normal(0, sigma, scene["uv"].shape)
    order = np.stack([rng.permutation(k) for _ in range(m)]).astype(np.int32)
    pts = np.take_along_axis(uv, order[:, :, None].astype(np.int64), 1)
    a, b, c = rng.uniform(0.5, 2.0, (m, k)), rng.uniform(-0.3, 0.3, (m, k)), rng.uniform(0.5, 2.0, (m, k))
    w = np.stack([a, b, c], 2)
    count = np.full(m, k, np.int32)
    count[list(SHORT)] = 3
    # keypoint rows in crops of rate 0.5 at integer origins (kp * 2 + origin is exact in f64); 3 peaks above the threshold
    # in the short images
    boxes_xy = rng.integers(0, 40, (m, 2)).astype(np.int32)
    rates = np.full(m, 0.5)
    peak = rng.uniform(0.6, 1.0, (m, k))
    for i in SHORT:
        peak[i, 3:] = rng.uniform(0.1, 0.4, k - 3)
    kp = np.concatenate([(uv - boxes_xy[:, None, :]) * 0.5, peak[:, :, None]], 2).astype(np.float32)
    return dict(kp3d=scene["kp3d"], pts=pts, w=w, count=count, order=order, kp=kp, boxes_xy=boxes_xy, rates=rates, m=m, k=k)


@pytest.fixture(scope="module")
def batch():
    return _batch()


def _solve_w(b, threads, report=True):
    return pnp.correspondences_to_pose_batch(b["pts"], b["w"], b["count"], b["order"], b["kp3d"], K, threads, report=report)


def _solve_kp(b, threads, report=True):
    return pnp.keypoints_to_pose_batch(b["kp"], b["kp3d"], K, b["boxes_xy"], b["rates"], thresh=0.5, min_k=0, threads=threads,
                                       report=report)


def _camera(q, t):
    """[angle-axis, t] of a returned pose.  Through scipy's quaternion -> rotation vector, which is accurate at every angle
    (from the matrix, the angle's acos loses digits near pi, where random attitudes are most frequent)."""
    from scipy.spatial.transform import Rotation
    return np.concatenate([Rotation.from_quat([q[1], q[2], q[3], q[0]]).as_rotvec(), t])


# ---- 1. the report does not touch the solve ------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", [_solve_w, _solve_kp], ids=["pnp_batch_w_ex", "pnp_batch_ex"])
def test_report_does_not_touch_the_solve(batch, solve):
    raws = []
    for threads in (1, 4):
        q0, t0 = solve(batch, threads, report=False)
        q, t, rep = solve(batch, threads)
        assert np.array_equal(q, q0, equal_nan=True) and np.array_equal(t, t0, equal_nan=True), threads
        raws.append(rep.raw)
    assert np.isnan(q[list(SHORT)]).all() and np.isfinite(np.delete(q, SHORT, 0)).all()
    assert raws[0].tobytes() == raws[1].tobytes()                    # the same bits for any thread count
    assert raws[0].shape == (batch["m"], L.POSE_REPORT_DOUBLES)


def test_null_report_is_the_old_entry(batch):
    """The C ABI with report = NULL, called directly: the poses of esahrnet_pnp_batch_w."""
    b = batch
    p = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    q0, t0 = _solve_w(b, 2, report=False)
    q, t = np.empty_like(q0), np.empty_like(t0)
    pts, w = np.ascontiguousarray(b["pts"]), np.ascontiguousarray(b["w"])
    L.check(L.lib().esahrnet_pnp_batch_w_ex(p(pts), p(w), p(b["count"]), b["m"], b["k"], p(b["kp3d"]), p(b["order"]),
                                            p(np.ascontiguousarray(K.reshape(9))), 2, p(q), p(t), None))
    assert np.array_equal(q, q0, equal_nan=True) and np.array_equal(t, t0, equal_nan=True)
    assert L.lib().esahrnet_pnp_batch_w_ex(None, p(w), p(b["count"]), b["m"], b["k"], p(b["kp3d"]), p(b["order"]),
                                           p(np.ascontiguousarray(K.reshape(9))), 2, p(q), p(t), None) == 1
    assert b"pnp_batch_w: null argument" in L.lib().esahrnet_last_error()


# ---- 2. native fields against the numpy oracle -----------------------------------------------------------------------------------
def _rows_w(b, i):
    n = int(b["count"][i])
    return b["kp3d"][b["order"][i, :n]], b["pts"][i, :n], b["w"][i, :n]


def _rows_kp(b, i):
    """The selection of val.py:172-180 for image i: peaks above 0.5, largest first; weights are the peaks."""
    kp = b["kp"][i].astype(np.float64)
    idx = [j for j in np.argsort(-kp[:, 2], kind="stable") if kp[j, 2] > 0.5]
    return b["kp3d"][idx], kp[idx, :2] * 2.0 + b["boxes_xy"][i], kp[idx, 2]


@pytest.mark.parametrize("solve,rows", [(_solve_w, _rows_w), (_solve_kp, _rows_kp)], ids=["pnp_batch_w_ex", "pnp_batch_ex"])
def test_fields_against_the_numpy_oracle(batch, solve, rows):
    """pnp.pose_report at the pose the native solver returned differs from the native row by summation order only: integer
    fields exact, the real fields to relative 1e-10, and the covariance to the forward bound of a backward-stable 6x6 inverse,
    max|cov (J^T J)_oracle - I| <= 100 eps cond((J^T J)_oracle).  The size of the consensus set is that of
    pnp.solve_pnp_ransac(return_stats=True).  ransac_iters and lm_iters are held to their ranges here: on noisy 5-point sets
    the numpy EPnP and the native one pick different models (their parity is unpinned, pnp.py), so the draw that first
    explains all points, and the last bits of the start the LM's 1e-14 stopping rule sees, differ.  The iteration count is
    compared where the minimal models are determined: test_covariance_is_calibrated (noise-free row) and
    test_no_consensus_sets_flag_bit_0."""
    q, t, rep = solve(batch, 4)
    worst = dict.fromkeys(REAL + ("cov",), 0.0)
    for i in range(batch["m"]):
        p3, p2, w = rows(batch, i)
        assert rep.n[i] == len(p3)
        if i in SHORT:
            continue
        R0, t0, mask, (inliers, iters, fallback) = pnp.solve_pnp_ransac(p3, p2, K, return_stats=True)
        want = pnp.pose_report(p3, p2, w, K, _camera(q[i], t[i]))
        assert (rep.status[i], rep.flags[i], rep.inliers[i], rep.argmax[i]) == (0, int(fallback), inliers, want["argmax"]), i
        assert inliers == int(mask.sum()) and 1 <= rep.ransac_iters[i] <= 100 and 1 <= rep.lm_iters[i] <= 50
        for name in REAL:
            got = getattr(rep, name)[i]
            worst[name] = max(worst[name], abs(got - want[name]) / abs(want[name]))
            assert abs(got - want[name]) <= 1e-10 * abs(want[name]), (i, name, got, want[name])
        H = want["JtJ"]
        err, bound = np.abs(rep.cov[i] @ H - np.eye(6)).max(), 100 * EPS * np.linalg.cond(H)
        worst["cov"] = max(worst["cov"], err / bound)
        assert err <= bound, (i, err, bound)
        assert np.array_equal(rep.cov[i], rep.cov[i].T)
    print("worst relative differences", {k: f"{v:.2e}" for k, v in worst.items()}, "(cov: as a fraction of its bound)")


# ---- 3. the oracle's Jacobian against scipy's finite differences ----------------------------------------------------------------
def _scipy_normal_matrix(p3d, p2d, w3, q, t):
    """J^T J of the weighted residuals in (dw, dt) around the pose (q, t), by scipy alone: the increment applied through
    scipy's Rotation, the Jacobian by least_squares' own '3-point' differences at the solution (max_nfev=1: no step taken)."""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    base = Rotation.from_quat([q[1], q[2], q[3], q[0]])

    def res(x):
        pc = (Rotation.from_rotvec(x[:3]) * base).apply(p3d) + t + x[3:]
        d = np.stack([K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2], K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2]], 1) - p2d
        return np.stack([w3[:, 0] * d[:, 0] + w3[:, 1] * d[:, 1], w3[:, 1] * d[:, 0] + w3[:, 2] * d[:, 1]], 1).ravel()

    sol = least_squares(res, np.zeros(6), jac="3-point", method="trf", max_nfev=1)
    assert np.array_equal(sol.x, np.zeros(6))
    return sol.jac.T @ sol.jac


def test_oracle_jacobian_against_scipy(batch):
    """To 1e-6 of sqrt(H_ii H_jj): scipy's step is eps^(1/3), a truncation error of about 4e-11 relative; the margin covers
    the curvature of the projection."""
    q, t, rep = _solve_w(batch, 4)
    worst = 0.0
    for i in (0, 1, 2, 3, 30, 63):
        p3, p2, w = _rows_w(batch, i)
        H = pnp.pose_report(p3, p2, w, K, _camera(q[i], t[i]))["JtJ"]
        Hs = _scipy_normal_matrix(p3, p2, w, q[i], t[i])
        d = np.sqrt(np.diag(H))
        worst = max(worst, (np.abs(H - Hs) / np.outer(d, d)).max())
    print(f"max |H - H_scipy| / sqrt(H_ii H_jj) = {worst:.3e} (bound 1e-6)")
    assert worst <= 1e-6


# ---- 4. calibration ----------------------------------------------------------------------------------------------------------------
def test_covariance_is_calibrated():
    """4000 noisy copies (sigma 0.2 px, weights 1/sigma) of one scene in one native batch: the six empirical variances within
    5 sampling standard deviations, 5 sqrt(2/(N-1)) = 11.2 %, of covariance(absolute_sigma=True) of the noise-free solve, and
    the mean of d^T cov^-1 d within 5 sqrt(12/N) = 0.27 of 6."""
    from scipy.spatial.transform import Rotation
    N, k, sigma = 4000, 11, 0.2
    rng = np.random.default_rng(7)
    kp3d = rng.uniform(-0.5, 0.5, (k, 3))                           # a 1 m cube; random points are not coplanar
    assert np.linalg.matrix_rank(kp3d - kp3d.mean(0)) == 3
    Rt = Rotation.from_rotvec([0.4, -0.7, 0.3])
    tt = np.array([0.1, -0.2, 8.0])
    uv = pnp.project(kp3d, Rt.as_matrix(), tt, K)
    pts = np.concatenate([uv[None], uv[None] + rng.normal(0, sigma, (N, k, 2))])              # row 0: noise-free
    w = np.broadcast_to(np.array([1 / sigma, 0.0, 1 / sigma]), (N + 1, k, 3))
    count = np.full(N + 1, k, np.int32)
    order = np.broadcast_to(np.arange(k, dtype=np.int32), (N + 1, k))
    q, t, rep = pnp.correspondences_to_pose_batch(pts, w, count, order, kp3d, K, 0, report=True)
    assert (rep.status == 0).all() and (rep.flags == 0).all() and (rep.inliers == k).all()
    *_, (inliers, iters, fallback) = pnp.solve_pnp_ransac(kp3d, uv, K, return_stats=True)
    assert (rep.inliers[0], rep.ransac_iters[0], rep.flags[0] & 1) == (inliers, iters, int(fallback)) == (k, 1, 0)
    cov = rep.covariance(absolute_sigma=True)[0]
    assert np.array_equal(cov, rep.cov[0])
    R_est = Rotation.from_quat(q[1:, [1, 2, 3, 0]])
    d = np.concatenate([(R_est * Rt.inv()).as_rotvec(), t[1:] - tt], 1)                        # [N, 6] = (dw, dt)
    ratio = d.var(0, ddof=1) / np.diag(cov)
    m2 = np.einsum("ni,ij,nj->n", d, np.linalg.inv(cov), d).mean()
    print("empirical / predicted variance", np.round(ratio, 4).tolist(), f"mean Mahalanobis^2 {m2:.4f}")
    assert np.abs(ratio - 1).max() <= 5 * np.sqrt(2 / (N - 1))
    assert abs(m2 - 6) <= 5 * np.sqrt(12 / N)


# ---- 5. scale invariance -------------------------------------------------------------------------------------------------------------
def test_scale_of_the_weights():
    """Scalar weights w and 3w: the same poses (1e-9), the same covariance(absolute_sigma=False) and cov smaller by 9, both to
    1e-6 of sqrt(C_ii C_jj).  The noise is 0.02 px: the LM stops when a step gains less than 1e-14 of the cost, which leaves the
    pose about 1e-7 sqrt(2n - 6) standard deviations from the minimum, on either side; for that to stay below 1e-9 m at
    Z <= 14 m, where sigma_tz is about Z^2 / (f * 1 m) / sqrt(n) = 0.02 m per pixel of noise, the noise has to stay below
    1e-9 / (1e-7 * 4 * 0.02) = 0.1 px.  (At the 0.5 px of the other tests the two solves stop up to 2e-8 m apart.)"""
    b = _batch(sigma=0.02, seed=1)
    peak = np.random.default_rng(3).uniform(0.5, 1.5, b["w"].shape[:2])
    reps = []
    for s in (1.0, 3.0):
        b["w"] = np.stack([s * peak, np.zeros_like(peak), s * peak], 2)
        reps.append(_solve_w(b, 4))
    (q1, t1, r1), (q3, t3, r3) = reps
    ok = r1.status == 0
    assert ok.sum() == b["m"] - len(SHORT) and np.array_equal(ok, r3.status == 0)
    assert np.abs(q1[ok] - q3[ok]).max() <= 1e-9 and np.abs(t1[ok] - t3[ok]).max() <= 1e-9
    c1, c3 = r1.covariance()[ok], r3.covariance()[ok]
    scale = np.sqrt(np.einsum("nii->ni", c1)[:, :, None] * np.einsum("nii->ni", c1)[:, None, :])
    print(f"poses: |dq| {np.abs(q1[ok] - q3[ok]).max():.2e} |dt| {np.abs(t1[ok] - t3[ok]).max():.2e}; covariance(): "
          f"{(np.abs(c1 - c3) / scale).max():.2e} of sqrt(C_ii C_jj)")
    assert (np.abs(c1 - c3) / scale).max() <= 1e-6
    assert (np.abs(r1.cov[ok] - 9 * r3.cov[ok]) / (scale / r1.s2[ok, None, None])).max() <= 1e-6
    assert np.abs(r3.cost[ok] / r1.cost[ok] - 9).max() <= 1e-6


# ---- 6. statuses and flags -----------------------------------------------------------------------------------------------------------
def test_three_points_give_status_1(batch):
    q, t, rep = _solve_w(batch, 2)
    for i in SHORT:
        assert np.isnan(q[i]).all() and np.isnan(t[i]).all()
        assert rep.raw[i, 0] == 1 and rep.raw[i, 2] == 3 and np.isnan(np.delete(rep.raw[i], [0, 2])).all()
        assert (rep.status[i], rep.n[i], rep.inliers[i], rep.flags[i]) == (1, 3, -1, -1) and np.isnan(rep.cov[i]).all()


def test_two_weighted_points_have_no_covariance(batch):
    b = dict(batch)
    b["w"] = batch["w"].copy()
    b["w"][:, 2:] = 0.0
    q, t, rep = _solve_w(b, 2)
    ok = rep.status == 0
    assert ok.sum() == b["m"] - len(SHORT)
    assert np.isfinite(q[ok]).all() and np.isfinite(t[ok]).all()
    assert ((rep.flags[ok] & 2) == 2).all() and np.isnan(rep.cov[ok]).all()
    assert np.isfinite(rep.raw[ok, :L.POSE_REPORT_COV]).all()
    assert np.isnan(rep.covariance()[ok]).all()


FALLBACK_SEED = 0        # chosen on the CPU: pnp.solve_pnp_ransac reports the fallback for it (asserted below)


def test_no_consensus_sets_flag_bit_0():
    """Six random image points under six random model points: no 5-point model explains 4 of them to 5 px, so RANSAC falls back
    to all points."""
    rng = np.random.default_rng(FALLBACK_SEED)
    kp3d = rng.uniform(-0.5, 0.5, (6, 3))
    pts = rng.uniform([200, 100], [1700, 1100], (6, 2))
    *_, (inliers, iters, fallback) = pnp.solve_pnp_ransac(kp3d, pts, K, return_stats=True)
    assert fallback and inliers == 6
    q, t, rep = pnp.correspondences_to_pose_batch(pts[None], np.tile([1.0, 0.0, 1.0], (1, 6, 1)), [6], np.arange(6)[None], kp3d, K, 1,
                                                  report=True)
    assert rep.status[0] == 0 and rep.flags[0] & 1 and rep.inliers[0] == rep.n[0] == 6 and rep.ransac_iters[0] == iters
    assert np.isfinite(q).all() and np.isfinite(t).all()


# ---- 7. the gate -----------------------------------------------------------------------------------------------------------------------
class StandInNet:
    """Stands in for the GPU model on the device-select path: hands estimate_poses a given correspondence record (CPU tensors)."""

    def __init__(self, pts, w, count, order):
        self.rec = [torch.as_tensor(np.ascontiguousarray(a)) for a in (count, order, pts, w)]

    def _loader(self, request, frames, boxes, idx, scale, rule, mean, std, pixel_format):
        m, k = self.rec[2].shape[:2]
        *views, cpacked = inference.pack_correspondences(m, k, "cpu")
        for v, a in zip(views, self.rec):
            v.copy_(a)
        return inference.LoaderResult(m, k, {"correspondences": (cpacked, inference.record_fields(k, "correspondences"))})


@pytest.fixture(scope="module")
def gate_scene():
    """Four images, sigma 0.1 px; image 2 carries a 40 px error on three of its 11 keypoints."""
    rng = np.random.default_rng(11)
    m, k = 4, 11
    scene = synth.make_scene(m, k, seed=5)
    pts = scene["uv"] + rng.normal(0, 0.1, scene["uv"].shape)
    pts[2, [1, 4, 8]] += np.array([[40.0, 0.0], [0.0, -40.0], [-28.3, 28.3]])
    w = np.tile([1.0, 0.0, 1.0], (m, k, 1))
    net = StandInNet(pts, w, np.full(m, k, np.int32), np.tile(np.arange(k, dtype=np.int32), (m, 1)))
    return net, scene


def test_the_gate(gate_scene):
    net, scene = gate_scene
    args = (net, None, [(0, 0, 1, 1)] * 4, scene["kp3d"], K)
    kw = dict(device_select=True, threads=2)
    poses, rep = pipeline.estimate_poses(*args, max_rms_px=2.0, on_fail="nan", return_report=True, **kw)
    finite = [bool(np.isfinite(q).all() and np.isfinite(t).all()) for q, t in poses]
    assert finite == [True, True, False, True]
    assert rep.status[2] == 0 and rep.rms_px[2] > 2 and rep.gated.tolist() == [False, False, True, False]
    assert (rep.rms_px[[0, 1, 3]] < 0.5).all()
    print("rms_px", rep.rms_px.tolist(), "inliers", rep.inliers.tolist())
    with pytest.raises(pipeline.PoseFailure, match=r"positions \[2\]"):
        pipeline.estimate_poses(*args, max_rms_px=2.0, on_fail="raise", **kw)
    # without the gate: a finite pose, as before, and the report changes nothing
    plain = pipeline.estimate_poses(*args, on_fail="raise", **kw)
    assert all(np.isfinite(q).all() and np.isfinite(t).all() for q, t in plain)
    again, rep2 = pipeline.estimate_poses(*args, on_fail="raise", return_report=True, **kw)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(plain, again))
    assert rep2.raw.tobytes() == rep.raw.tobytes() and not rep2.gated.any()
    for i in (0, 1, 3):
        assert np.array_equal(poses[i][0], plain[i][0]) and np.array_equal(poses[i][1], plain[i][1])
    # the other gate: the three displaced points are no inliers
    assert rep.inliers.tolist() == [11, 11, 8, 11]
    gated = pipeline.estimate_poses(*args, min_inliers=9, on_fail="nan", **kw)
    assert [bool(np.isfinite(q).all()) for q, _ in gated] == [True, True, False, True]
    with pytest.raises(ValueError, match="native"):
        pipeline.estimate_poses(*args, native=False, return_report=True)
    with pytest.raises(ValueError, match="native"):
        pipeline.estimate_poses(*args, native=False, max_rms_px=2.0)


def test_run_submission_writes_the_fallback_for_a_gated_pose(gate_scene):
    net, scene = gate_scene
    names = ["img0.jpg", "img1.jpg", "img2.jpg", "img3.jpg"]
    batches = [(names, None, [(0, 0, 1, 1)] * 4)]
    writer = pipeline.run_submission(net, batches, scene["kp3d"], K, pipeline.SubmissionWriter(), device_select=True, max_rms_px=2.0)
    assert writer.failed == ["img2.jpg"]
    rows = {r["filename"]: r for r in writer.test_results}
    assert (tuple(rows["img2.jpg"]["q"]), tuple(rows["img2.jpg"]["r"])) == pipeline.FALLBACK_POSE
    assert all(tuple(rows[n]["q"]) != pipeline.FALLBACK_POSE[0] for n in ("img0.jpg", "img1.jpg", "img3.jpg"))
    writer = pipeline.run_submission(net, batches, scene["kp3d"], K, pipeline.SubmissionWriter(), device_select=True)
    assert writer.failed == []


class StandInLoader:
    """Stands in for the GPU model on the device-loader path: a keypoint record with one crop the loader could not make."""

    def __init__(self, kp):
        self.kp = kp

    def _loader(self, request, frames, boxes, idx, scale, rule, mean, std, pixel_format):
        m, k = self.kp.shape[:2]
        lay = inference.packed_layout(m, k, False)
        packed = torch.zeros(lay["total"][1], dtype=torch.uint8)
        part = lambda name, dtype, *shape: packed[lay[name][0]:lay[name][0] + lay[name][1]].view(dtype).view(*shape)   # noqa: E731
        part("rates", torch.float64, m).fill_(1.0)
        part("kp", torch.float32, m, k, 3).copy_(torch.as_tensor(self.kp))
        part("valid", torch.int32, m).copy_(torch.tensor([1, 0, 1], dtype=torch.int32))
        return inference.LoaderResult(m, k, {"keypoints": (packed, inference.record_fields(k, "keypoints"))})


def test_report_on_the_device_loader_path():
    """The report of device_loader=True is the report of pnp.keypoints_to_pose_batch on the fetched rows; a crop the loader
    could not make has status 1 with n = 0."""
    m, k = 3, 11
    scene = synth.make_scene(m, k, seed=9)
    kp = np.concatenate([scene["uv"], np.random.default_rng(2).uniform(0.85, 1.0, (m, k, 1))], 2).astype(np.float32)
    kp[1] = np.nan
    args = (StandInLoader(kp), None, [(0, 0, 1, 1)] * m, scene["kp3d"], K)
    poses, rep = pipeline.estimate_poses(*args, device_loader=True, min_k=k, on_fail="nan", return_report=True, threads=2)
    plain = pipeline.estimate_poses(*args, device_loader=True, min_k=k, on_fail="nan", threads=2)
    assert all(np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) for a, b in zip(plain, poses))
    q, t, want = pnp.keypoints_to_pose_batch(kp[[0, 2]], scene["kp3d"], K, [(0, 0)] * 2, [1.0] * 2, 0.8, k, 2, report=True)
    assert rep.raw[[0, 2]].tobytes() == want.raw.tobytes() and (rep.status[[0, 2]] == 0).all()
    assert (rep.status[1], rep.n[1]) == (1, 0) and np.isnan(np.delete(rep.raw[1], [0, 2])).all() and np.isnan(poses[1][0]).all()


# ---- 8. header -------------------------------------------------------------------------------------------------------------------------
def test_header_names_every_offset():
    text = open(os.path.join(ROOT, "include", "esahrnet.h")).read()
    body = text[text.index("enum esahrnet_pose_report"):]
    body = body[:body.index("};")]
    offsets = {name.lower(): int(v) for name, v in re.findall(r"ESAHRNET_REPORT_(\w+)\s*=\s*(\d+)\s*,\s*/\*", body)}   # each with a comment
    assert offsets == {**{name: i for i, name in enumerate(L.POSE_REPORT_FIELDS)}, "cov": L.POSE_REPORT_COV}
    assert int(re.search(r"ESAHRNET_POSE_REPORT_DOUBLES\s*=\s*(\d+)", body).group(1)) == L.POSE_REPORT_DOUBLES == 12 + 21
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in (("esahrnet_pnp_batch_ex", 13), ("esahrnet_pnp_batch_w_ex", 12)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and name in L.exported_symbols()
        assert hasattr(C.CDLL(L.LIB_PATH), name) and len(getattr(L.lib(), name).argtypes) == nargs
    assert re.search(r"#define\s+ESAHRNET_ABI_VERSION\s+6\b", text) and L.lib().esahrnet_abi_version() == 6 == L.ABI_VERSION
