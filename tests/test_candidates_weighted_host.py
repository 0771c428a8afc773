"""The native candidate solve with 2x2 weights (csrc/pnp_host.hip, `esahrnet_pnp_batch_cand_w`) against its oracle, the numpy
statement pnp.candidates_to_pose(..., hess=...), and its invariants.  Pure host code: runs without a GPU.

Scenes: the recipe and the seeds of tests/test_candidates_host.py (`scene`, `seed_of`, CASES), plus a Hessian per candidate: minus
the information matrix of a rotated Gaussian blob after the decoder's blur (correspond_ref.gaussian_hessian), NaN where the
candidate row is NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correspond_ref as R  # noqa: E402
import test_candidates_host as T  # noqa: E402

from esa_pose_estimation_amd import _lib, pnp  # noqa: E402

K, N, CASES, scene, seed_of, _bits = T.K, T.N, T.CASES, T.scene, T.seed_of, T._bits


def hessians(rng, cand):
    """A blob shape per candidate -> hess f64 [n,k,M,3], NaN where the candidate is."""
    n, k, M = cand.shape[:3]
    hess = np.full((n, k, M, 3), np.nan)
    for i in range(n):
        for j in range(k):
            for m in range(M):
                if np.isfinite(cand[i, j, m, 0]):
                    hess[i, j, m] = R.gaussian_hessian(rng.uniform(1.0, 3.0), rng.uniform(1.0, 3.0), rng.uniform(0, np.pi))
    return hess


def _raw(cand, hess, kp3d, boxes, rates, thresh, min_k, min_ratio=0.3, threads=2):
    """esahrnet_pnp_batch_cand_w itself (hess may be None: NULL) -> (q, t, report, used)."""
    cand = np.ascontiguousarray(cand, np.float32)
    n, k, m = cand.shape[:3]
    q, t, used = np.empty((n, 4)), np.empty((n, 3)), np.empty((n, k), np.int32)
    rep = np.empty((n, _lib.POSE_REPORT_DOUBLES))
    kp3d, K9 = np.ascontiguousarray(kp3d, np.float64), np.ascontiguousarray(K, np.float64).reshape(9)
    bxy, rt = np.ascontiguousarray(np.asarray(boxes)[:, :2], np.int32), np.ascontiguousarray(rates, np.float64)
    hess = None if hess is None else np.ascontiguousarray(hess, np.float64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)        # noqa: E731
    _lib.check(_lib.lib().esahrnet_pnp_batch_cand_w(p(cand), p(hess), n, k, m, p(kp3d), p(K9), p(bxy), p(rt), float(thresh), int(min_k),
                                                    float(min_ratio), int(threads), p(q), p(t), p(rep), p(used)))
    return q, t, rep, used


@pytest.mark.parametrize("k,nbad", CASES)
def test_without_hessians_it_is_the_peak_weighted_entry_bit_for_bit(k, nbad):
    kp3d, cand, boxes, rates, _, _ = scene(np.random.default_rng(seed_of(k, nbad)), N, k, nbad)
    q0, t0, u0, r0 = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=k, threads=2, report=True)
    q, t, rep, used = _raw(cand, None, kp3d, boxes, rates, 0.0, k)
    assert _bits(q, t, rep, used) == _bits(q0, t0, r0.raw, u0)
    assert r0.rescued.all()
    q1, t1, u1 = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=k, threads=2, hess=None)
    assert _bits(q1, t1, u1) == _bits(q0, t0, u0)


@pytest.mark.parametrize("k,nbad", CASES)
def test_native_matches_numpy_with_hessians(k, nbad):
    rng = np.random.default_rng(seed_of(k, nbad))
    kp3d, cand, boxes, rates, poses, bads = scene(rng, N, k, nbad)
    hess = hessians(rng, cand)
    q, t, used, rep = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=k, threads=3, report=True, hess=hess)
    qp, tp, _ = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=k, threads=3)
    differs = 0
    for i in range(N):
        qn, tn, un = pnp.candidates_to_pose(cand[i], kp3d, K, boxes[i], rates[i], thresh=0.0, min_k=k, hess=hess[i])
        assert np.array_equal(used[i], un), (i, used[i], un)
        s_pair = pnp.speed_score(q[i], t[i], qn, tn)[0]
        print(f"k={k} bad={nbad} image {i}: native - numpy {s_pair:.3e} SPEED, inliers {int(rep.inliers[i])}")
        assert s_pair < 1e-6, (i, s_pair)                                       # tests/test_candidates_host.py's bound
        want = np.zeros(k, np.int32)
        want[bads[i]] = 1
        assert np.array_equal(used[i], want), (i, used[i], bads[i])             # the swap rule does not look at the weights
        differs += not np.array_equal(q[i], qp[i])
    assert differs == N and rep.rescued.all()                                   # ... but the refinement does


def test_isotropic_hessians_are_scalar_weights():
    """H = -c I weighs a point by rate * sqrt(c), isotropically: the solve with such Hessians is the peak-weighted solve on
    candidates whose peak column is rate * sqrt(c).  c is chosen per candidate so that those peaks keep the scene's order."""
    kp3d, cand, boxes, rates, _, _ = scene(np.random.default_rng(seed_of(11, 2)), N, 11, 2)
    rate = np.asarray(rates).reshape(-1, 1, 1)
    c = (cand[..., 2].astype(np.float64) / rate) ** 2                           # NaN where the candidate is
    hess = np.stack([-c, np.zeros_like(c), -c], -1)
    peaks = cand.copy()
    peaks[..., 2] = (rate * np.sqrt(c)).astype(np.float32)
    assert np.array_equal(np.argsort(-peaks[:, :, 0, 2], 1, kind="stable"), np.argsort(-cand[:, :, 0, 2], 1, kind="stable"))
    q, t, used = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=11, hess=hess)
    q0, t0, used0 = pnp.candidates_to_pose_batch(peaks, kp3d, K, boxes, rates, thresh=0.0, min_k=11)
    assert np.array_equal(used, used0) and (used == 1).any()
    for i in range(N):
        s = pnp.speed_score(q[i], t[i], q0[i], t0[i])[0]
        assert s < 1e-6, (i, s)


def test_a_nan_or_indefinite_hessian_is_weight_zero():
    """On one keypoint per image the Hessian is NaN, a saddle, or not negative definite: the same bits each time, and those of the
    solve in which that keypoint's weight row is zero (esahrnet_pnp_batch_w on the same points, in an image where nothing is
    repaired); the point still reaches EPnP / RANSAC, so it is still selected and can still be swapped."""
    from esa_pose_estimation_amd import inference
    rng = np.random.default_rng(21)
    k = 11
    kp3d, cand, boxes, rates, _, bads = scene(rng, N, k, 2)
    hess = hessians(rng, cand)
    js = [int(bads[i][0]) if i % 2 else int(np.setdiff1d(np.arange(k), bads[i])[0]) for i in range(N)]
    runs = []
    for bad in ([np.nan, np.nan, np.nan], [0.1, 0.0, -0.2], [-0.1, 0.2, -0.1], [0.0, 0.0, 0.0], [-0.2, np.nan, -0.2]):
        h = hess.copy()
        for i, j in enumerate(js):
            h[i, j, :] = bad
        runs.append(pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=k, hess=h))
    for q, t, used in runs[1:]:
        assert _bits(q, t, used) == _bits(*runs[0])
    q, t, used = runs[0]
    assert all(used[i, j] == (1 if i % 2 else 0) for i, j in enumerate(js))      # selected, and swapped where its primary is bad
    qf, tf, _ = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=k, hess=hess)
    assert all(not np.array_equal(q[i], qf[i]) for i in range(N))               # the weight mattered
    # nothing to repair: the solve is pose_solve on candidate 0, which esahrnet_pnp_batch_w runs on explicit weight rows
    kp3d, cand, boxes, rates, _, _ = scene(rng, N, k, 0)
    hess = hessians(rng, cand)
    for i in range(N):
        hess[i, i % k, 0] = np.nan
    q, t, used = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=k, hess=hess)
    assert (used == 0).all()
    order = np.argsort(-cand[:, :, 0, 2], 1, kind="stable").astype(np.int32)
    pts, w = np.zeros((N, k, 2)), np.zeros((N, k, 3))
    for i in range(N):
        xy = inference.crop_to_image(cand[i, :, 0, :2].astype(np.float64), rates[i], boxes[i][0], boxes[i][1])
        for r, j in enumerate(order[i]):
            pts[i, r] = xy[j]
            w[i, r] = 0.0 if j == i % k else pnp.hessian_weight(hess[i, j, 0], rates[i])
            assert (w[i, r] == 0).all() == (j == i % k)
    qw, tw = pnp.correspondences_to_pose_batch(pts, w, np.full(N, k, np.int32), order, kp3d, K)
    assert _bits(q, t) == _bits(qw, tw)


def test_same_bits_for_any_thread_count():
    rng = np.random.default_rng(13)
    kp3d, cand, boxes, rates, _, _ = scene(rng, 17, 11, 3)
    hess = hessians(rng, cand)
    ref = None
    for threads in (1, 3, 16):
        q, t, used, rep = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=11, threads=threads, report=True,
                                                       hess=hess)
        got = _bits(q, t, used, rep.raw)
        ref = ref or got
        assert got == ref, threads
    assert rep.rescued.any()


def test_numpy_weight_rule_is_correspond_refs():
    rng = np.random.default_rng(3)
    for H in list(rng.uniform(-1, 0.2, (200, 3))) + [np.full(3, np.nan), np.zeros(3), np.array([-1e-320, 0, -1e-320]),
                                                     np.array([-1e300, 0, -1e300]), np.array([-np.inf, 0, -1.0])]:
        for rate in (0.05, 1.0, 7.5):
            assert _bits(pnp.hessian_weight(H, rate)) == _bits(R.hessian_weight(H, rate)), (H, rate)


def test_every_refusal_with_its_text():
    L = _lib.lib()
    assert "esahrnet_pnp_batch_cand_w" in _lib.exported_symbols() and L.esahrnet_abi_version() == 6
    buf = (C.c_double * 512)()
    p = C.cast(buf, C.c_void_p)

    def call(cand=p, hess=p, n=1, k=11, M=2, kp3d=p, K9=p, boxes=p, rates=p, ratio=0.3, q=p, t=p, rep=p, used=p):
        rc = L.esahrnet_pnp_batch_cand_w(cand, hess, n, k, M, kp3d, K9, boxes, rates, 0.8, 24, ratio, 1, q, t, rep, used)
        assert rc == 1
        return L.esahrnet_last_error().decode()

    for name in ("cand", "kp3d", "K9", "boxes", "rates", "q", "t", "used"):
        assert call(**{name: None}) == "pnp_batch_cand_w: null argument", name
    assert call(n=-1) == "pnp_batch_cand_w: negative image count -1"
    assert call(k=0) == "pnp_batch_cand_w: 0 keypoints per image unsupported (1..64)"
    assert call(k=65) == "pnp_batch_cand_w: 65 keypoints per image unsupported (1..64)"
    assert call(M=0) == "pnp_batch_cand_w: 0 candidates per keypoint unsupported (1..4)"
    assert call(M=5) == "pnp_batch_cand_w: 5 candidates per keypoint unsupported (1..4)"
    assert call(ratio=-0.1) == "pnp_batch_cand_w: min_ratio -0.1 must be a number >= 0"
    assert "min_ratio" in call(ratio=float("nan"))
    assert call(cand=None, n=-1, k=0) == "pnp_batch_cand_w: null argument"       # the order: pointers, n, k, M, min_ratio
    assert call(n=-1, k=0, M=9) == "pnp_batch_cand_w: negative image count -1"
    # NULL hess and NULL report are no errors: an empty batch returns at once
    assert L.esahrnet_pnp_batch_cand_w(p, None, 0, 11, 2, p, p, p, p, 0.8, 24, 0.3, 1, p, p, None, p) == 0
    kp3d, cand, boxes, rates, _, _ = scene(np.random.default_rng(16), 2, 11, 1, M=2)
    with pytest.raises(ValueError, match=r"expected hess \[N, K, M, 3\]"):
        pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, hess=np.zeros((2, 11, 3)))
    with pytest.raises(_lib.EsaHrnetError, match="pnp_batch_cand_w: min_ratio"):
        pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, min_ratio=-1.0, hess=np.zeros((2, 11, 2, 3)))
