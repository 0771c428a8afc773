"""The native solve on candidates (csrc/pnp_host.hip, `esahrnet_pnp_batch_cand`) against its oracle, the numpy statement
pnp.candidates_to_pose, and its invariants: with one candidate, or nothing to repair, it is `esahrnet_pnp_batch_ex` bit for bit.
Pure host code: runs without a GPU.

Scenes (`scene`): ESA camera, depth 5-12 m, point noise 0.3 px.  `bad` keypoints per image have their primary (candidate 0)
displaced by 30-120 px, the true position is candidate 1 with a peak 0.5-0.95 of the primary's; half of the good keypoints
carry a decoy runner-up 30-120 px away; candidate 2 is the NaN row of "no further peak".  All keypoints are selected
(thresh 0, min_k = K)."""
import numpy as np
import pytest

from esa_pose_estimation_amd import _lib, pnp

K = np.array([[3003.41297, 0.0, 960.0], [0.0, 3003.41297, 600.0], [0.0, 0.0, 1.0]])
CASES = [(11, 2), (11, 4), (30, 10)]                       # (keypoints, bad primaries per image)
N = 12


def seed_of(k, bad):
    return 7000 + 100 * k + bad


def _far(rng, m):
    return rng.uniform(30, 120, (m, 2)) * rng.choice([-1, 1], (m, 2))


def scene(rng, n, k, nbad, M=3, noise=0.3):
    """-> kp3d [k,3], cand f32 [n,k,M,3], boxes, rates, poses [(R, t)], bad [n][nbad] keypoint indices."""
    kp3d = rng.uniform(-0.6, 0.6, (k, 3))
    cand = np.full((n, k, M, 3), np.nan, np.float32)
    boxes, rates, poses, bads = [], [], [], []
    for i in range(n):
        R = pnp.rodrigues(rng.uniform(-1.2, 1.2, 3))
        t = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(5.0, 12.0)])
        true = pnp.project(kp3d, R, t, K) + rng.normal(0, noise, (k, 2))
        peak = rng.uniform(0.3, 1.0, k)
        bad = rng.choice(k, nbad, replace=False) if nbad else np.zeros(0, np.int64)
        good = np.setdiff1d(np.arange(k), bad)
        decoy = rng.choice(good, len(good) // 2, replace=False)
        first = true.copy()
        first[bad] += _far(rng, len(bad))
        second = np.full((k, 2), np.nan)
        peak2 = np.full(k, np.nan)
        second[bad] = true[bad]
        peak2[bad] = peak[bad] * rng.uniform(0.5, 0.95, len(bad))
        second[decoy] = true[decoy] + _far(rng, len(decoy))
        peak2[decoy] = peak[decoy] * rng.uniform(0.3, 0.95, len(decoy))
        allp = np.concatenate([first, second[np.isfinite(second[:, 0])]])
        x0, y0 = int(allp[:, 0].min()) - 20, int(allp[:, 1].min()) - 20
        rate = 256.0 / (max(np.ptp(allp[:, 0]), np.ptp(allp[:, 1])) + 40.0)
        cand[i, :, 0, :2] = (first - [x0, y0]) * rate
        cand[i, :, 0, 2] = peak
        if M > 1:
            cand[i, :, 1, :2] = (second - [x0, y0]) * rate
            cand[i, :, 1, 2] = peak2
        boxes.append((x0, y0)); rates.append(rate); poses.append((R, t)); bads.append(np.sort(bad))
    return kp3d, cand, boxes, rates, poses, bads


def _score(q, t, pose):
    return pnp.speed_score(q, t, pnp.rotation_to_quat_wxyz(pose[0]), pose[1])[0]


@pytest.mark.parametrize("k,nbad", CASES)
def test_native_matches_numpy_and_repairs_every_bad_primary(k, nbad):
    kp3d, cand, boxes, rates, poses, bads = scene(np.random.default_rng(seed_of(k, nbad)), N, k, nbad)
    q, t, used, rep = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=k, threads=3, report=True)
    q1, t1 = pnp.keypoints_to_pose_batch(cand[:, :, 0], kp3d, K, boxes, rates, thresh=0.0, min_k=k, threads=3)
    assert used.shape == (N, k) and used.dtype == np.int32 and rep.used is used and rep.raw.shape == (N, _lib.POSE_REPORT_DOUBLES)
    for i in range(N):
        qn, tn, un = pnp.candidates_to_pose(cand[i], kp3d, K, boxes[i], rates[i], thresh=0.0, min_k=k)
        assert np.array_equal(used[i], un), (i, used[i], un)
        s_pair = pnp.speed_score(q[i], t[i], qn, tn)[0]
        assert s_pair < 1e-6, (i, s_pair)                                       # native == numpy
        want = np.zeros(k, np.int32)
        want[bads[i]] = 1
        assert np.array_equal(used[i], want), (i, used[i], bads[i])             # every bad primary swapped, no decoy taken
        s2, s1 = _score(q[i], t[i], poses[i]), _score(q1[i], t1[i], poses[i])
        print(f"k={k} bad={nbad} image {i}: SPEED {s1:.5f} -> {s2:.5f}, inliers {int(rep.inliers[i])}")
        assert s2 < s1, (i, s2, s1)                                             # and the pose is better for it
    assert rep.rescued.all()


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint8).tobytes() for a in arrays]


def test_one_candidate_is_the_plain_solve_bit_for_bit():
    kp3d, cand, boxes, rates, _, _ = scene(np.random.default_rng(11), N, 11, 2)
    q0, t0, r0 = pnp.keypoints_to_pose_batch(cand[:, :, 0], kp3d, K, boxes, rates, thresh=0.5, min_k=6, threads=2, report=True)
    q, t, used, rep = pnp.candidates_to_pose_batch(cand[:, :, :1], kp3d, K, boxes, rates, thresh=0.5, min_k=6, threads=2, report=True)
    assert _bits(q, t, rep.raw) == _bits(q0, t0, r0.raw)
    assert set(np.unique(used)) <= {0, -1} and (used == -1).any() and not rep.rescued.any()
    assert np.array_equal((used == 0).sum(1), r0.n)
    q, t, used = pnp.candidates_to_pose_batch(cand[:, :, :1], kp3d, K, boxes, rates, thresh=0.5, min_k=6, threads=2)
    assert _bits(q, t) == _bits(q0, t0)


def test_nothing_bad_nothing_changes():
    kp3d, cand, boxes, rates, _, _ = scene(np.random.default_rng(12), N, 11, 0)           # decoys only
    assert np.isfinite(cand[:, :, 1]).any()
    q0, t0, r0 = pnp.keypoints_to_pose_batch(cand[:, :, 0], kp3d, K, boxes, rates, thresh=0.4, min_k=8, report=True)
    q, t, used, rep = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.4, min_k=8, report=True)
    assert _bits(q, t, rep.raw) == _bits(q0, t0, r0.raw)
    assert set(np.unique(used)) <= {0, -1} and not rep.rescued.any()


def test_same_bits_for_any_thread_count():
    kp3d, cand, boxes, rates, _, _ = scene(np.random.default_rng(13), 17, 11, 3)
    ref = None
    for threads in (1, 3, 16):
        q, t, used, rep = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=11, threads=threads, report=True)
        got = _bits(q, t, used, rep.raw)
        ref = ref or got
        assert got == ref, threads
    assert rep.rescued.any()


def test_weak_decoy_and_nan_rows_are_not_taken():
    kp3d, cand, boxes, rates, poses, bads = scene(np.random.default_rng(14), 6, 11, 2)
    args = dict(thresh=0.0, min_k=11, min_ratio=0.3)
    q, t, used = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, **args)
    assert all((used[i, bads[i]] == 1).all() for i in range(6))
    # the right runner-up of image 0's first bad keypoint, but below min_ratio of its primary: not taken, the others still are
    weak = cand.copy()
    j = bads[0][0]
    weak[0, j, 1, 2] = 0.29 * weak[0, j, 0, 2]
    _, _, used_w = pnp.candidates_to_pose_batch(weak, kp3d, K, boxes, rates, **args)
    assert used_w[0, j] == 0 and used_w[0, bads[0][1]] == 1 and np.array_equal(used_w[1:], used[1:])
    assert np.array_equal(used_w[0], pnp.candidates_to_pose(weak[0], kp3d, K, boxes[0], rates[0], **args)[2])
    _, _, used_r = pnp.candidates_to_pose_batch(weak, kp3d, K, boxes, rates, thresh=0.0, min_k=11, min_ratio=0.25)
    assert used_r[0, j] == 1                                                    # ... and taken once the ratio admits it
    # an all-NaN runner-up row in front of the right one: ignored, the right one is found at rank 2
    shifted = cand.copy()
    shifted[:, :, 2] = cand[:, :, 1]
    shifted[:, :, 1] = np.nan
    q2, t2, used_s = pnp.candidates_to_pose_batch(shifted, kp3d, K, boxes, rates, **args)
    assert np.array_equal(used_s, used * 2) and _bits(q2, t2) == _bits(q, t)
    # no runner-up at all (NaN rows only): candidate 0's solve
    none = cand.copy()
    none[:, :, 1:] = np.nan
    q3, t3, used_n = pnp.candidates_to_pose_batch(none, kp3d, K, boxes, rates, **args)
    q0, t0 = pnp.keypoints_to_pose_batch(cand[:, :, 0], kp3d, K, boxes, rates, thresh=0.0, min_k=11)
    assert (used_n == 0).all() and _bits(q3, t3) == _bits(q0, t0)


def test_fewer_than_four_points_give_the_nan_row():
    kp3d, cand, boxes, rates, _, _ = scene(np.random.default_rng(15), 3, 3, 1)
    q, t, used, rep = pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, thresh=0.0, min_k=3, report=True)
    assert np.isnan(q).all() and np.isnan(t).all() and (rep.status == 1).all() and (used == 0).all() and not rep.rescued.any()
    q, t, used = pnp.candidates_to_pose_batch(cand[:0], kp3d, K, np.zeros((0, 2), np.int32), [], thresh=0.0, min_k=3)
    assert q.shape == (0, 4) and used.shape == (0, 3)


def test_bad_arguments_give_the_librarys_error_text():
    import ctypes as C
    kp3d, cand, boxes, rates, _, _ = scene(np.random.default_rng(16), 2, 11, 1, M=2)
    with pytest.raises(_lib.EsaHrnetError, match="candidates per keypoint unsupported"):
        pnp.candidates_to_pose_batch(np.concatenate([cand, cand, cand], 2)[:, :, :5], kp3d, K, boxes, rates)
    for ratio in (-0.1, float("nan")):
        with pytest.raises(_lib.EsaHrnetError, match="min_ratio"):
            pnp.candidates_to_pose_batch(cand, kp3d, K, boxes, rates, min_ratio=ratio)
    # the decoder's argument checks answer before anything is enqueued: no GPU is touched
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for m, r, text in ((0, 6, "0 candidates per heat-map unsupported"), (5, 6, "5 candidates per heat-map unsupported"),
                       (2, -1, "negative nms_radius")):
        assert L.esahrnet_keypoints_candidates(p, 1, 1, 4, 4, m, r, p, None, None) == 1
        assert text in L.esahrnet_last_error().decode()
    assert L.esahrnet_keypoints_candidates(None, 1, 1, 4, 4, 2, 6, p, None, None) == 1
    assert "null argument" in L.esahrnet_last_error().decode()
    assert L.esahrnet_abi_version() == 6 and _lib.MAX_CANDIDATES == 4


@pytest.mark.parametrize("kw", [dict(device_select=True), dict(device_loader=True), dict(keypoints_only=True),
                                dict(distributed=True), dict(native=False), dict(refine="get_final2"), dict(refine="gaussfit")])
def test_estimate_poses_refuses_candidates_on_the_other_paths(kw):
    from esa_pose_estimation_amd import pipeline
    with pytest.raises(ValueError, match="candidates=2"):
        pipeline.estimate_poses(None, None, [], np.zeros((11, 3)), K, candidates=2, **kw)


def test_heatmaps_to_candidates_refuses_what_heatmaps_to_keypoints_refuses():
    import torch
    from esa_pose_estimation_amd import inference
    with pytest.raises(ValueError, match="4-D tensor"):
        inference.heatmaps_to_candidates(torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        inference.heatmaps_to_candidates(torch.zeros(1, 3, 8, 8))


def test_wrong_blob_heatmaps_end_to_end_with_the_numpy_decoder():
    """The end-to-end case of tests/test_gpu_candidates.py with the decoder's numpy oracle in the device kernel's place."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import candidates_ref as CR
    sc = CR.wrong_blob_scene()
    cand, _ = CR.candidates(CR.wrong_blob_heatmaps(sc).numpy(), 3, 6)
    CR.check_wrong_blob_poses(sc, cand)
