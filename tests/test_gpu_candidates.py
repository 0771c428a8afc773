"""The candidate decoder on the GPU (include/esahrnet.h esahrnet_keypoints_candidates, csrc/keypoints_candidates.hip) against its
numpy oracle tests/candidates_ref.py: equal indices, coordinates within the decoder's bound, bit-equal peaks, candidate 0 the
row of esahrnet_keypoints_ex, a plane's bits independent of its batch, replay from a captured graph; then heat-maps whose
global maximum sits on the wrong blob, through the decoder and the native solve.

Shapes: 16 x 16, 15 x 17 (255 floats: plane 1 is not 16-byte aligned and takes the scalar sweep), 18 x 34 (a width that is no
multiple of 4), 64 x 64 (more than one float4 per lane) and 15 x 264 (66 float4 per row: rows that go on across the end of a wave,
where a lane loads the column beside its float4 itself), each as two batches of n x k = 2 x 3 planes (candidates_ref.NAMES);
M in {1, 2, 4}; r in {0, 1, 6, 64} (64 suppresses the whole plane but the 264 wide one)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import candidates_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (15, 17), (18, 34), (64, 64), (15, 264)]
MS = (1, 2, 4)
RS = (0, 1, 6, 64)
COORD_TOL = 2e-5                 # the get_final decoder's bound against its oracle (f64 log of the device library against math.log)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import inference
    return dict(inference=inference)


@pytest.fixture(scope="module")
def runs(env):
    """Per shape and half h: the batch f32 [2,3,H,W] (numpy and cuda), and per (M, r) the oracle's and the GPU's (cand, idx)."""
    out = {}
    for (h, w) in SHAPES:
        pl = CR.planes(h, w)
        for half in (0, 1):
            hm = np.ascontiguousarray(pl[6 * half:6 * half + 6].reshape(2, 3, h, w))
            t = torch.from_numpy(hm).cuda()
            res = {}
            for M in MS:
                for r in RS:
                    cand, idx = env["inference"].heatmaps_to_candidates(t, M, r, return_index=True)
                    res[M, r] = dict(ref=CR.candidates(hm, M, r), gpu=(cand.cpu().numpy(), idx.cpu().numpy()))
            out[h, w, half] = dict(hm=hm, t=t, names=CR.NAMES[6 * half:6 * half + 6], res=res)
    return out


def _same_bits(a, b):
    """bit-equal, a NaN matching any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))


def test_indices_coordinates_and_peaks_equal_the_oracle(runs):
    worst = 0.0
    for key, f in runs.items():
        for (M, r), d in f["res"].items():
            (rc, ri), (gc, gi) = d["ref"], d["gpu"]
            assert gi.tolist() == ri.tolist(), (key, M, r, f["names"])
            assert _same_bits(gc[..., 2], rc[..., 2]), (key, M, r)
            assert np.array_equal(np.isnan(gc[..., :2]), np.isnan(rc[..., :2])), (key, M, r)
            err = float(np.nanmax(np.abs(gc[..., :2].astype(np.float64) - rc[..., :2]), initial=0.0))
            worst = max(worst, err)
            assert err <= COORD_TOL, (key, M, r, err)
    print(f"largest coordinate difference to the oracle: {worst:.3e} px")


def test_the_planes_show_what_they_were_built_for(runs):
    """The oracle-independent readings: what each plane must give by the rules alone."""
    for (h, w) in SHAPES:
        a, b = runs[h, w, 0], runs[h, w, 1]
        at = lambda f, name, M, r: tuple(x.reshape(6, M, -1)[f["names"].index(name)] for x in f["res"][M, r]["gpu"])     # noqa: E731
        flat = lambda rc: rc[0] * w + rc[1]                                                                              # noqa: E731
        # r = 64 suppresses the whole plane (where it is no wider than that): no runner-up anywhere
        for f in (a, b) if max(h, w) <= 65 else ():
            gc, gi = f["res"][4, 64]["gpu"]
            assert (gi[..., 1:] == -1).all() and np.isnan(gc[..., 1:, :]).all() and (gi[..., 0] >= 0).all()
        # constant plane: ties by index — pixel 0, then the first pixel more than r away
        _, gi = at(a, "constant", 4, 1)
        assert gi.ravel().tolist() == [0, 2, 4, 6]
        _, gi = at(a, "constant", 2, 0)
        assert gi.ravel().tolist() == [0, 1]
        # twins of equal value: the lower index first, the other as the runner-up with the same peak
        gc, gi = at(a, "twins", 2, 6)
        assert gi.ravel().tolist() == [2 * w + 3, 12 * w + 11] and gc[0, 2] == gc[1, 2] == 1.0
        # ring: a runner-up at Chebyshev distance exactly r is suppressed, one at r + 1 is kept
        R = CR.RING
        _, gi = at(a, "ring", 4, 6)
        assert gi.ravel().tolist()[:2] == [flat(R["peak"]), flat(R["d7"])]
        _, gi = at(a, "ring", 4, 1)
        assert gi.ravel().tolist()[:3] == [flat(R["peak"]), flat(R["d2"]), flat(R["d6"])]
        _, gi = at(a, "ring", 4, 0)
        assert gi.ravel().tolist() == [flat(R["peak"]), flat(R["twin"]), flat(R["d2"]), flat(R["d6"])]
        # shoulder: its pixels are never local maxima, at no radius
        for M in MS:
            for r in RS:
                _, gi = at(b, "shoulder", M, r)
                assert gi[0, 0] == 5 * w + 5 and not set(gi.ravel().tolist()) & {flat(rc) for rc in CR.SHOULDER}
        # one NaN pixel: it is candidate 0 (NaN is the maximum), the blob's peak is the first runner-up
        gc, gi = at(b, "one-nan", 2, 1)
        assert gi.ravel().tolist() == [(h - 3) * w + (w - 4), 5 * w + 5] and np.isnan(gc[0, 2]) and np.isfinite(gc[1]).all()
        # a NaN beside the 0.7 spike: the spike is never a candidate, nor is any other neighbour of the NaN
        gc, gi = at(b, "nan-neighbour", 4, 1)
        assert gi[0, 0] == 10 * w + 11 and gi[1, 0] == 3 * w + 3 and 10 * w + 10 not in gi.ravel().tolist()
        assert (gc[2:, 2] == np.float32(0.05)).all()
        # all -inf and all NaN: index 0, no runner-up
        for name in ("all-neg-inf", "all-nan"):
            gc, gi = at(b, name, 4, 0)
            assert gi.ravel().tolist() == [0, -1, -1, -1] and gc[0, :2].tolist() == [0.0, 0.0]


def test_candidate_zero_is_the_existing_decoder_bit_for_bit(env, runs):
    inf = env["inference"]
    for key, f in runs.items():
        kp, idx = inf._keypoints(f["t"], True)                      # esahrnet_keypoints_ex
        kp, idx = kp.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(inf.heatmaps_to_keypoints(f["t"]).cpu().numpy().view(np.int32), kp.view(np.int32))
        preds, maxvals = inf.get_max_preds(f["t"])
        w = key[1]
        for (M, r), d in f["res"].items():
            gc, gi = d["gpu"]
            assert np.array_equal(gc[:, :, 0].view(np.int32), kp.view(np.int32)), (key, M, r)          # NaN bits included
            assert np.array_equal(gi[:, :, 0], idx), (key, M, r)
            assert np.array_equal(np.stack([gi[:, :, 0] % w, gi[:, :, 0] // w], 2).astype(np.float32), preds)
            assert np.array_equal(gc[:, :, 0, 2:3].view(np.int32), maxvals.view(np.int32))


def test_a_plane_gives_the_same_bits_alone_and_in_its_batch(env, runs):
    for key, f in runs.items():
        gc, gi = f["res"][4, 1]["gpu"]
        for a in range(2):
            for b in range(3):
                view = f["t"][a:a + 1, b:b + 1]                     # where it lies in the batch (15 x 17: not 16-byte aligned)
                for one in (view, view.clone()):
                    c1, i1 = env["inference"].heatmaps_to_candidates(one, 4, 1, return_index=True)
                    assert np.array_equal(c1.cpu().numpy().view(np.int32)[0, 0], gc.view(np.int32)[a, b]), (key, a, b)
                    assert np.array_equal(i1.cpu().numpy()[0, 0], gi[a, b]), (key, a, b)
    f = runs[15, 17, 0]
    assert f["t"][0:1, 1:2].data_ptr() % 16 != 0 and f["t"][0:1, 1:2].is_contiguous()


def test_the_call_replays_from_a_captured_graph(env, runs):
    f = runs[18, 34, 0]
    static = torch.zeros_like(f["t"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        env["inference"].heatmaps_to_candidates(static, 4, 1, return_index=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cand, idx = env["inference"].heatmaps_to_candidates(static, 4, 1, return_index=True)
    for other in (runs[18, 34, 1], f):
        static.copy_(other["t"])
        g.replay()
        torch.cuda.synchronize()
        gc, gi = other["res"][4, 1]["gpu"]
        assert np.array_equal(cand.cpu().numpy().view(np.int32), gc.view(np.int32)) and np.array_equal(idx.cpu().numpy(), gi)


def test_wrong_blob_heatmaps_end_to_end(env):
    """64 x 64 maps of 11 keypoints for 4 images; two keypoints per image have amplitude 1.0 at a wrong place and 0.7 at the true
    one.  The decoder's runner-ups and the native solve mark exactly those two, reach the no-outlier bound of
    tests/test_pnp_native.py (0.05), and the one-candidate pose of the same maps is worse."""
    sc = CR.wrong_blob_scene()
    heat = CR.wrong_blob_heatmaps(sc).cuda()
    cand = env["inference"].heatmaps_to_candidates(heat, 3, 6)
    CR.check_wrong_blob_poses(sc, cand.cpu().numpy())
