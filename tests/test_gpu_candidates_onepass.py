"""The one-sweep candidate kernel (include/esahrnet.h esahrnet_keypoints_candidates_form, csrc/keypoints_candidates_onepass.hip:
form 1, and form -1, what the fused paths launch) against the multi-sweep kernel (form 0) bit for bit, and against the numpy
oracle tests/candidates_ref.py: equal indices, coordinates within the decoder's bound, bit-equal peaks.

Planes: the twelve kinds of tests/test_gpu_candidates.py (candidates_ref.planes; they need 15 x 16 pixels, so every shape but
5 x 8 has them) and the kinds below, which aim at the table of per-cell bests: two maxima in one 8 x 8 cell with the higher one
suppressed, equal maxima in one cell and in adjacent cells, a maximum on a cell corner, noise quantised to 8 levels, peaks
whose suppression squares leave the plane.  Shapes: 16 x 16; 20 x 36 (H no multiple of 8, the last cell column half a cell); 5 x 8
(fewer rows than a cell); 64 x 64; 15 x 264 (a row goes on past a wave's 256 columns); 18 x 34 and an unaligned 15 x 17 view, which
the one-sweep kernel does not serve: form -1 equals form 0 there and form 1 is refused.  M in {1, 2, 4}, r in {0, 1, 6, 64}.

The oracle is evaluated once per plane and radius at M = 4: its rows are chosen one after the other, so the rows of a smaller M
are the first M of them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import candidates_ref as CR  # noqa: E402
from test_gpu_candidates import COORD_TOL, MS, RS, _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

ELIGIBLE = [(16, 16), (20, 36), (5, 8), (64, 64), (15, 264)]
INELIGIBLE = [(15, 17), (18, 34)]


def extra_planes(h, w, seed=0):
    """name -> f32 [h,w]: the kinds of this file that fit into h x w."""
    rng = np.random.default_rng(seed + 77 * h + w)
    out = {}
    out["quantised"] = np.floor(rng.random((h, w)) * 8) / 8                     # plateaux, many ties
    out["noise"] = rng.random((h, w))
    p = 0.2 * rng.random((h, w))                                                  # squares that leave the plane on every side
    p[0, 0], p[h - 1, w - 1], p[0, w - 1], p[h - 1, 0] = 1.0, 0.9, 0.8, 0.7
    out["leaving"] = p
    p = np.full((h, w), 0.1)                                                      # one cell, three maxima: each choice must reveal
    p[1, 6], p[3, 1], p[1, 4] = 0.9, 0.5, 1.0                                     # the next one of the same cell
    out["small-pair"] = p
    if h < 15 or w < 16:
        return out
    p = np.zeros((h, w))                                                          # peak in cell (0, 1); cell (0, 0) holds A = 0.9 at
    p[3, 9], p[3, 6], p[1, 1] = 1.0, 0.9, 0.5                                     # distance 3 of it and B = 0.5 at distance 8: at
    out["cell-pair"] = p                                                          # r = 6 the stored best A is wrong until rescanned
    p = np.zeros((h, w))                                                          # the same with the pair's cell two rows down and
    p[11, 12], p[13, 9], p[9, 14], p[4, 3] = 1.0, 0.9, 0.9, 0.6                    # the partners in the peak's own cell
    out["cell-pair-2"] = p
    p = np.full((h, w), 0.1)                                                      # equal maxima: two in cell (0, 0), one in each of
    p[2, 2] = p[5, 5] = p[2, 10] = p[10, 2] = 0.8                                 # the cells right of it and below it
    p[13, 13] = 1.0
    out["ties"] = p
    p = np.full((h, w), 0.05)                                                     # (7, 7): its 8 neighbours lie in four cells; (8, 8)
    p[7, 7] = p[8, 8] = 0.9                                                       # ties with it across the corner; a slope beside them
    p[7, 8], p[8, 7] = 0.5, 0.9
    p[12, 3] = 1.0
    out["cell-corner"] = p
    return out


def all_planes(h, w):
    extra = extra_planes(h, w)
    names, planes = list(extra), [extra[n] for n in extra]
    if h >= 15 and w >= 16:
        names = list(CR.NAMES) + names
        planes = list(CR.planes(h, w)) + planes
    return names, np.ascontiguousarray(np.stack(planes).astype(np.float32)[None])      # [1, P, h, w]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, inference
    return dict(inference=inference, L=_lib)


def _run(env, t, M, r, form):
    cand, idx = env["inference"].heatmaps_to_candidates(t, M, r, return_index=True, form=form)
    return cand.cpu().numpy(), idx.cpu().numpy()


@pytest.fixture(scope="module")
def runs(env):
    """Per shape: names, the batch (numpy and cuda), per r the oracle at M = 4, per (M, r, form) the GPU's (cand, idx)."""
    out = {}
    for (h, w) in ELIGIBLE + INELIGIBLE:
        names, hm = all_planes(h, w)
        t = torch.from_numpy(hm).cuda()
        forms = (0, 1, -1) if (h, w) in ELIGIBLE else (0, -1)
        ref = {r: CR.candidates(hm, 4, r) for r in RS}
        gpu = {(M, r, f): _run(env, t, M, r, f) for M in MS for r in RS for f in forms}
        out[h, w] = dict(names=names, hm=hm, t=t, ref=ref, gpu=gpu, forms=forms)
    return out


def test_the_oracle_rows_are_what_the_cases_are_for(runs):
    """Asserted on the oracle, so that a case cannot degrade silently."""
    for shape in ((64, 64), (15, 264)):
        f = runs[shape]
        for name in ("noisy", "noise", "quantised"):
            for r in (0, 1, 6):
                assert (f["ref"][r][1][0, f["names"].index(name)] >= 0).all(), (shape, name, r)      # M real candidates
    for shape, f in runs.items():
        at = lambda name, r: f["ref"][r][1][0, f["names"].index(name)]                               # noqa: E731
        if max(shape) <= 65:                                                                         # r = 64 covers the plane
            assert (f["ref"][64][1][0, :, 1:] == -1).all() and np.isnan(f["ref"][64][0][0, :, 1:]).all(), shape
        if "constant" in f["names"]:
            assert at("all-nan", 0).tolist() == [0, -1, -1, -1] and at("all-neg-inf", 6).tolist() == [0, -1, -1, -1]
            assert (at("constant", 1) >= 0).all()
        if "cell-pair" in f["names"]:
            w = shape[1]
            assert at("cell-pair", 6).tolist()[:2] == [3 * w + 9, 1 * w + 1]                           # A suppressed, B the runner-up
            assert at("cell-pair", 1).tolist()[:3] == [3 * w + 9, 3 * w + 6, 1 * w + 1]                # A, then B from A's cell
            assert at("cell-pair-2", 6).tolist()[:2] == [11 * w + 12, 4 * w + 3]
            assert at("cell-pair-2", 1).tolist() == [11 * w + 12, 9 * w + 14, 13 * w + 9, 4 * w + 3]   # the tie: lower index first
            assert at("ties", 1).tolist() == [13 * w + 13, 2 * w + 2, 2 * w + 10, 5 * w + 5]
            assert at("cell-corner", 0).tolist() == [12 * w + 3, 7 * w + 7, 8 * w + 7, 8 * w + 8]
        assert at("small-pair", 1).tolist()[:3] == [shape[1] + 4, shape[1] + 6, 3 * shape[1] + 1]      # (3, 1) from (1, 6)'s cell
        assert at("leaving", 6).tolist()[:2] == [0, shape[0] * shape[1] - 1]


def test_forms_one_and_auto_have_the_bits_of_form_zero(runs):
    for shape, f in runs.items():
        for M in MS:
            for r in RS:
                c0, i0 = f["gpu"][M, r, 0]
                for form in f["forms"][1:]:
                    c, i = f["gpu"][M, r, form]
                    bad = [f["names"][p] for p in range(len(f["names"])) if not (_same_bits(c[0, p], c0[0, p]) and
                                                                                np.array_equal(i[0, p], i0[0, p]))]
                    assert not bad, (shape, M, r, form, bad)


def test_indices_coordinates_and_peaks_equal_the_oracle(runs):
    worst = 0.0
    for shape, f in runs.items():
        for (M, r, form), (gc, gi) in f["gpu"].items():
            rc, ri = f["ref"][r][0][:, :, :M], f["ref"][r][1][:, :, :M]
            assert gi.tolist() == ri.tolist(), (shape, M, r, form)
            assert _same_bits(gc[..., 2], rc[..., 2]), (shape, M, r, form)
            assert np.array_equal(np.isnan(gc[..., :2]), np.isnan(rc[..., :2])), (shape, M, r, form)
            err = float(np.nanmax(np.abs(gc[..., :2].astype(np.float64) - rc[..., :2]), initial=0.0))
            worst = max(worst, err)
            assert err <= COORD_TOL, (shape, M, r, form, err)
    print(f"largest coordinate difference to the oracle: {worst:.3e} px")


def test_form_one_is_refused_on_planes_it_does_not_serve(env, runs):
    f = runs[18, 34]
    view = runs[15, 17]["t"][0:1, 1:2]                          # 255 floats in: not 16-byte aligned
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    big = torch.zeros((1, 1, 8, 8 * 4097), device="cuda")       # 4097 cells
    for t in (f["t"], view, big):
        with pytest.raises(env["L"].EsaHrnetError, match="form 1"):
            env["inference"].heatmaps_to_candidates(t, 2, 1, form=1)
    # the unaligned view: form -1 gives what form 0 gives, which is what the plane gives in its batch
    c0, i0 = _run(env, view, 4, 1, 0)
    c1, i1 = _run(env, view, 4, 1, -1)
    assert _same_bits(c0, c1) and np.array_equal(i0, i1)
    assert _same_bits(c0[0, 0], runs[15, 17]["gpu"][4, 1, 0][0][0, 1])
    # the widest plane the table holds (4096 cells) is served; one more cell column takes the multi-sweep kernel under form -1
    ok = torch.rand((1, 1, 8, 8 * 4096), device="cuda")
    assert _same_bits(*[_run(env, ok, 3, 6, form)[0] for form in (0, 1)])
    big.copy_(torch.rand_like(big))
    assert _same_bits(*[_run(env, big, 3, 6, form)[0] for form in (0, -1)])
    for bad in (2, -2):
        with pytest.raises(env["L"].EsaHrnetError, match="form"):
            env["inference"].heatmaps_to_candidates(ok, 2, 1, form=bad)


def test_a_plane_gives_the_same_bits_alone_and_in_its_batch(env, runs):
    for shape in ELIGIBLE:
        f = runs[shape]
        gc, gi = f["gpu"][4, 1, 1]
        for p in range(len(f["names"])):
            c1, i1 = _run(env, f["t"][:, p:p + 1].clone(), 4, 1, 1)
            assert _same_bits(c1[0, 0], gc[0, p]) and np.array_equal(i1[0, 0], gi[0, p]), (shape, f["names"][p])


def test_the_call_replays_from_a_captured_graph(env, runs):
    f = runs[20, 36]
    other = torch.flip(f["t"], dims=(1,)).contiguous()          # the same planes in another order
    static = torch.zeros_like(f["t"])
    call = lambda: env["inference"].heatmaps_to_candidates(static, 4, 6, return_index=True, form=1)     # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cand, idx = call()
    gc, gi = f["gpu"][4, 6, 0]
    for t, order in ((other, slice(None, None, -1)), (f["t"], slice(None))):
        static.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        assert _same_bits(cand.cpu().numpy(), gc[:, order]) and np.array_equal(idx.cpu().numpy(), gi[:, order])


def test_a_second_call_overwrites_every_element(env, runs):
    """Raw calls into the same two output buffers, pre-filled with a pattern: first r = 64 (NaN rows), then r = 1."""
    lib, L = env["L"].lib(), env["L"]
    for shape in ((64, 64), (5, 8)):
        f = runs[shape]
        t = f["t"]
        _, k, h, w = t.shape
        cand = torch.empty((1, k, 4, 3), dtype=torch.float32, device="cuda")
        idx = torch.empty((1, k, 4), dtype=torch.int32, device="cuda")
        for r in (64, 1):
            cand.view(torch.uint8).fill_(0xA5)
            idx.view(torch.uint8).fill_(0xA5)
            L.check(lib.esahrnet_keypoints_candidates_form(t.data_ptr(), 1, k, h, w, 4, r, 1, cand.data_ptr(), idx.data_ptr(),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            gc, gi = f["gpu"][4, r, 0]
            assert _same_bits(cand.cpu().numpy(), gc) and np.array_equal(idx.cpu().numpy(), gi), (shape, r)
