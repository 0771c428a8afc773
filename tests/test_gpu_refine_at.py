"""The decoders at caller-given pixels on the GPU (include/esahrnet.h esahrnet_keypoints_at, esahrnet_keypoints_candidates_refined,
csrc/keypoints_at.hip; inference.refine_at, get_final_at, get_final2_at, heatmaps_to_candidates(refine=...);
pipeline.candidate_poses).

At a plane's arg-max every decoder must give the bits of the arg-max decoder it restates; at a candidate's pixel decoder 0 must give
the candidate kernel's row; anywhere else the outputs are held to the numpy restatements at a given pixel (tests/refine_at_ref.py)
with the tolerances the arg-max decoders' own tests use, and to the reference's outputs on the fixtures of
tests/golden/make_refine_at_golden.py.  Planes of 16 x 16, 20 x 36, 5 x 8, 64 x 64 and 48 x 80, n = 2, k = 3, m = 1..4."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import candidates_ref as CR  # noqa: E402
import final2_ref as F  # noqa: E402
import gaussfit_cov_ref as V  # noqa: E402
import gaussfit_ref as G  # noqa: E402
import refine_at_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (20, 36), (5, 8), (64, 64), (48, 80)]
COORD_TOL = 2e-5                # get_final against its oracle (tests/test_gpu_candidates.py)
REF_TOL = 1e-3                  # get_final2 against the reference's own outputs (tests/test_gpu_final2.py)
HESS_REL_TOL = 2.0 ** -23       # the get_final2 Hessian, relative to its largest entry (tests/test_gpu_correspond.py)
MEASURED_CENTRE = 2.165e-11     # the Gaussian fit against its restatement (tests/test_gpu_gaussfit.py: 4 x these)
MEASURED_ABC = 4.426e-11
NAMES = ("kp", "hess", "fit", "status", "cov", "info")
WRITES = {0: ("kp", "status"), 1: ("kp", "status", "hess"), 2: NAMES}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, crops, inference, pipeline, pnp, seg_hrnet2, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, crops=crops, inference=inference, pipeline=pipeline, pnp=pnp, synth=synth,
                seg_hrnet2=seg_hrnet2)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a, b):
    """Bit-identical tensors (NaN included)."""
    a, b = a.contiguous(), b.contiguous()
    it = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _heat(h, w):
    """f32 [2,3,h,w]: runner-up planes (candidates_ref.planes), rotated blobs (final2_ref), a noisy blob with an offset."""
    rng = np.random.default_rng(100 * h + w)
    if h < 15:                                              # 5 x 8: all guard band but one row; blobs only
        cen = [(rng.uniform(1, w - 2), rng.uniform(1, h - 2)) for _ in range(6)]
        pl = F.gaussian_planes(h, w, cen, 1.5) + rng.uniform(0, 0.05, (6, h, w)).astype(np.float32)
        return np.ascontiguousarray(pl.reshape(2, 3, h, w), np.float32)
    c = CR.planes(h, w)
    cen = [(rng.uniform(4, w - 5), rng.uniform(4, h - 5)) for _ in range(2)]
    rot = F.gaussian_planes(h, w, cen, 2.5, 1.5, [0.4, 2.1])
    rot[1] += 0.6 * F.gaussian_planes(h, w, [(w - 1 - cen[1][0], h - 1 - cen[1][1])], 2.0)[0]
    noisy = (G.blob(h, w, w * 0.4, h * 0.6, 2.0, 1.6, 0.7, 1.0, 0.1)[0] + 0.01 * rng.standard_normal((h, w))).astype(np.float32)
    pl = np.stack([c[0], c[1], c[10], rot[0], rot[1], noisy])           # two-blobs, three-blobs, noisy, ...
    return np.ascontiguousarray(pl.reshape(2, 3, h, w), np.float32)


@pytest.fixture(scope="module")
def heats():
    out = {}
    for hw in SHAPES:
        hm = _heat(*hw)
        out[hw] = dict(hm=hm, t=torch.from_numpy(hm).cuda())
    return out


def _ws(env, n, k, h, w, dec):
    need = C.c_size_t()
    env["L"].check(env["lib"].esahrnet_keypoints_at_workspace_bytes(n, k, h, w, dec, C.byref(need)))
    return need.value


def _outs(shape, fill):
    o = dict(kp=torch.empty((*shape, 3), dtype=torch.float32, device="cuda"), status=torch.empty(shape, dtype=torch.int32, device="cuda"),
             hess=torch.empty((*shape, 3), dtype=torch.float64, device="cuda"), fit=torch.empty((*shape, 8), dtype=torch.float64, device="cuda"),
             cov=torch.empty((*shape, 3), dtype=torch.float64, device="cuda"), info=torch.empty((*shape, 3), dtype=torch.float64, device="cuda"))
    for t in o.values():
        t.view(torch.uint8).fill_(fill)
    return o


def _at(env, heat, at, dec, fill=0xFF, ws_fill=0xFF, floor=V.COV_FLOOR, sync=True):
    """esahrnet_keypoints_at on buffers of the test's own, pre-filled with `fill` bytes -> dict of the outputs decoder `dec` writes
    (+ "unwritten": the others, still as pre-filled)."""
    n, k, h, w = heat.shape
    at = at.reshape(n, k, -1).contiguous()
    m = at.shape[2]
    o = _outs((n, k, m), fill)
    need = _ws(env, n, k, h, w, dec)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda").fill_(ws_fill) if need else None
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256 if need else None
    p = lambda name: o[name].data_ptr() if name in WRITES[dec] else None     # noqa: E731
    env["L"].check(env["lib"].esahrnet_keypoints_at(heat.data_ptr(), n, k, h, w, at.data_ptr(), m, dec, p("kp"), p("hess"), p("fit"),
                                                    p("status"), p("cov"), p("info"), float(floor), ws_ptr, need, _stream()))
    if sync:
        torch.cuda.synchronize()
    o["ws"] = ws
    return o


def _existing(env, heat):
    """The arg-max decoders: esahrnet_keypoints_ex, _final2_hess, _gaussfit_cov -> per decoder a dict like _at's, + idx."""
    inf = env["inference"]
    kp0, idx = inf._keypoints(heat, True)
    kp1, idx1, hess1 = inf._keypoints(heat, True, "get_final2", True)
    kp2, fit, status, hess2, idx2, cov, info = inf._gaussfit(heat, True, True, V.COV_FLOOR)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx1) and torch.equal(idx, idx2)
    return idx, {0: dict(kp=kp0), 1: dict(kp=kp1, hess=hess1), 2: dict(kp=kp2, fit=fit, status=status, hess=hess2, cov=cov, info=info)}


# ---- 1. at the arg-max: the bits of the existing decoders --------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SHAPES)
def test_at_the_arg_max_every_decoder_has_the_existing_decoders_bits(env, heats, hw):
    heat = heats[hw]["t"]
    idx, want = _existing(env, heat)
    for dec in (0, 1, 2):
        got = _at(env, heat, idx, dec)
        for name, ref in want[dec].items():
            assert _bits(got[name].reshape(ref.shape), ref), (hw, dec, name)
        if dec != 2:
            assert (got["status"] == 0).all()
        for name in set(NAMES) - set(WRITES[dec]):          # what a decoder does not write, it does not touch
            assert bool((got[name].view(torch.uint8) == 0xFF).all()), (dec, name)
    if hw == (64, 64):
        assert (want[2]["status"] == 0).any() and torch.isfinite(want[1]["hess"]).any()


# ---- 2. at the candidates' pixels ---------------------------------------------------------------------------------------------------
def _candidates(env, heat, M, r=3, form=None):
    n, k, h, w = heat.shape
    cand = torch.empty((n, k, M, 3), dtype=torch.float32, device="cuda")
    cidx = torch.empty((n, k, M), dtype=torch.int32, device="cuda")
    lib = env["lib"]
    if form is None:
        env["L"].check(lib.esahrnet_keypoints_candidates(heat.data_ptr(), n, k, h, w, M, r, cand.data_ptr(), cidx.data_ptr(), _stream()))
    else:
        env["L"].check(lib.esahrnet_keypoints_candidates_form(heat.data_ptr(), n, k, h, w, M, r, form, cand.data_ptr(), cidx.data_ptr(),
                                                              _stream()))
    torch.cuda.synchronize()
    return cand, cidx


def _refined(env, heat, M, dec, r=3, fill=0xFF):
    n, k, h, w = heat.shape
    o = _outs((n, k, M), fill)
    o["cidx"] = torch.empty((n, k, M), dtype=torch.int32, device="cuda").fill_(-5)
    need = _ws(env, n, k, h, w, dec)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda").fill_(0xFF) if need else None
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256 if need else None
    p = lambda name: o[name].data_ptr() if name in WRITES[dec] else None     # noqa: E731
    env["L"].check(env["lib"].esahrnet_keypoints_candidates_refined(heat.data_ptr(), n, k, h, w, M, r, dec, p("kp"), o["cidx"].data_ptr(),
                                                                    p("hess"), p("fit"), p("status"), p("cov"), p("info"), V.COV_FLOOR,
                                                                    ws_ptr, need, _stream()))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("hw", SHAPES)
def test_at_the_candidates_pixels(env, heats, hw):
    """at = cidx of esahrnet_keypoints_candidates: decoder 0's rows are cand, bit for bit, NaN rows and status -1 where there is no
    candidate; esahrnet_keypoints_candidates_refined is that entry with decoder 0 and the two-call chain with decoders 1 and 2."""
    heat = heats[hw]["t"]
    seen_none = 0
    for M in (1, 2, 3, 4):
        cand, cidx = _candidates(env, heat, M)
        got = _at(env, heat, cidx, 0)
        assert _bits(got["kp"], cand), (hw, M)
        assert torch.equal(got["status"] == -1, cidx == -1) and torch.equal(got["status"] == 0, cidx >= 0)
        seen_none += int((cidx == -1).sum())
        cand_auto, cidx_auto = _candidates(env, heat, M, form=-1)
        assert _bits(cand_auto, cand) and torch.equal(cidx_auto, cidx)
        for dec in (0, 1, 2):
            ref = _refined(env, heat, M, dec)
            assert torch.equal(ref["cidx"], cidx), (hw, M, dec)
            chain = _at(env, heat, cidx, dec)
            for name in WRITES[dec]:
                assert _bits(ref[name], chain[name]), (hw, M, dec, name)
            if dec == 0:
                assert _bits(ref["kp"], cand), (hw, M)
            assert _bits(ref["kp"][..., 2], cand[..., 2]), (hw, M, dec)               # the peak column: the raw value at the pixel
    if max(hw) <= 36:                  # (a larger plane's far field underflows to a plateau of zeros, whose pixels all qualify)
        assert seen_none > 0


# ---- 3. anywhere else: the numpy restatements at the given pixel ------------------------------------------------------------------------
def _pixels(hm, cidx, m=4):
    """at int32 [n,k,m]: the best runner-up (or a random pixel), a pixel next to the arg-max, a random one, one in the guard band."""
    n, k, h, w = hm.shape
    rng = np.random.default_rng(h * 1000 + w)
    at = np.empty((n, k, m), np.int32)
    for i in range(n):
        for j in range(k):
            with np.errstate(all="ignore"):
                bi = int(np.argmax(hm[i, j]))
            py, px = divmod(bi, w)
            near = min(max(py + rng.integers(-2, 3), 0), h - 1) * w + min(max(px + rng.integers(-2, 3), 0), w - 1)
            guard = rng.integers(h) * w + rng.choice([0, 1, w - 2, w - 1])
            run = int(cidx[i, j, 1]) if cidx[i, j, 1] >= 0 else int(rng.integers(h * w))
            at[i, j] = [run, near, rng.integers(h * w), guard][:m]
    return at


@pytest.fixture(scope="module")
def anywhere(env, heats):
    """Per shape: the pixels, the restatements' outputs (computed once) and the GPU's, per decoder."""
    out = {}
    for hw in SHAPES:
        hm, heat = heats[hw]["hm"], heats[hw]["t"]
        _, cidx = _candidates(env, heat, 2)
        at = _pixels(hm, cidx.cpu().numpy())
        t_at = torch.from_numpy(at).cuda()
        out[hw] = dict(at=at, t_at=t_at, ref={d: A.decode_at(hm, at, d) for d in (0, 1, 2)},
                       gpu={d: {k_: v.cpu().numpy() for k_, v in _at(env, heat, t_at, d).items() if k_ in WRITES[d]} for d in (0, 1, 2)})
    return out


@pytest.mark.parametrize("hw", SHAPES)
def test_get_final_anywhere_equals_the_restatement(anywhere, heats, hw):
    g, r, at = anywhere[hw]["gpu"][0], anywhere[hw]["ref"][0], anywhere[hw]["at"]
    hm = heats[hw]["hm"]
    raw = np.take_along_axis(hm.reshape(*hm.shape[:2], -1), at.astype(np.int64), 2)
    assert np.array_equal(g["kp"][..., 2].view(np.int32), raw.view(np.int32))
    assert np.array_equal(np.isnan(g["kp"][..., :2]), np.isnan(r["kp"][..., :2]))
    err = float(np.nanmax(np.abs(g["kp"][..., :2] - r["kp"][..., :2])))
    moved = int((g["kp"][..., 0] != at % hw[1]).sum())
    print(f"{hw}: get_final at given pixels - restatement {err:.3e} px, {moved} of {at.size} rows moved")
    assert err <= COORD_TOL, (hw, err)
    assert (g["status"] == 0).all()


@pytest.mark.parametrize("hw", SHAPES)
def test_get_final2_anywhere_equals_the_restatement(anywhere, heats, hw):
    """tests/test_gpu_final2.py's rule: no step, exactly the integer pixel; a step, within one f32 ulp of the restatement.  The Hessian
    as in tests/test_gpu_correspond.py: NaN exactly where no step, else within 2^-23 of its largest entry."""
    g, r, at = anywhere[hw]["gpu"][1], anywhere[hw]["ref"][1], anywhere[hw]["at"]
    hm = heats[hw]["hm"]
    raw = np.take_along_axis(hm.reshape(*hm.shape[:2], -1), at.astype(np.int64), 2)
    assert np.array_equal(g["kp"][..., 2].view(np.int32), raw.view(np.int32))
    applied = r["applied"]
    integer = np.stack([at % hw[1], at // hw[1]], -1).astype(np.float32)
    np.testing.assert_array_equal(g["kp"][..., :2][~applied], integer[~applied])
    ulp = np.spacing(np.abs(r["kp"][..., :2]))
    err = np.abs(g["kp"][..., :2] - r["kp"][..., :2])
    print(f"{hw}: get_final2 at given pixels: {int(applied.sum())} of {applied.size} steps, max err / ulp {float((err / ulp).max()):.2f}")
    assert np.all(err <= ulp), (hw, float((err / ulp).max()))
    assert np.array_equal(np.isnan(g["hess"]), np.repeat(~applied[..., None], 3, -1))
    if applied.any():
        scale = np.abs(r["hess"][applied]).max(-1, keepdims=True)
        herr = np.abs(g["hess"][applied] - r["hess"][applied])
        assert np.all(herr <= HESS_REL_TOL * scale), (hw, float((herr / scale).max()))
    if hw != (5, 8):
        assert applied.any() and not applied.all()


@pytest.mark.parametrize("hw", SHAPES)
def test_gaussfit_anywhere_equals_the_restatement(anywhere, heats, hw):
    """tests/test_gpu_gaussfit.py's rules: the statuses are the restatement's; a rejected slot keeps decoder 0's row and has NaN fit
    and hess; an accepted fit lies within 4 x the measured deviation of the restatement's (centre, (a, b, c)), hess = -2 (a, b, c)
    of the GPU's own fit, kp = f32 of its centre.  tests/test_gpu_gaussfit_cov.py's: cov and info NaN exactly where the restatement's
    are, info the three lines on the GPU's own cov, and cov against scipy least_squares' no further than 4 x the restatement's own
    distance from it (floor 1e-12)."""
    g, r, at = anywhere[hw]["gpu"][2], anywhere[hw]["ref"][2], anywhere[hw]["at"]
    g0 = anywhere[hw]["gpu"][0]
    hm = heats[hw]["hm"]
    print(hw, "status", g["status"].ravel().tolist())
    assert g["status"].tolist() == r["status"].tolist(), hw
    rej, acc = g["status"] != 0, g["status"] == 0
    assert np.array_equal(g["kp"][rej].view(np.int32), g0["kp"][rej].view(np.int32))
    assert np.array_equal(g["kp"][..., 2].view(np.int32), g0["kp"][..., 2].view(np.int32))
    assert np.isnan(g["fit"][rej]).all() and np.isnan(g["hess"][rej]).all() and np.isfinite(g["fit"][acc]).all()
    assert np.array_equal(g["hess"][acc], -2.0 * g["fit"][acc][:, 3:6])
    assert np.array_equal(g["kp"][acc][:, :2], g["fit"][acc][:, 1:3].astype(np.float32))
    if acc.any():
        dc = float(np.abs(g["fit"][acc][:, 1:3] - r["fit"][acc][:, 1:3]).max())
        dabc = float(np.abs(g["fit"][acc][:, 3:6] - r["fit"][acc][:, 3:6]).max())
        print(f"{hw}: {int(acc.sum())} accepted of {acc.size}; to the restatement: centre {dc:.3e} px, (a, b, c) {dabc:.3e}")
        assert dc <= 4 * MEASURED_CENTRE and dabc <= 4 * MEASURED_ABC, (hw, dc, dabc)
    assert np.array_equal(np.isnan(g["cov"]), np.isnan(r["cov"])) and np.array_equal(np.isnan(g["info"]), np.isnan(r["info"]))
    want = V.info_of(g["cov"])
    assert np.array_equal(np.isnan(g["info"]), np.isnan(want))
    assert np.array_equal(g["info"][~np.isnan(want)].view(np.int64), want[~np.isnan(want)].view(np.int64))
    seen = 0
    for i, j, s in zip(*np.nonzero(~np.isnan(g["cov"][..., 0]))):
        if seen == 3:
            break
        with np.errstate(all="ignore"):                     # (least_squares tries parameters whose exp overflows)
            lsq = V.lsq_pcov(hm[i, j], int(at[i, j, s]))
        d_gpu, d_ref = V.deviation(g["cov"][i, j, s], lsq), V.deviation(r["cov"][i, j, s], lsq)
        print(f"{hw} slot {(i, j, s)}: cov GPU - least_squares {d_gpu:.3e}, restatement - least_squares {d_ref:.3e}")
        assert d_gpu <= max(4 * d_ref, 1e-12), (hw, (i, j, s), d_gpu, d_ref)
        seen += 1
    if hw in ((64, 64), (48, 80)):
        assert acc.any() and rej.any() and seen > 0


def test_the_reference_fixtures_through_get_final_at_and_get_final2_at(env, golden_dir):
    inf = env["inference"]
    files = sorted(glob.glob(os.path.join(golden_dir, "refine_at_*.npz")))
    assert len(files) == 5
    for p in files:
        d = np.load(p)
        hm, coords = d["hm"].copy(), d["coords"].copy()
        out, out2 = inf.get_final_at(hm, coords), inf.get_final2_at(hm, coords)
        np.testing.assert_array_equal(hm, d["hm"])                  # the caller's arrays are not modified
        np.testing.assert_array_equal(coords, d["coords"])
        assert out.shape == d["final"].shape and out.dtype == np.float32 and out2.shape == d["final2"].shape
        e, e2 = float(np.abs(out - d["final"]).max()), float(np.abs(out2 - d["final2"]).max())
        print(f"{os.path.basename(p)}: get_final_at - reference {e:.3e} px, get_final2_at - reference {e2:.3e} px")
        assert e <= COORD_TOL, (p, e)
        assert e2 <= REF_TOL, (p, e2)
        # ... and they differ from the decoders that ignore coords
        assert np.abs(inf.get_final(hm, coords) - d["final"]).max() > 1


# ---- 4. pixels outside the plane ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(16, 16), (5, 8), (48, 80)])
def test_pixels_outside_the_plane_give_nan_rows_and_status_minus_one(env, heats, hw):
    heat = heats[hw]["t"]
    h, w = hw
    idx, _ = _existing(env, heat)
    at = torch.stack([torch.full_like(idx, -1), idx, torch.full_like(idx, h * w), torch.full_like(idx, -7)], -1).contiguous()
    for dec in (0, 1, 2):
        got = _at(env, heat, at, dec)
        alone = _at(env, heat, idx, dec)
        for name in WRITES[dec]:
            out = got[name]
            if name == "status":
                assert (out[:, :, [0, 2, 3]] == -1).all() and torch.equal(out[:, :, 1], alone[name][:, :, 0])
            else:
                assert torch.isnan(out[:, :, [0, 2, 3]]).all(), (dec, name)
                assert _bits(out[:, :, 1], alone[name][:, :, 0]), (dec, name)    # the slot between them is not disturbed


# ---- 5. contracts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", [0, 1, 2])
def test_outputs_are_written_whole_and_inputs_are_only_read(env, heats, anywhere, dec):
    for hw in ((20, 36), (64, 64)):
        heat, at = heats[hw]["t"], anywhere[hw]["t_at"].clone()
        at[0, 0, 3], at[1, 2, 0] = -1, hw[0] * hw[1]
        heat0, at0 = heat.clone(), at.clone()
        a, b = _at(env, heat, at, dec, fill=0xFF, ws_fill=0xFF), _at(env, heat, at, dec, fill=0x00, ws_fill=0x00)
        for name in WRITES[dec]:
            assert _bits(a[name], b[name]), (hw, dec, name)
        assert _bits(heat, heat0) and torch.equal(at, at0)
        if dec == 1:                                                # the workspace's contents do not matter: zeros, NaN, 0xFF
            ws = _at(env, heat, at, dec, ws_fill=0x00)["ws"]
            ws.view(torch.float32)[:ws.numel() // 4].fill_(float("nan"))
            n, k, h, w = heat.shape
            o = _outs(tuple(at.shape), 0x55)
            need = _ws(env, n, k, h, w, 1)
            ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
            env["L"].check(env["lib"].esahrnet_keypoints_at(heat.data_ptr(), n, k, h, w, at.data_ptr(), at.shape[2], 1, o["kp"].data_ptr(),
                                                            o["hess"].data_ptr(), None, o["status"].data_ptr(), None, None, 1e-6, ptr,
                                                            need, _stream()))
            torch.cuda.synchronize()
            for name in WRITES[1]:
                assert _bits(o[name], a[name]), (hw, name)
            # one byte short: refused before anything is enqueued
            rc = env["lib"].esahrnet_keypoints_at(heat.data_ptr(), n, k, h, w, at.data_ptr(), at.shape[2], 1, o["kp"].data_ptr(), None, None,
                                                  None, None, None, 1e-6, ptr, need - 1, _stream())
            assert rc == 1 and f"workspace too small ({need - 1} < {need})" in env["lib"].esahrnet_last_error().decode()


@pytest.mark.parametrize("dec", [0, 1, 2])
def test_a_slot_alone_in_a_batch_and_in_a_permuted_batch(env, heats, anywhere, dec):
    """A slot's bits depend on its plane and its pixel alone: not on n, k, m, nor on its place among the planes or the slots."""
    hw = (48, 80)
    heat, at = heats[hw]["t"], anywhere[hw]["t_at"]
    full = _at(env, heat, at, dec)
    flat, fat = heat.reshape(6, 1, *hw), at.reshape(6, 1, 4)
    perm, sperm = [4, 0, 5, 2, 1, 3], [2, 0, 3, 1]
    shuf = _at(env, flat[perm].reshape(3, 2, *hw).contiguous(), fat[perm][:, :, sperm].reshape(3, 2, 4).contiguous(), dec, fill=0x00)
    for name in WRITES[dec]:
        a = full[name].reshape(6, 4, -1)
        assert _bits(a[perm][:, sperm], shuf[name].reshape(6, 4, -1)), (dec, name)
    for i in (0, 3, 5):
        for s in (0, 2):
            one = _at(env, flat[i:i + 1].contiguous(), fat[i:i + 1, :, s:s + 1].contiguous(), dec)
            for name in WRITES[dec]:
                assert _bits(one[name].reshape(-1), full[name].reshape(6, 4, -1)[i, s]), (dec, name, i, s)


def test_the_calls_replay_from_a_captured_graph(env, heats, anywhere):
    inf = env["inference"]
    hw = (20, 36)
    heat, at = heats[hw]["t"].clone(), anywhere[hw]["t_at"].clone()
    other, other_at = heats[hw]["t"].flip(0).contiguous(), anywhere[hw]["t_at"].flip(0).contiguous()
    calls = [lambda: inf.refine_at(heat, at), lambda: inf.refine_at(heat, at, refine="get_final2", return_hessian=True),
             lambda: inf.refine_at(heat, at, refine="gaussfit", return_fit=True, return_hessian=True, return_cov=True),
             lambda: inf.heatmaps_to_candidates(heat, 3, 3, return_index=True, refine="get_final2", return_hessian=True)]
    for call in calls:
        heat.copy_(heats[hw]["t"])
        at.copy_(anywhere[hw]["t_at"])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            call()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = call()
        heat.copy_(other)
        at.copy_(other_at)
        eager = call()
        g.replay()
        torch.cuda.synchronize()
        out, eager = (out,) if isinstance(out, torch.Tensor) else out, (eager,) if isinstance(eager, torch.Tensor) else eager
        assert len(out) == len(eager) > 0
        for a, b in zip(out, eager):
            assert _bits(a, b)


# ---- 6. the Python forms -------------------------------------------------------------------------------------------------------------
def test_refine_at_returns_and_shapes(env, heats, anywhere):
    inf = env["inference"]
    hw = (16, 16)
    heat, at = heats[hw]["t"], anywhere[hw]["t_at"]
    raw = {d: _at(env, heat, at, d) for d in (0, 1, 2)}
    kp = inf.refine_at(heat, at)
    assert isinstance(kp, torch.Tensor) and _bits(kp, raw[0]["kp"])
    kp, hess = inf.refine_at(heat, at, refine="get_final2", return_hessian=True)
    assert _bits(kp, raw[1]["kp"]) and _bits(hess, raw[1]["hess"])
    assert _bits(inf.refine_at(heat, at, refine="get_final2"), raw[1]["kp"])
    out = inf.refine_at(heat, at, refine="gaussfit", return_fit=True, return_hessian=True, return_cov=True)
    for t, name in zip(out, ("kp", "fit", "status", "hess", "cov", "info")):
        assert _bits(t, raw[2][name]), name
    kp, cov, info = inf.refine_at(heat, at, refine="gaussfit", return_cov=True)
    assert _bits(kp, raw[2]["kp"]) and _bits(cov, raw[2]["cov"]) and _bits(info, raw[2]["info"])
    two = inf.refine_at(heat, at[:, :, 1].contiguous(), refine="get_final2")           # [N,K]: one pixel per plane
    assert two.shape == (2, 3, 3) and _bits(two, raw[1]["kp"][:, :, 1])
    for bad in (at.to(torch.int64), at[:1], at.cpu(), at[:, :, :0]):
        with pytest.raises(ValueError, match="at must be an int32 tensor"):
            inf.refine_at(heat, bad)


@pytest.mark.parametrize("refine", ["get_final2", "gaussfit"])
def test_heatmaps_to_candidates_refined_is_the_search_then_refine_at(env, heats, refine):
    inf = env["inference"]
    for hw in ((20, 36), (64, 64)):
        heat = heats[hw]["t"]
        plain, idx = inf.heatmaps_to_candidates(heat, 3, return_index=True)
        cand, idx2, hess = inf.heatmaps_to_candidates(heat, 3, return_index=True, refine=refine, return_hessian=True)
        kp, hess2 = inf.refine_at(heat, idx, refine=refine, return_hessian=True)
        assert torch.equal(idx2, idx) and _bits(cand, kp) and _bits(hess, hess2)
        assert _bits(cand[..., 2], plain[..., 2]) and not _bits(cand, plain)
        cand3, hess3 = inf.heatmaps_to_candidates(heat, 3, refine=refine, return_hessian=True, form=-1)
        assert _bits(cand3, cand) and _bits(hess3, hess)
        assert _bits(inf.heatmaps_to_candidates(heat, 3, refine=refine), cand)
    out = inf.heatmaps_to_candidates(heat, 2, refine="gaussfit", return_fit=True, return_hessian=True, return_cov=True)
    ref = inf.refine_at(heat, inf.heatmaps_to_candidates(heat, 2, return_index=True)[1], refine="gaussfit", return_fit=True,
                        return_hessian=True, return_cov=True)
    assert len(out) == len(ref) == 6 and all(_bits(a, b) for a, b in zip(out, ref))
    assert _bits(inf.heatmaps_to_candidates(heat, 3, refine="get_final"), plain)      # the defaults are the call it was


def test_candidate_poses_with_get_final_and_peak_weights_is_estimate_poses(env):
    import test_gpu_candidates_forward as TF
    pipeline = env["pipeline"]
    sc = TF._wrong_blob_frames(env)
    net = TF._pattern_net(env, sc["patterns"])
    frames = torch.from_numpy(sc["frames"]).cuda()
    args = (net, frames, sc["bboxes"], sc["kp3d"], sc["K"])
    kw = dict(scale=TF.CROP, on_fail="nan", thresh=0.0, min_k=8, candidates=3, nms_radius=6, return_report=True)
    poses, rep = pipeline.estimate_poses(*args, **kw)
    got, grep = pipeline.candidate_poses(*args, refine="get_final", weights="peak", **kw)
    assert TF._same_poses(got, poses) and rep.rescued.all()
    assert np.array_equal(grep.used, rep.used) and np.array_equal(grep.rescued, rep.rescued)
    assert np.array_equal(grep.raw.view(np.int64), rep.raw.view(np.int64))
    plain = pipeline.candidate_poses(*args, refine="get_final", weights="peak", **dict(kw, return_report=False))
    assert TF._same_poses(plain, poses)
    # the combination estimate_poses refuses: runner-up repair under anisotropic weights.  This net's maps are one-pixel spikes in
    # clutter, nothing a blur or a Gaussian fit is meant for: what is held here is that the entry is the chain it documents, bit for
    # bit (the poses' quality is test_wrong_blob_heatmaps_end_to_end_with_refined_candidates' subject, on blobs)
    inf, pnp = env["inference"], env["pnp"]
    x, boxes, rates = env["crops"].crop_batch(frames, sc["bboxes"], TF.CROP)
    with torch.no_grad():
        heat = net(x)
    for refine, weights in (("get_final2", "hessian"), ("gaussfit", "hessian"), ("gaussfit", "covariance"), ("get_final2", "peak")):
        with pytest.raises(ValueError, match="candidates=3"):
            pipeline.estimate_poses(*args, refine=refine, **kw)
        wp, wrep = pipeline.candidate_poses(*args, refine=refine, weights=weights, **kw)
        out = inf.heatmaps_to_candidates(heat, 3, 6, refine=refine, return_hessian=weights == "hessian",
                                         return_cov=weights == "covariance")
        cand, hess = (out[0], out[-1]) if weights != "peak" else (out, None)
        q, t, used, crep = pnp.candidates_to_pose_batch(cand.cpu().numpy(), sc["kp3d"], sc["K"], [(b[0], b[1]) for b in boxes], rates,
                                                        0.0, 8, 0.3, 0, report=True, hess=None if hess is None else hess.cpu().numpy())
        assert TF._same_poses(wp, [(q[i], t[i]) for i in range(len(wp))]), (refine, weights)
        assert np.array_equal(wrep.used, used) and np.array_equal(wrep.raw.view(np.int64), crep.raw.view(np.int64))
        scores = [pnp.speed_score(q_, t_, pnp.rotation_to_quat_wxyz(R), tt)[0] for (q_, t_), (R, tt) in zip(wp, sc["poses"])]
        print(refine, weights, "SPEED", [round(float(s_), 5) for s_ in scores], "weights that are zero:",
              None if hess is None else int((~torch.isfinite(hess[..., 0])).sum()), "of", cand[..., 0].numel())
        assert (wrep.status == 0).all() and wrep.used.shape == rep.used.shape
        if weights != "peak":
            assert not TF._same_poses(wp, poses)                        # the weights did enter the refinement
    with pytest.raises(ValueError, match="weights='covariance' needs refine='gaussfit'"):
        pipeline.candidate_poses(*args, refine="get_final2", weights="covariance")
    with pytest.raises(ValueError, match="weights='hessian' needs"):
        pipeline.candidate_poses(*args, refine="get_final", weights="hessian")


def _weighted_wrong_blob_check(env, scene, cand, hess):
    """candidates_ref.check_wrong_blob_poses, statement for statement, on the solve that takes the 2x2 weights."""
    pnp = env["pnp"]
    a = (scene["kp3d"], scene["K"], scene["boxes"], scene["rates"])
    q, t, used = pnp.candidates_to_pose_batch(cand, *a, thresh=0.5, min_k=0, hess=hess)
    q1, t1, used1 = pnp.candidates_to_pose_batch(cand[:, :, :1], *a, thresh=0.5, min_k=0, hess=hess[:, :, :1])
    for i, (R, tt) in enumerate(scene["poses"]):
        want = np.zeros(cand.shape[1], np.int32)
        want[scene["bad"][i]] = 1
        assert np.array_equal(used[i], want), (i, used[i], scene["bad"][i])
        assert (used1[i] == 0).all()
        qt = pnp.rotation_to_quat_wxyz(R)
        s, s1 = pnp.speed_score(q[i], t[i], qt, tt)[0], pnp.speed_score(q1[i], t1[i], qt, tt)[0]
        print(f"image {i}: weighted SPEED with one candidate {s1:.5f}, with runner-ups {s:.3e}")
        assert s < 0.05, (i, s)
        assert s1 > s, (i, s1, s)


def test_wrong_blob_heatmaps_end_to_end_with_refined_candidates(env):
    """candidates_ref.check_wrong_blob_poses on the candidates each decoder refines, and its assertions again on the solve that
    weighs them by the decoder's Hessian.  The scene's blobs are noise-free Gaussians: the covariance of their fitted centres is some
    1e-14 px^2, far below the reference's floor of 1e-6, so with the default floor every covariance weight is zero (the numpy oracle
    on the CPU says the same) and the poses are the RANSAC consensus poses, with and without runner-ups: the helper's last clause has
    nothing to compare there, and the covariance weights are checked with cov_floor = 0."""
    inf = env["inference"]
    sc = CR.wrong_blob_scene()
    heat = CR.wrong_blob_heatmaps(sc).cuda()
    cand2, hess2 = inf.heatmaps_to_candidates(heat, 3, 6, refine="get_final2", return_hessian=True)
    CR.check_wrong_blob_poses(sc, cand2.cpu().numpy())
    _weighted_wrong_blob_check(env, sc, cand2.cpu().numpy(), hess2.cpu().numpy())
    candg, hessg, cov, info = inf.heatmaps_to_candidates(heat, 3, 6, refine="gaussfit", return_hessian=True, return_cov=True)
    CR.check_wrong_blob_poses(sc, candg.cpu().numpy())
    _weighted_wrong_blob_check(env, sc, candg.cpu().numpy(), hessg.cpu().numpy())
    assert torch.isnan(info).all() and float(cov[torch.isfinite(cov)].abs().max()) < 1e-6
    _, _, info0 = inf.heatmaps_to_candidates(heat, 3, 6, refine="gaussfit", return_cov=True, cov_floor=0.0)
    assert torch.isfinite(info0[:, :, 0]).all()
    _weighted_wrong_blob_check(env, sc, candg.cpu().numpy(), info0.cpu().numpy())
