"""CPU: the decoders at caller-given pixels (include/esahrnet.h esahrnet_keypoints_at, esahrnet_keypoints_candidates_refined;
inference.refine_at, get_final_at, get_final2_at).  The numpy restatements at a given pixel (tests/refine_at_ref.py) are held to the
REAL reference's get_final(hm, coords) / get_final2(hm, coords) on fixtures whose coords are not the arg-max
(tests/golden/refine_at_*.npz, make_refine_at_golden.py), and every refusal of the two entries answers, with its text, before
anything touches a device."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_at_ref as A  # noqa: E402

from esa_pose_estimation_amd import _lib, inference  # noqa: E402

REF_TOL = 1e-3          # px: get_final2's restatement against the reference's own outputs (tests/test_final2_host.py)
COORD_TOL = 2e-5        # px: get_final against its oracle (tests/test_gpu_candidates.py)
CASES = ("second_blob", "slope", "guard", "det0", "nonsquare")
ENTRIES = ("esahrnet_keypoints_at_workspace_bytes", "esahrnet_keypoints_at", "esahrnet_keypoints_candidates_refined")


def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "refine_at_*.npz")))
    assert [os.path.basename(f)[len("refine_at_"):-4] for f in files] == sorted(CASES)
    return {os.path.basename(f)[len("refine_at_"):-4]: np.load(f) for f in files}


def at_of(d):
    w = d["hm"].shape[3]
    return (d["coords"][:, 1].astype(np.int64) * w + d["coords"][:, 0].astype(np.int64)).astype(np.int32)


def test_fixtures_are_off_the_arg_max_and_cover_the_cases(golden_dir):
    fx = fixtures(golden_dir)
    for name, d in fx.items():
        hm, at = d["hm"], at_of(d)
        assert hm.dtype == np.float32 and hm.shape[0] == 1 and max(hm.shape[2:]) <= 80, name
        assert not (at == hm[0].reshape(hm.shape[1], -1).argmax(1)).any(), name
        assert os.path.getsize(os.path.join(golden_dir, f"refine_at_{name}.npz")) < 64 * 1024
    assert fx["nonsquare"]["hm"].shape[2:] == (48, 80)
    s = fx["slope"]
    stay = (s["final"] == s["coords"]).all(1)
    assert stay.any() and not stay.all()                        # my_taylor's offset >= 1: no step; the other pixels step
    assert (np.abs(s["final2"] - s["coords"]).max(1) > 2).all()  # get_final2 steps from every one of them
    g = fx["guard"]
    assert (g["final"] == g["coords"]).all() and (g["final2"] == g["coords"]).all()
    assert (fx["det0"]["final2"] == fx["det0"]["coords"]).all()


def test_restatements_equal_the_reference_at_the_given_pixels(golden_dir):
    for name, d in fixtures(golden_dir).items():
        hm, at = d["hm"], at_of(d)
        got0 = np.stack([A.final_at(hm[0, j], int(a)) for j, a in enumerate(at)])
        got1 = [A.final2_at(hm[0, j], int(a)) for j, a in enumerate(at)]
        e0 = np.abs(got0[:, :2] - d["final"]).max()
        e1 = np.abs(np.stack([g[0][:2] for g in got1]) - d["final2"]).max()
        print(f"{name}: get_final restatement - reference {e0:.3e} px, get_final2 {e1:.3e} px")
        assert e0 <= COORD_TOL, (name, e0)
        assert e1 <= REF_TOL, (name, e1)
        raw = hm[0].reshape(hm.shape[1], -1)[np.arange(len(at)), at]
        assert np.array_equal(got0[:, 2], raw) and np.array_equal(np.stack([g[0][2] for g in got1]), raw)
        for (kp, hess, applied), c in zip(got1, d["coords"]):
            assert np.isnan(hess).all() == (not applied) and (applied or (kp[:2] == c).all())
    # the restatement at the arg-max is the arg-max restatement
    import final2_ref as F
    d = np.load(os.path.join(golden_dir, "final2_rotated.npz"))
    for pl in d["hm"][0]:
        kp, bi, applied = F.decode_plane(pl)
        kp2, _, ap2 = A.final2_at(pl, bi)
        assert np.array_equal(kp, kp2) and applied == ap2


def test_a_pixel_outside_the_plane_is_a_nan_row():
    pl = np.ones((8, 9), np.float32)
    for a in (-1, 72, -7):
        assert np.isnan(A.final_at(pl, a)).all() and np.isnan(A.final2_at(pl, a)[0]).all()
        r = A.gaussfit_at(pl, a)
        assert r["status"] == -1 and all(np.isnan(r[n]).all() for n in ("kp", "fit", "hess", "cov", "info"))
    o = A.decode_at(pl[None, None], np.array([[[-1, 40]]]), 2)
    assert o["status"].tolist() == [[[-1, 2]]]                  # a constant plane: the fit is rejected, the row kept
    assert np.array_equal(o["kp"][0, 0, 1], [4, 4, 1])


# ---- the entries' refusals: all before anything is enqueued, so none of this touches a device ----------------------------------------
def test_entries_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "esahrnet.h")).read()
    raw = _lib.lib()
    for name in ENTRIES:
        assert f"int {name}(" in header and name in _lib.exported_symbols() and hasattr(raw, name), name
    assert raw.esahrnet_abi_version() == 6
    from esa_pose_estimation_amd import build
    assert "keypoints_at.hip" in build.SOURCES


def _err(rc):
    assert rc == 1
    return _lib.lib().esahrnet_last_error().decode()


def test_workspace_query():
    L = _lib.lib()
    b, f2 = C.c_size_t(7), C.c_size_t()
    for m in (1, 4):                                            # it does not know m: it cannot grow with it
        for dec, want in ((0, 0), (2, 0)):
            _lib.check(L.esahrnet_keypoints_at_workspace_bytes(2, 3, 64, 64, dec, C.byref(b)))
            assert b.value == want
    _lib.check(L.esahrnet_keypoints_at_workspace_bytes(32, 11, 256, 256, 1, C.byref(b)))
    _lib.check(L.esahrnet_keypoints_final2_workspace_bytes(32, 11, 256, 256, C.byref(f2)))
    assert b.value == f2.value > 0
    assert "null argument" in _err(L.esahrnet_keypoints_at_workspace_bytes(1, 1, 8, 8, 0, None))
    assert "bad shape" in _err(L.esahrnet_keypoints_at_workspace_bytes(0, 1, 8, 8, 0, C.byref(b)))
    assert "decoder=3 unknown" in _err(L.esahrnet_keypoints_at_workspace_bytes(1, 1, 8, 8, 3, C.byref(b)))


def test_every_refusal_of_keypoints_at_with_its_text_in_the_documented_order():
    L = _lib.lib()
    buf = (C.c_double * 1024)()
    base = C.addressof(buf)
    base += (-base) % 256
    p, odd4, odd8 = C.c_void_p(base), C.c_void_p(base + 2), C.c_void_p(base + 4)

    def call(heat=p, n=1, k=1, h=16, w=16, at=p, m=1, dec=0, kp=p, hess=None, fit=None, status=None, cov=None, info=None,
             floor=1e-6, ws=None, ws_bytes=0):
        return L.esahrnet_keypoints_at(heat, n, k, h, w, at, m, dec, kp, hess, fit, status, cov, info, floor, ws, ws_bytes, None)

    need = C.c_size_t()
    _lib.check(L.esahrnet_keypoints_at_workspace_bytes(1, 1, 16, 16, 1, C.byref(need)))
    # each row violates its own rule AND every later one it can: the earlier rule answers
    rows = [(dict(heat=None, n=0), "keypoints_at: null argument"),
            (dict(at=None, m=0), "keypoints_at: null argument"),
            (dict(kp=None, dec=9), "keypoints_at: null argument"),
            (dict(n=0, m=0), "keypoints_at: bad shape 0 x 1 x 16 x 16"),
            (dict(h=-1, dec=5), "keypoints_at: bad shape 1 x 1 x -1 x 16"),
            (dict(h=65536, w=65536), "keypoints_at: bad shape 1 x 1 x 65536 x 65536"),
            (dict(m=0, dec=7), "keypoints_at: 0 pixels per heat-map unsupported"),
            (dict(n=1 << 20, k=1 << 10, m=4), "keypoints_at: 4 pixels per heat-map unsupported"),
            (dict(dec=3, hess=p), "keypoints_at: decoder=3 unknown (0: get_final, 1: get_final2, 2: gaussfit)"),
            (dict(dec=-1), "keypoints_at: decoder=-1 unknown"),
            (dict(dec=0, hess=p, floor=-1.0), "keypoints_at: decoder 0 (get_final) writes no hess_dev, fit_dev, cov_dev or info_dev"),
            (dict(dec=0, info=p), "keypoints_at: decoder 0 (get_final) writes no"),
            (dict(dec=1, fit=p, ws=p, ws_bytes=need.value), "keypoints_at: decoder 1 (get_final2) writes no fit_dev, cov_dev or info_dev"),
            (dict(dec=1, cov=p, ws=p, ws_bytes=need.value), "keypoints_at: decoder 1 (get_final2) writes no"),
            (dict(dec=2, floor=float("nan")), "keypoints_at: decoder 2 (gaussfit) needs status_dev"),
            (dict(dec=2, status=p, floor=-1e-9, kp=odd4), "keypoints_at: cov_floor must be a finite number >= 0"),
            (dict(floor=float("nan")), "keypoints_at: cov_floor must be a finite number >= 0"),
            (dict(floor=float("inf")), "keypoints_at: cov_floor must be a finite number >= 0"),
            (dict(kp=odd4, dec=1), "keypoints_at: heat_dev, at_dev, kp_dev and status_dev must be 4-byte aligned"),
            (dict(at=odd4), "keypoints_at: heat_dev, at_dev, kp_dev and status_dev must be 4-byte aligned"),
            (dict(status=odd4), "keypoints_at: heat_dev, at_dev, kp_dev and status_dev must be 4-byte aligned"),
            (dict(dec=1, hess=odd8), "keypoints_at: hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned"),
            (dict(dec=2, status=p, info=odd8), "keypoints_at: hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned"),
            (dict(dec=1), f"keypoints_at: workspace too small (0 < {need.value})"),
            (dict(dec=1, ws=p, ws_bytes=need.value - 1), f"keypoints_at: workspace too small ({need.value - 1} < {need.value})"),
            (dict(dec=1, ws=C.c_void_p(base + 128), ws_bytes=need.value), "keypoints_at: workspace must be 256-byte aligned"),
            (dict(dec=1, n=1 << 12, k=1 << 11, ws=p, ws_bytes=1 << 40), "too many tiles for one launch")]
    for kw, text in rows:
        assert text in _err(call(**kw)), (kw, text)


def test_refusals_of_candidates_refined():
    L = _lib.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 256)

    def call(heat=p, n=1, k=1, h=16, w=16, M=3, r=6, dec=0, cand=p, cidx=p, hess=None, fit=None, status=None, cov=None, info=None,
             floor=1e-6, ws=None, ws_bytes=0):
        return L.esahrnet_keypoints_candidates_refined(heat, n, k, h, w, M, r, dec, cand, cidx, hess, fit, status, cov, info, floor, ws,
                                                       ws_bytes, None)

    for kw, text in [(dict(cidx=None), "keypoints_candidates_refined: null argument (cidx_dev is required here)"),
                     (dict(cand=None), "keypoints_candidates_refined: null argument"),
                     (dict(w=0), "keypoints_candidates_refined: bad shape 1 x 1 x 16 x 0"),
                     (dict(M=0), "keypoints_candidates_refined: 0 candidates per heat-map unsupported (1..4)"),
                     (dict(M=5), "keypoints_candidates_refined: 5 candidates per heat-map unsupported (1..4)"),
                     (dict(r=-1, dec=4), "keypoints_candidates_refined: negative nms_radius -1"),
                     (dict(dec=4), "keypoints_candidates_refined: decoder=4 unknown"),
                     (dict(dec=0, hess=p), "keypoints_candidates_refined: decoder 0 (get_final) writes no"),
                     (dict(dec=2), "keypoints_candidates_refined: decoder 2 (gaussfit) needs status_dev"),
                     (dict(dec=1), "keypoints_candidates_refined: workspace too small")]:
        assert text in _err(call(**kw)), (kw, text)


def test_python_refusals_need_no_device():
    hm = np.zeros((1, 2, 8, 9), np.float32)
    ok = np.array([[3, 4], [8, 7]], np.float32)
    for bad, text in ((np.array([[3.5, 4], [1, 1]]), "integer-valued"), (np.array([[np.nan, 4], [1, 1]]), "integer-valued"),
                      (np.array([[9, 4], [1, 1]]), "outside the 8 x 9 plane"), (np.array([[3, 8], [1, 1]]), "outside"),
                      (np.array([[-1, 0], [1, 1]]), "outside"), (ok[:1], r"coords must be \[2, 2\]")):
        for fn in (inference.get_final_at, inference.get_final2_at):
            with pytest.raises(ValueError, match=text):
                fn(hm, bad)
    assert inference._coords_to_at(hm, ok).tolist() == [[4 * 9 + 3, 7 * 9 + 8]]
    heat, at = torch.zeros(1, 2, 8, 9), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="refine must be one of"):
        inference.refine_at(heat, at, refine="taylor")
    with pytest.raises(ValueError, match="get_final computes no Hessian"):
        inference.refine_at(heat, at, return_hessian=True)
    for kw in (dict(return_fit=True), dict(return_cov=True), dict(refine="get_final2", return_cov=True)):
        with pytest.raises(ValueError, match="need refine='gaussfit'"):
            inference.refine_at(heat, at, **kw)
    with pytest.raises(ValueError, match="cov_floor"):
        inference.refine_at(heat, at, refine="gaussfit", cov_floor=-1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        inference.refine_at(heat, at)
    with pytest.raises(ValueError, match="4-D tensor"):
        inference.refine_at(heat[0], at)
    with pytest.raises(ValueError, match="need refine='gaussfit'"):
        inference.heatmaps_to_candidates(heat, 3, return_fit=True)
    with pytest.raises(ValueError, match="takes form None or -1"):
        inference.heatmaps_to_candidates(heat, 3, form=1, refine="get_final2")
    with pytest.raises(RuntimeError, match="GPU only"):
        inference.heatmaps_to_candidates(heat, 3, refine="get_final2", return_hessian=True)
