"""CPU: the refined candidates in the fused forward and behind the device loader (include/esahrnet.h
esahrnet_forward_keypoints_candidates_refined, esahrnet_frames_keypoints_candidates_refined and their workspace queries; DESIGN.md
5.6.3) are declared, exported and bound with the ABI number unchanged; every refusal of both entries answers in the documented order
with its text, on handles without weights and without a device; the workspace is the candidates forward's plus the stated terms; the
packed record of kind "candidates_refined"; what pipeline.candidate_poses refuses; the marking kernel stays in registers."""
import ctypes as C
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"esahrnet_keypoints_candidates_refined_forward_workspace_bytes": 6, "esahrnet_forward_keypoints_candidates_refined": 19,
           "esahrnet_frames_keypoints_candidates_refined_workspace_bytes": 5, "esahrnet_frames_keypoints_candidates_refined": 30}
MAXC = 4
# the handles the refusals are asked of: name -> (variant, cin, K)
HANDLES = {"seg_hrnet2": (0, 1, 11), "seg_hrnet": (0, 3, 32), "seg_hrnet3": (1, 1, 30)}


def test_header_declares_lib_exports_and_binds_the_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esahrnet.h")).read(), flags=re.S)
    from esa_pose_estimation_amd import _lib as L
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == L.ABI_VERSION
    assert int(re.search(r"#define ESAHRNET_MAX_CANDIDATES (\d+)", header).group(1)) == MAXC == L.MAX_CANDIDATES
    lib, raw = L.lib(), C.CDLL(L.LIB_PATH)
    assert lib.esahrnet_abi_version() == 6
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name            # the declaration's own argument count
        assert name in L.exported_symbols() and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name


def _handle(lib, L, variant=0, cin=1, k=11, precision="fp32"):
    from esa_pose_estimation_amd import config, hrnet
    widths = (16, 16, 32, 64) if variant else (8, 16, 32, 64)
    cfg = hrnet._cfg_struct(config.make_config(widths=widths), cin, k, variant, precision)
    h = C.c_void_p()
    L.check(lib.esahrnet_create(C.byref(cfg), 0, C.byref(h)))
    return h


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


P, ODD4, ODD8 = 0x10000, 0x10002, 0x10004       # pointers that are only numbers: aligned, not 4-byte aligned, not 8-byte aligned


def _ladder(who):
    """The decoder's own refusals, shared by both entries, in the documented order: each row makes its check fire and, where it
    can, a LATER check too, so the row pins which one speaks.  (keywords, text)"""
    w = who.encode()
    return [
        (dict(M=0, r=-1), w + b": 0 candidates per heat-map unsupported (1..4)"),
        (dict(M=5, dec=7), w + b": 5 candidates per heat-map unsupported (1..4)"),
        (dict(r=-1, dec=3), w + b": negative nms_radius -1"),
        (dict(dec=3, hess=P), w + b": decoder=3 unknown (0: get_final, 1: get_final2, 2: gaussfit)"),
        (dict(dec=-1, floor=-1.0), w + b": decoder=-1 unknown (0: get_final, 1: get_final2, 2: gaussfit)"),
        (dict(dec=0, hess=P, floor=-1.0), w + b": decoder 0 (get_final) writes no hess_dev, fit_dev, cov_dev or info_dev: pass NULL"),
        (dict(dec=0, info=P, cand=ODD4), w + b": decoder 0 (get_final) writes no"),
        (dict(dec=1, fit=P, floor=float("nan")), w + b": decoder 1 (get_final2) writes no fit_dev, cov_dev or info_dev: pass NULL"),
        (dict(dec=1, cov=P), w + b": decoder 1 (get_final2) writes no"),
        (dict(dec=2, status=None, floor=float("nan")), w + b": decoder 2 (gaussfit) needs status_dev"),
        (dict(dec=2, floor=-1e-9, cand=ODD4), w + b": cov_floor must be a finite number >= 0"),
        (dict(dec=1, floor=float("nan"), hess=ODD8), w + b": cov_floor must be a finite number >= 0"),
        (dict(dec=0, floor=float("inf")), w + b": cov_floor must be a finite number >= 0"),
        (dict(dec=1, cand=ODD4, hess=ODD8), w + b": cand_dev, cidx_dev and status_dev must be 4-byte aligned"),
        (dict(dec=1, cidx=ODD4), w + b": cand_dev, cidx_dev and status_dev must be 4-byte aligned"),
        (dict(dec=2, status=ODD4, fit=ODD8), w + b": cand_dev, cidx_dev and status_dev must be 4-byte aligned"),
        (dict(dec=1, hess=ODD8), w + b": hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned"),
        (dict(dec=2, fit=ODD8), w + b": hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned"),
        (dict(dec=2, cov=ODD8), w + b": hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned"),
        (dict(dec=2, info=ODD8), w + b": hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned"),
    ]


@pytest.mark.parametrize("name", sorted(HANDLES))
def test_every_refusal_in_the_documented_order_with_its_text(name):
    """Pointers that are only numbers, a handle without weights, no GPU: every call returns non-zero without a launch."""
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    err = lib.esahrnet_last_error
    variant, cin, k = HANDLES[name]
    h = _handle(lib, L, variant, cin, k)
    nb = C.c_size_t()
    try:
        def fwd(hh=h, x=P, n=2, M=3, r=6, dec=2, cand=P, cidx=P, hess=None, fit=None, status=P, cov=None, info=None, floor=1e-6,
                ws=P, wsb=1 << 40):
            return lib.esahrnet_forward_keypoints_candidates_refined(hh, x, n, 48, 80, M, r, dec, cand, cidx, hess, fit, status, cov,
                                                                     info, floor, ws, wsb, None)
        who = "forward_keypoints_candidates_refined"
        # 1. a NULL handle or cand_dev, before M is looked at
        assert fwd(hh=None, M=0) != 0 and err() == who.encode() + b": null argument"
        assert fwd(cand=None, M=0) != 0 and err() == who.encode() + b": null argument"
        # 2.-8. the decoder's own
        for kw, text in _ladder(who):
            assert fwd(**kw) != 0 and err().startswith(text), (kw, err())
        # ... each of them before the forward's ladder (x_dev and ws_dev NULL, no weights: all would be refused later)
        for kw, text in _ladder(who):
            assert fwd(x=None, ws=None, **kw) != 0 and err().startswith(text), (kw, err())
        # 9. the forward's ladder: NULL x_dev / ws_dev, then the commit
        for arg in ("x", "ws"):
            assert fwd(**{arg: None}) != 0 and b"null argument" in err(), arg
        for dec, extra in ((0, dict(status=None)), (0, {}), (1, dict(hess=P, status=None)), (2, dict(hess=P, fit=P, cov=P, info=P))):
            assert fwd(dec=dec, **extra) != 0 and b"esahrnet_commit has not been called" in err(), dec
        assert fwd(cidx=None) != 0 and b"esahrnet_commit has not been called" in err()          # cidx_dev may be NULL here
        assert fwd(floor=0.0) != 0 and b"esahrnet_commit has not been called" in err()
        q = lib.esahrnet_keypoints_candidates_refined_forward_workspace_bytes
        qwho = b"keypoints_candidates_refined_forward_workspace_bytes"
        assert q(h, 2, 48, 80, 3, None) != 0 and err() == qwho + b": null argument"
        assert q(None, 2, 48, 80, 1, C.byref(nb)) != 0 and err() == qwho + b": null argument"
        for dec in (-1, 3):
            assert q(h, 0, 48, 80, dec, C.byref(nb)) != 0 and err().startswith(qwho + b": decoder=%d unknown" % dec)
        assert q(h, 0, 48, 80, 1, C.byref(nb)) != 0 and b"batch must be positive" in err()
        assert q(h, 2, 47, 80, 1, C.byref(nb)) != 0 and b"even" in err()

        def fr(hh=h, frames=P, det=P, m=1, nframes=1, fmt=0, rule=0, std=0.229, M=3, r=6, dec=2, cand=P, cidx=P, hess=None, fit=None,
               status=P, cov=None, info=None, floor=1e-6, boxes=P, rates=P, valid=P, ws=P, wsb=1 << 40, fidx=None):
            return lib.esahrnet_frames_keypoints_candidates_refined(hh, frames, nframes, 1200, 1920, fmt, det, fidx, m, 256, rule, 0.485,
                                                                    std, M, r, dec, cand, cidx, hess, fit, status, cov, info, floor,
                                                                    boxes, rates, valid, ws, wsb, None)
        who = "frames_keypoints_candidates_refined"
        for arg in ("hh", "frames", "det", "cand", "boxes", "rates", "valid", "ws"):
            assert fr(m=0, M=0, **{arg: None}) != 0 and err() == who.encode() + b": null argument", arg
        # the frames' and boxes' arguments come before the decoder's (M = 0 would be refused next)
        assert fr(m=0, M=0) != 0 and b"candidates per heat-map" not in err()
        assert fr(m=-1, M=0) != 0 and b"candidates per heat-map" not in err()
        assert fr(rule=3, M=0) != 0 and b"rule" in err()
        assert fr(fmt=5, M=0) != 0 and b"pixel_format" in err()
        assert fr(std=-1.0, M=0) != 0 and b"stdv" in err()
        assert fr(m=2, M=0) != 0 and b"frame index" in err()
        # the decoder's own, before the handle's commit
        for kw, text in _ladder(who):
            assert fr(**kw) != 0 and err().startswith(text), (kw, err())
        assert fr() != 0 and err() == who.encode() + b": esahrnet_commit has not been called"
        assert fr(cidx=None, dec=1, status=None, hess=P) != 0 and err() == who.encode() + b": esahrnet_commit has not been called"
        fq = lib.esahrnet_frames_keypoints_candidates_refined_workspace_bytes
        assert fq(h, 1, 256, 1, None) != 0 and err() == b"frames_keypoints_candidates_refined_workspace_bytes: null argument"
        assert fq(None, 1, 256, 1, C.byref(nb)) != 0 and b"null argument" in err()
        assert fq(h, 1, 256, 3, C.byref(nb)) != 0 and err().startswith(who.encode() + b": decoder=3 unknown")
        if cin != 1:                            # the loader's refusal, with its existing text
            assert fq(h, 1, 256, 1, C.byref(nb)) != 0
            assert err() == who.encode() + (b": the loader makes 1-channel crops (data_load_val.py / data_load4.py); this handle takes "
                                            b"%d channels" % cin)
            old = lib.esahrnet_frames_keypoints_candidates_workspace_bytes
            assert old(h, 1, 256, C.byref(nb)) != 0 and err().split(b": ", 1)[1] == (
                b"the loader makes 1-channel crops (data_load_val.py / data_load4.py); this handle takes %d channels" % cin)
        else:
            assert fq(h, 0, 256, 1, C.byref(nb)) != 0 and err().startswith(who.encode() + b": scale 256 with 0 boxes")
            assert fq(h, 1, 256, 1, C.byref(nb)) == 0 and nb.value > 0
    finally:
        lib.esahrnet_destroy(h)


@pytest.mark.parametrize("name,precision", [("seg_hrnet2", "fp32"), ("seg_hrnet3", "fp32"), ("seg_hrnet3", "bf16"),
                                            ("seg_hrnet2", "bf16x3"), ("seg_hrnet2", "bf16"), ("seg_hrnet", "fp32")])
def test_workspace_is_the_candidates_forwards_plus_the_stated_terms(name, precision):
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    variant, cin, k = HANDLES[name]
    h = _handle(lib, L, variant, cin, k, precision)
    pad = lambda b: (b + 255) & ~255            # noqa: E731
    try:
        for n, hh, ww in ((1, 64, 64), (3, 80, 112), (32, 256, 256)):
            base, at = C.c_size_t(), C.c_size_t()
            L.check(lib.esahrnet_keypoints_candidates_forward_workspace_bytes(h, n, hh, ww, C.byref(base)))
            got = {}
            for dec in (0, 1, 2):
                nb = C.c_size_t()
                L.check(lib.esahrnet_keypoints_candidates_refined_forward_workspace_bytes(h, n, hh, ww, dec, C.byref(nb)))
                L.check(lib.esahrnet_keypoints_at_workspace_bytes(n, k, hh, ww, dec, C.byref(at)))
                assert at.value == 0 or dec == 1
                assert nb.value == base.value + pad(n * k * MAXC * 4) + (at.value if dec == 1 else 0), (n, hh, ww, dec)
                got[dec] = nb.value
            assert got[0] == got[2] < got[1] and base.value % 256 == 0
        if cin == 1:
            for m, s in ((1, 256), (32, 256), (3, 90)):
                for dec in (0, 1, 2):
                    nb, fwd = C.c_size_t(), C.c_size_t()
                    L.check(lib.esahrnet_frames_keypoints_candidates_refined_workspace_bytes(h, m, s, dec, C.byref(nb)))
                    L.check(lib.esahrnet_keypoints_candidates_refined_forward_workspace_bytes(h, m, s, s, dec, C.byref(fwd)))
                    assert nb.value == fwd.value + pad(m * s * s * 4), (m, s, dec)
    finally:
        lib.esahrnet_destroy(h)


F64 = ("rates", "cand_fit", "cand_hess", "cand_cov", "cand_info")


@pytest.mark.parametrize("gaussfit,cov", [(False, False), (True, False), (True, True)])
def test_the_record_of_the_refined_candidates(gaussfit, cov):
    from esa_pose_estimation_amd import inference
    assert inference.RECORD_KINDS[-1] == "candidates_refined" and inference.RECORD_KINDS[:3] == ("keypoints", "correspondences",
                                                                                                 "candidates")
    want = ["rates"] + (["cand_fit"] if gaussfit else []) + ["cand_hess"] + (["cand_cov", "cand_info"] if cov else []) + \
        ["cand", "boxes", "valid", "cidx"] + (["cand_status"] if gaussfit else [])
    per = {"rates": (8, ()), "cand_fit": (8, ("k", "M", 8)), "cand_hess": (8, ("k", "M", 3)), "cand_cov": (8, ("k", "M", 3)),
           "cand_info": (8, ("k", "M", 3)), "cand": (4, ("k", "M", 3)), "boxes": (4, (4,)), "valid": (4, ()), "cidx": (4, ("k", "M")),
           "cand_status": (4, ("k", "M"))}
    for k in (1, 11, 30):
        for M in (1, 2, 3, 4):
            fields = inference.record_fields(k, "candidates_refined", gaussfit, cov, M)
            assert [n for n, _ in fields] == want                                   # the f64 fields first, then cand .. status
            dims = lambda n: tuple(k if d == "k" else M if d == "M" else d for d in per[n][1])     # noqa: E731
            for n, b in fields:
                assert b % 4 == 0 and b == per[n][0] * int(np.prod(dims(n), dtype=np.int64)), (n, b)
            for m in (1, 2, 3, 5):
                lay = inference.packed_layout(m, k, gaussfit, cov, M, kind="candidates_refined")
                off = 0
                for n, b in fields:
                    assert lay[n] == (off, m * b), (n, m)
                    if n in F64:
                        assert off % 8 == 0, (n, m, k, M)                           # every f64 field 8-byte aligned
                    off += m * b
                assert lay["total"] == (0, off) and list(lay) == want + ["total"]
                # the views round-trip: numpy on a host copy, torch on the buffer, the same places, shapes and types
                host = (np.arange(off) % 251).astype(np.uint8)
                hv = inference.record_views(host, m, k, fields)
                tv = inference.record_views(torch.from_numpy(host), m, k, fields)
                assert list(hv) == want == list(tv)
                for n in want:
                    assert hv[n].shape == (m, *dims(n)) == tuple(tv[n].shape), n
                    assert hv[n].ctypes.data - host.ctypes.data == lay[n][0] and np.shares_memory(hv[n], host), n
                    assert hv[n].dtype == (np.float64 if n in F64 else np.float32 if n == "cand" else np.int32), n
                    assert hv[n].tobytes() == tv[n].numpy().tobytes() == host[lay[n][0]:lay[n][0] + lay[n][1]].tobytes(), n
                # the loader's result gives the same places under the same names; the public return picks them in net.candidates' order
                out = inference.LoaderResult(m, k, {"candidates_refined": (torch.from_numpy(host), fields)})
                assert list(out.views) == want and [out[n].data_ptr() for n in want] == [tv[n].data_ptr() for n in want]
                rest = (["cand_fit", "cand_status"] if gaussfit else []) + ["cand_hess"] + (["cand_cov", "cand_info"] if cov else [])
                assert [t.data_ptr() for t in inference.candidate_returns(out, True, gaussfit, cov)] == \
                    [tv[n].data_ptr() for n in ["cand", "boxes", "rates", "valid"] + rest]
                with pytest.raises(ValueError, match="a record of"):
                    inference.record_views(host[:-4], m, k, fields)
    for bad in (None, 0, 5):
        with pytest.raises(ValueError, match="candidates must be in 1..4"):
            inference.record_fields(11, "candidates_refined", gaussfit, cov, bad)
    with pytest.raises(ValueError, match="cov=True belongs to gaussfit=True"):
        inference.record_fields(11, "candidates_refined", False, True, 3)


def test_the_three_old_kinds_give_what_they_gave():
    from esa_pose_estimation_amd import inference
    with open(os.path.join(ROOT, "tests", "golden", "record_layouts.json")) as f:
        golden = json.load(f)
    kinds = {"keypoints/plain": ("keypoints", False, False), "keypoints/gaussfit": ("keypoints", True, False),
             "keypoints/gaussfit+cov": ("keypoints", True, True), "correspondences": ("correspondences", False, False)}
    for k, rec in golden["record_fields"].items():
        for name, (kind, g, c) in kinds.items():
            assert [list(f) for f in inference.record_fields(int(k), kind, g, c)] == rec[name], (k, name)
    forms = {"plain": (False, False, None), "gaussfit": (True, False, None), "gaussfit+cov": (True, True, None),
             **{f"candidates={M}": (False, False, M) for M in (1, 2, 3, 4)}}
    for key, rec in golden["packed_layout"].items():
        m, k = (int(v) for v in key.split("x"))
        for form, (g, c, M) in forms.items():
            assert [[n, list(v)] for n, v in inference.packed_layout(m, k, g, c, M).items()] == rec[form], (key, form)
            if M is not None:                   # the candidates kind, from record_fields
                off, want = 0, []
                for n, b in inference.record_fields(k, "candidates", candidates=M):
                    want.append([n, [off, m * b]])
                    off += m * b
                assert want + [["total", [0, off]]] == rec[form], (key, form)
    with pytest.raises(ValueError, match=r"candidates=M belongs to the get_final decoder \(gaussfit=False\)"):
        inference.record_fields(11, "candidates", gaussfit=True, candidates=3)       # stays refused
    with pytest.raises(ValueError, match="candidates=M belongs to kind='candidates'"):
        inference.record_fields(11, "keypoints", candidates=2)


def test_python_names_and_what_candidate_poses_refuses():
    import inspect
    from esa_pose_estimation_amd import config, hrnet, pipeline, seg_hrnet2
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64))).eval()
    sig = inspect.signature(pipeline.candidate_poses).parameters
    assert sig["candidates_path"].default == "heatmaps" and sig["frame_idx"].default is None and sig["rule"].default == "val"
    with pytest.raises(ValueError, match=r"candidates_path must be one of \('heatmaps', 'fused', 'loader'\), got 'device'"):
        pipeline.candidate_poses(net, None, None, None, None, candidates_path="device")
    for path in ("heatmaps", "fused"):
        with pytest.raises(ValueError, match="frame_idx and rule belong to candidates_path='loader'"):
            pipeline.candidate_poses(net, None, None, None, None, candidates_path=path, frame_idx=[0, 0])
        with pytest.raises(ValueError, match="frame_idx and rule belong to candidates_path='loader'"):
            pipeline.candidate_poses(net, None, None, None, None, candidates_path=path, rule="train")
    # the argument errors it had come first, on every path, with the texts they had
    for path in ("heatmaps", "fused", "loader", "device"):
        with pytest.raises(ValueError, match="refine must be one of"):
            pipeline.candidate_poses(net, None, None, None, None, refine="taylor", candidates_path=path)
        with pytest.raises(ValueError, match="weights='hessian' needs refine='get_final2' or 'gaussfit'"):
            pipeline.candidate_poses(net, None, None, None, None, refine="get_final", candidates_path=path)
        with pytest.raises(ValueError, match="weights='covariance' needs refine='gaussfit'"):
            pipeline.candidate_poses(net, None, None, None, None, weights="covariance", candidates_path=path)
        with pytest.raises(ValueError, match="cov_floor must be a number >= 0"):
            pipeline.candidate_poses(net, None, None, None, None, cov_floor=-1.0, candidates_path=path)
    # net.candidates / net.frames_to_candidates: the keywords of inference.heatmaps_to_candidates, refused with its texts
    sig = inspect.signature(net.candidates).parameters
    assert [sig[n].default for n in ("candidates", "nms_radius", "return_index", "refine", "return_hessian", "return_fit", "return_cov",
                                     "cov_floor")] == [3, 6, False, "get_final", False, False, False, 1e-6]
    x = torch.zeros(1, 1, 32, 32)
    frames, boxes = torch.zeros(1, 64, 64, dtype=torch.uint8), [[0, 0, 9, 9]]
    for call in (lambda **kw: net.candidates(x, **kw), lambda **kw: net.frames_to_candidates(frames, boxes, scale=64, **kw)):
        with pytest.raises(ValueError, match="refine must be one of"):
            call(refine="taylor")
        with pytest.raises(ValueError, match="return_hessian=True needs refine='get_final2' or 'gaussfit'"):
            call(return_hessian=True)
        with pytest.raises(ValueError, match="return_fit=True and return_cov=True need refine='gaussfit'"):
            call(refine="get_final2", return_cov=True)
        with pytest.raises(ValueError, match="cov_floor must be a number >= 0"):
            call(refine="gaussfit", return_cov=True, cov_floor=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU"):                                # the fused path: no eager fall-back
        net.candidates(x, refine="get_final2")
    kinds = hrnet._Runtime.WS_KINDS
    assert kinds["candidates_refined"][1] == "esahrnet_keypoints_candidates_refined_forward_workspace_bytes"
    assert kinds["frames_candidates_refined"][1] == "esahrnet_frames_keypoints_candidates_refined_workspace_bytes"
    assert kinds["candidates"][1] == "esahrnet_keypoints_candidates_forward_workspace_bytes"


def test_the_added_kernel_uses_no_scratch_memory():
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    usage = json.load(open(b.USAGE))
    new = [k for k in usage if "mark_invalid_refined_kernel" in k]
    assert len(new) == 1 and new[0].startswith("frontend.hip:"), new
    u = usage[new[0]]
    print(new[0], u)
    assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["lds"] == 0
    # the kernels the fused entry launches behind the search are keypoints_at.hip's, and stay what they were: no scratch either
    at = [k for k in usage if k.startswith("keypoints_at.hip:") and "_kernel" in k]
    assert len(at) >= 5, at
    for k in at:
        if "at_final" in k or "at_gaussfit" in k:
            assert usage[k]["scratch"] == 0, (k, usage[k])
    old = [k for k in usage if k.startswith("frontend.hip:") and "mark_invalid_kernel" in k]
    assert len(old) == 1 and usage[old[0]]["scratch"] == 0
