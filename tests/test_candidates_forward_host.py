"""CPU: runner-up peaks in the fused forward and behind the device loader (include/esahrnet.h esahrnet_keypoints_candidates_form,
esahrnet_forward_keypoints_candidates, esahrnet_frames_keypoints_candidates and the two workspace queries) are declared, exported
and bound with the ABI number unchanged; every argument error answers with its text before anything touches a GPU; the workspace is
the forward's plus the padded heat-maps; the packed record of the loader; what pipeline.estimate_poses refuses; the one-sweep
kernel uses neither scratch memory nor spills and its cell table is what the header says."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"esahrnet_keypoints_candidates_form": 11, "esahrnet_keypoints_candidates_forward_workspace_bytes": 5,
           "esahrnet_forward_keypoints_candidates": 12, "esahrnet_frames_keypoints_candidates_workspace_bytes": 4,
           "esahrnet_frames_keypoints_candidates": 23}


def test_header_declares_lib_exports_and_binds_the_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esahrnet.h")).read(), flags=re.S)
    from esa_pose_estimation_amd import _lib as L
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == L.ABI_VERSION
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
    widths = (16, 16, 32, 64) if variant else (16, 32, 64, 128)
    cfg = hrnet._cfg_struct(config.make_config(widths=widths), cin, k, variant, precision)
    h = C.c_void_p()
    L.check(lib.esahrnet_create(C.byref(cfg), 0, C.byref(h)))
    return h


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


def test_argument_errors_are_reported_before_anything_is_enqueued():
    """Pointers that are only numbers, a handle without weights, no GPU: every call returns non-zero without a launch."""
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    err = lib.esahrnet_last_error
    h = _handle(lib, L)
    h3 = _handle(lib, L, cin=3, k=32)
    p = 0x10000
    nb = C.c_size_t()
    try:
        # the stand-alone entry: the checks and texts of esahrnet_keypoints_candidates, then the form's
        def form(heat=p, n=2, hh=64, ww=64, M=3, r=6, f=1, cand=p, cidx=p):
            return lib.esahrnet_keypoints_candidates_form(heat, n, 11, hh, ww, M, r, f, cand, cidx, None)

        def old(heat=p, n=2, hh=64, ww=64, M=3, r=6, cand=p, cidx=p):
            return lib.esahrnet_keypoints_candidates(heat, n, 11, hh, ww, M, r, cand, cidx, None)
        for kw in (dict(heat=None), dict(cand=None), dict(n=0), dict(hh=0), dict(ww=-4), dict(M=0), dict(M=5), dict(r=-1),
                   dict(heat=p + 2), dict(cand=p + 1), dict(cidx=p + 2)):
            assert old(**kw) != 0
            text = err()
            for f in (-1, 0, 1):
                assert form(f=f, **kw) != 0 and err() == text, (kw, f)
        assert form(M=5) != 0 and b"5 candidates per heat-map unsupported (1..4)" in err()
        assert form(r=-3) != 0 and b"negative nms_radius -3" in err()
        assert form(cand=None) != 0 and b"null argument" in err()
        assert form(cidx=p + 2) != 0 and b"4-byte aligned" in err()
        for f in (-2, 2, 7):
            assert form(f=f) != 0 and b"form=%d unknown" % f in err()
        # form 1 on a plane the one-sweep kernel does not serve: unaligned, a width that is no multiple of 4, too many cells
        for kw in (dict(heat=p + 4), dict(ww=34), dict(hh=8, ww=8 * 4097), dict(hh=520, ww=512)):
            assert form(**kw) != 0 and b"form 1" in err() and b"4096 cells" in err(), kw

        def fwd(hh=h, x=p, n=2, M=3, r=6, cand=p, cidx=p, ws=p, wsb=1 << 40):
            return lib.esahrnet_forward_keypoints_candidates(hh, x, n, 48, 80, M, r, cand, cidx, ws, wsb, None)
        for name in ("hh", "x", "cand", "ws"):
            assert fwd(**{name: None}) != 0 and b"null" in err(), name
        for M in (0, 5, -1):
            assert fwd(M=M) != 0 and b"forward_keypoints_candidates: %d candidates per heat-map unsupported (1..4)" % M in err()
        assert fwd(r=-1) != 0 and b"forward_keypoints_candidates: negative nms_radius -1" in err()
        for name in ("cand", "cidx"):
            assert fwd(**{name: p + 2}) != 0 and b"cand_dev and cidx_dev must be 4-byte aligned" in err(), name
        assert fwd() != 0 and b"commit" in err()                                  # the handle has no weights
        assert fwd(cidx=None) != 0 and b"commit" in err()                         # cidx_dev may be NULL
        q = lib.esahrnet_keypoints_candidates_forward_workspace_bytes
        assert q(h, 2, 48, 80, None) != 0 and b"null" in err()
        assert q(None, 2, 48, 80, C.byref(nb)) != 0 and b"null" in err()
        assert q(h, 0, 48, 80, C.byref(nb)) != 0

        def fr(hh=h, m=1, nframes=1, fmt=0, rule=0, std=0.229, M=3, r=6, cand=p, cidx=p, ws=p, wsb=1 << 40, fidx=None):
            return lib.esahrnet_frames_keypoints_candidates(hh, p, nframes, 1200, 1920, fmt, p, fidx, m, 256, rule, 0.485, std, M, r,
                                                            cand, cidx, p, p, p, ws, wsb, None)
        for name in ("hh", "cand", "ws"):
            assert fr(**{name: None}) != 0 and b"null" in err(), name
        assert fr(m=0) != 0 and fr(m=-1) != 0
        assert fr(rule=3) != 0 and b"rule" in err()
        assert fr(fmt=5) != 0 and b"pixel_format" in err()
        assert fr(std=-1.0) != 0 and b"stdv" in err()
        assert fr(m=2) != 0 and b"frame index" in err()
        for M in (0, 5):
            assert fr(M=M) != 0 and b"frames_keypoints_candidates: %d candidates per heat-map unsupported (1..4)" % M in err()
        assert fr(r=-2) != 0 and b"frames_keypoints_candidates: negative nms_radius -2" in err()
        assert fr(cand=p + 2) != 0 and b"4-byte aligned" in err()
        assert fr() != 0 and b"commit" in err()
        fq = lib.esahrnet_frames_keypoints_candidates_workspace_bytes
        assert fq(h, 1, 256, None) != 0 and b"null" in err()
        assert fq(h, 0, 256, C.byref(nb)) != 0
        assert fq(h3, 1, 256, C.byref(nb)) != 0 and b"1-channel" in err()
    finally:
        lib.esahrnet_destroy(h)
        lib.esahrnet_destroy(h3)


@pytest.mark.parametrize("variant,precision", [(0, "fp32"), (1, "fp32"), (1, "bf16"), (0, "bf16x3"), (0, "bf16")])
def test_workspace_is_the_forwards_plus_the_padded_heat_maps(variant, precision):
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    k = 30 if variant else 11
    h = _handle(lib, L, variant=variant, k=k, precision=precision)
    try:
        for n, hh, ww in ((1, 64, 64), (32, 256, 256), (3, 80, 112), (1, 18, 34)):
            got, fwd = C.c_size_t(), C.c_size_t()
            L.check(lib.esahrnet_keypoints_candidates_forward_workspace_bytes(h, n, hh, ww, C.byref(got)))
            L.check(lib.esahrnet_workspace_bytes(h, n, hh, ww, C.byref(fwd)))
            assert got.value == fwd.value + ((n * k * hh * ww * 4 + 255) & ~255) and fwd.value % 256 == 0
        for m, s in ((1, 256), (32, 256), (3, 90)):
            got, base = C.c_size_t(), C.c_size_t()
            L.check(lib.esahrnet_frames_keypoints_candidates_workspace_bytes(h, m, s, C.byref(got)))
            L.check(lib.esahrnet_keypoints_candidates_forward_workspace_bytes(h, m, s, s, C.byref(base)))
            assert got.value == base.value + ((m * s * s * 4 + 255) & ~255)
    finally:
        lib.esahrnet_destroy(h)


def test_packed_layout_with_candidates():
    from esa_pose_estimation_amd import inference
    for m, k, M in ((1, 11, 1), (5, 11, 3), (3, 30, 4), (7, 11, 2)):
        lay = inference.packed_layout(m, k, candidates=M)
        end = 0
        for name, size, nbytes in (("rates", 8, 8 * m), ("cand", 4, 12 * m * k * M), ("boxes", 4, 16 * m), ("valid", 4, 4 * m),
                                   ("cidx", 4, 4 * m * k * M)):
            assert lay[name] == (end, nbytes) and end % size == 0, name
            end += nbytes
        assert lay["total"] == (0, end) and set(lay) == {"rates", "cand", "boxes", "valid", "cidx", "total"}
        # the existing layouts are what they were
        old = inference.packed_layout(m, k)
        assert old == inference.packed_layout(m, k, candidates=None) and set(old) == {"rates", "kp", "boxes", "valid", "idx", "total"}
        assert [old[n] for n in ("rates", "kp", "boxes", "valid", "idx")] == \
            [(0, 8 * m), (8 * m, 12 * m * k), (8 * m + 12 * m * k, 16 * m), (24 * m + 12 * m * k, 4 * m), (28 * m + 12 * m * k, 4 * m * k)]
        assert inference.packed_layout(m, k, True) == inference.packed_layout(m, k, True, False, None)
    for bad in (0, 5):
        with pytest.raises(ValueError, match="candidates"):
            inference.packed_layout(2, 11, candidates=bad)
    with pytest.raises(ValueError, match="gaussfit"):
        inference.packed_layout(2, 11, True, candidates=2)


def test_python_names_and_what_estimate_poses_refuses():
    import torch
    from esa_pose_estimation_amd import config, hrnet, inference, pipeline, seg_hrnet2
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64)))
    assert pipeline.CANDIDATES_PATHS == ("heatmaps", "fused", "loader")
    with pytest.raises(ValueError, match="candidates_path must be one of"):
        pipeline.estimate_poses(net, None, None, None, None, candidates=2, candidates_path="device")
    for path in ("fused", "loader"):
        with pytest.raises(ValueError, match="belongs to candidates > 1"):
            pipeline.estimate_poses(net, None, None, None, None, candidates_path=path)
        for kw in (dict(device_loader=True), dict(keypoints_only=True), dict(device_select=True), dict(distributed=True),
                   dict(native=False), dict(refine="get_final2")):
            with pytest.raises(ValueError, match="candidates=2 is not available with"):
                pipeline.estimate_poses(net, None, None, None, None, candidates=2, candidates_path=path, **kw)
    with pytest.raises(ValueError, match="candidates=2 is not available with device_loader"):
        pipeline.estimate_poses(net, None, None, None, None, candidates=2, device_loader=True)
    with pytest.raises(RuntimeError, match="no CPU"):                                # the fused path: no eager fall-back
        net.eval().candidates(torch.zeros(1, 1, 32, 32))
    with pytest.raises(RuntimeError, match="GPU only"):
        inference.heatmaps_to_candidates(torch.zeros(1, 3, 32, 40), form=1)
    assert hrnet._Runtime.WS_KINDS["candidates"][1] == "esahrnet_keypoints_candidates_forward_workspace_bytes"
    assert hrnet._Runtime.WS_KINDS["frames_candidates"][1] == "esahrnet_frames_keypoints_candidates_workspace_bytes"
    assert hrnet.HighResolutionNet.OUTPUTS == ("heatmaps", "keypoints", "keypoints+index")


def test_the_one_sweep_kernel_stays_in_registers():
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    assert "keypoints_candidates_onepass.hip" in b.SOURCES
    usage = json.load(open(b.USAGE))
    new = [k for k in usage if "keypoints_candidates_onepass_kernel" in k]
    assert len(new) == 1, new
    u = usage[new[0]]
    print(new[0], u)
    assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0
    assert u["vgprs"] <= 128 and u["waves_per_simd"] >= 4                         # 16 waves per workgroup: four per SIMD
    assert 4096 * 8 <= u["lds"] <= 4096 * 8 + 1024                                # the table of 4096 cells and the reduction's slots
    old = [k for k in usage if k.startswith("keypoints_candidates.hip:") and "keypoints_candidates_kernel" in k]
    assert len(old) == 1 and usage[old[0]]["scratch"] == 0
