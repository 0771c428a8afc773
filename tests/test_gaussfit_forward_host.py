"""CPU: the Gaussian-fit decoder fused into the forward and behind the device loader (include/esahrnet.h
esahrnet_forward_keypoints_gaussfit, esahrnet_frames_keypoints_gaussfit and their workspace queries) is declared, exported and
bound with the ABI number unchanged; argument errors answer before anything touches a GPU; the workspace is that of
esahrnet_forward_keypoints (no n * K * H * W term where the forward keeps none); the Python names know the decoder; the new
kernels use neither scratch memory nor spills and gaussfit_kernel is compiled to what it was."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"esahrnet_keypoints_gaussfit_forward_workspace_bytes": 5, "esahrnet_forward_keypoints_gaussfit": 13,
           "esahrnet_frames_keypoints_gaussfit_workspace_bytes": 4, "esahrnet_frames_keypoints_gaussfit": 24}


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
        def fwd(hh=h, x=p, n=2, kp=p, idx=p, fit=p, status=p, hess=p, ws=p, wsb=1 << 40):
            return lib.esahrnet_forward_keypoints_gaussfit(hh, x, n, 48, 80, kp, idx, fit, status, hess, ws, wsb, None)
        for name in ("hh", "x", "kp", "status", "ws"):
            assert fwd(**{name: None}) != 0 and b"null" in err(), name
        for name in ("kp", "idx", "status"):
            assert fwd(**{name: p + 2}) != 0 and b"4-byte aligned" in err(), name
        for name in ("fit", "hess"):
            assert fwd(**{name: p + 4}) != 0 and b"8-byte aligned" in err(), name
        assert fwd() != 0 and b"commit" in err()                                  # the handle has no weights
        assert fwd(n=0) != 0
        q = lib.esahrnet_keypoints_gaussfit_forward_workspace_bytes
        assert q(h, 2, 48, 80, None) != 0 and b"null" in err()
        assert q(None, 2, 48, 80, C.byref(nb)) != 0 and b"null" in err()
        assert q(h, 0, 48, 80, C.byref(nb)) != 0

        def fr(hh=h, m=1, nframes=1, fmt=0, rule=0, std=0.229, kp=p, status=p, fit=p, ws=p, wsb=1 << 40, fidx=None):
            return lib.esahrnet_frames_keypoints_gaussfit(hh, p, nframes, 1200, 1920, fmt, p, fidx, m, 256, rule, 0.485, std, kp,
                                                          None, fit, status, None, p, p, p, ws, wsb, None)
        for name in ("hh", "kp", "status", "ws"):
            assert fr(**{name: None}) != 0 and b"null" in err(), name
        assert fr(m=0) != 0 and fr(m=-1) != 0
        assert fr(rule=3) != 0 and b"rule" in err()
        assert fr(fmt=5) != 0 and b"pixel_format" in err()
        assert fr(std=-1.0) != 0 and b"stdv" in err()
        assert fr(m=2) != 0 and b"frame index" in err()
        assert fr(fit=p + 4) != 0 and b"commit" in err()                          # the same order as esahrnet_frames_keypoints
        assert fr() != 0 and b"commit" in err()
        fq = lib.esahrnet_frames_keypoints_gaussfit_workspace_bytes
        assert fq(h, 1, 256, None) != 0 and b"null" in err()
        assert fq(h, 0, 256, C.byref(nb)) != 0
        assert fq(h3, 1, 256, C.byref(nb)) != 0 and b"1-channel" in err()
        # the existing entries still refuse the third decoder: it has symbols of its own
        assert lib.esahrnet_frames_keypoints_workspace_bytes(h, 1, 256, 2, C.byref(nb)) != 0 and b"decoder" in err()
    finally:
        lib.esahrnet_destroy(h)
        lib.esahrnet_destroy(h3)


@pytest.mark.parametrize("variant,precision", [(0, "fp32"), (1, "fp32"), (1, "bf16x3"), (1, "bf16"), (0, "bf16x3")])
def test_workspace_is_that_of_forward_keypoints(variant, precision):
    """The query equals esahrnet_keypoints_workspace_bytes; for the VALU output layer and for seg_hrnet3 that is the forward's
    workspace plus 8 bytes per plane and tile, no n * K * H * W term.  The loader adds its 256-byte-aligned crop tensor."""
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    k = 30 if variant else 11
    h = _handle(lib, L, variant=variant, k=k, precision=precision)
    try:
        for n, hh, ww in ((1, 64, 64), (32, 256, 256), (3, 80, 112)):
            got, base, fwd = C.c_size_t(), C.c_size_t(), C.c_size_t()
            L.check(lib.esahrnet_keypoints_gaussfit_forward_workspace_bytes(h, n, hh, ww, C.byref(got)))
            L.check(lib.esahrnet_keypoints_workspace_bytes(h, n, hh, ww, C.byref(base)))
            L.check(lib.esahrnet_workspace_bytes(h, n, hh, ww, C.byref(fwd)))
            assert got.value == base.value
            if precision == "fp32" or variant == 1:
                assert got.value - fwd.value < n * k * hh * ww * 4 // 8, (got.value, fwd.value)
        for m, s in ((1, 256), (32, 256), (3, 90)):
            got, base = C.c_size_t(), C.c_size_t()
            L.check(lib.esahrnet_frames_keypoints_gaussfit_workspace_bytes(h, m, s, C.byref(got)))
            L.check(lib.esahrnet_keypoints_gaussfit_forward_workspace_bytes(h, m, s, s, C.byref(base)))
            assert got.value == base.value + ((m * s * s * 4 + 255) & ~255)
    finally:
        lib.esahrnet_destroy(h)


def test_python_names_know_the_decoder():
    from esa_pose_estimation_amd import config, inference, pipeline, seg_hrnet2
    assert "gaussfit" in inference.REFINES and inference.check_refine("gaussfit") == "gaussfit"
    assert inference.check_weights("hessian", "gaussfit") == 1 == inference.check_weights("hessian")
    assert inference.check_weights("peak", "gaussfit") == 0
    with pytest.raises(ValueError, match="get_final2"):
        inference.check_weights("hessian", "get_final")
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64)))
    with pytest.raises(ValueError, match="keypoints"):
        net(torch.zeros(1, 1, 32, 32), output="heatmaps", refine="gaussfit")
    with pytest.raises(RuntimeError, match="no CPU"):                                # the fused path: no eager fall-back
        net(torch.zeros(1, 1, 32, 32), output="keypoints", refine="gaussfit")
    with pytest.raises(RuntimeError, match="GPU only"):
        inference.heatmaps_to_keypoints(torch.zeros(1, 3, 32, 40), refine="gaussfit")
    with pytest.raises(ValueError, match="device_select"):
        pipeline.estimate_poses(net, None, None, None, None, refine="gaussfit", weights="hessian")
    # the packed record of the loader: the f64 parts first, every part aligned to its element, nothing overlaps
    for m, k in ((1, 11), (5, 11), (3, 30)):
        lay = inference.packed_layout(m, k, True)
        end = 0
        for name, size in (("rates", 8), ("fit", 8), ("hess", 8), ("kp", 4), ("boxes", 4), ("valid", 4), ("idx", 4), ("status", 4)):
            off, nbytes = lay[name]
            assert off == end and off % size == 0 and nbytes > 0, name
            end = off + nbytes
        assert lay["total"] == (0, end)
        old = inference.packed_layout(m, k)
        assert [old[n] for n in ("rates", "kp", "boxes", "valid", "idx")] == \
            [(0, 8 * m), (8 * m, 12 * m * k), (8 * m + 12 * m * k, 16 * m), (24 * m + 12 * m * k, 4 * m), (28 * m + 12 * m * k, 4 * m * k)]


def test_new_kernels_stay_in_registers_and_gaussfit_kernel_is_what_it_was():
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    assert "gaussfit.h" in b.HEADERS                                              # a change of the solver rebuilds the library
    usage = json.load(open(b.USAGE))
    new = [k for k in usage if "final_gf_finish_kernel" in k or "gf_nhwc_fit_kernel" in k or "mark_invalid_gaussfit_kernel" in k]
    assert len(new) == 4, new                                                     # the NHWC fit: f32 and split-bf16
    for k in new:
        u = usage[k]
        print(k, u)
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, k
    fin = usage[[k for k in new if "final_gf_finish_kernel" in k][0]]
    assert k and fin["lds"] <= 8 * 15 * 15 * 4 + 13 * 13 * 4 and fin["waves_per_simd"] >= 2       # one 8-channel chunk + the window
    for k in new:
        if "gf_nhwc_fit_kernel" in k:
            assert usage[k]["lds"] == 0 and usage[k]["waves_per_simd"] >= 2
    # gaussfit_kernel, moved into csrc/gaussfit.h: the figures of the build before the move
    hits = [k for k in usage if k.startswith("keypoints_gaussfit.hip:") and "gaussfit_kernel" in k]
    assert len(hits) == 1, hits
    assert usage[hits[0]] == dict(agprs=0, lds=0, scratch=0, sgpr_spill=0, vgpr_spill=0, vgprs=226, waves_per_simd=2), usage[hits[0]]
