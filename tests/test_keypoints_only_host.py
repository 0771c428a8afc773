"""CPU: the keypoints-only forward (include/esahrnet.h esahrnet_forward_keypoints) is declared, bound and exported, its
workspace query answers without a GPU, its argument checks answer before anything touches a device, and its kernels keep
their registers (build/resource_usage.json)."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esahrnet_keypoints_workspace_bytes", "esahrnet_forward_keypoints")


def test_header_declares_the_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esahrnet.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    import torch  # noqa: F401
    from esa_pose_estimation_amd import _lib as L
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == L.ABI_VERSION
    assert L.lib().esahrnet_abi_version() == L.ABI_VERSION


def test_lib_binds_and_exports_the_entries():
    import torch  # noqa: F401
    from esa_pose_estimation_amd import _lib as L
    assert set(ENTRIES) <= set(L.exported_symbols())
    lib = L.lib()
    for name in ENTRIES:
        assert getattr(lib, name).argtypes is not None, name
    raw = C.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name


def _handle(L, variant, precision, cin, k, widths=(16, 32, 64, 128)):
    from esa_pose_estimation_amd import config, hrnet
    cfg = hrnet._cfg_struct(config.make_config(widths=widths), cin, k, variant, precision)
    h = C.c_void_p()
    L.check(L.lib().esahrnet_create(C.byref(cfg), 0, C.byref(h)))
    return h


@pytest.mark.parametrize("variant,precision,cin,k", [(0, "fp32", 1, 11), (0, "bf16x3", 3, 32), (0, "bf16", 1, 11),
                                                     (1, "fp32", 1, 30), (1, "bf16", 1, 30)])
def test_workspace_covers_the_forward_and_the_maxima(monkeypatch, variant, precision, cin, k):
    for e in [e for e in os.environ if e.startswith("ESAHRNET_")]:
        monkeypatch.delenv(e)
    import torch  # noqa: F401
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    h = _handle(L, variant, precision, cin, k)
    try:
        for n, hh, ww in [(2, 48, 80), (3, 34, 18), (32, 256, 256)]:
            fw, kw = C.c_size_t(), C.c_size_t()
            L.check(lib.esahrnet_workspace_bytes(h, n, hh, ww, C.byref(fw)))
            L.check(lib.esahrnet_keypoints_workspace_bytes(h, n, hh, ww, C.byref(kw)))
            # at least the per-tile maxima (8 bytes per plane and tile) behind the forward's own workspace
            assert kw.value >= fw.value + n * k * 8, (n, hh, ww, fw.value, kw.value)
            mfma = variant == 0 and precision != "fp32"
            if mfma:                            # the matrix-core output layer writes its heat-maps into the workspace
                assert kw.value >= fw.value + n * k * hh * ww * 4
            else:                               # no heat-map of N * K * H * W floats anywhere
                assert kw.value - fw.value < n * k * hh * ww * 4 // 8
    finally:
        lib.esahrnet_destroy(h)


def test_errors_before_commit_and_on_null_arguments():
    import torch  # noqa: F401
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    h = _handle(L, 0, "fp32", 1, 11)
    buf = (C.c_char * 512)()
    try:
        p = C.cast(buf, C.c_void_p)
        assert lib.esahrnet_forward_keypoints(h, p, 1, 64, 64, p, None, p, 512, None) != 0
        assert b"commit" in lib.esahrnet_last_error()
        assert lib.esahrnet_forward_keypoints(h, p, 1, 64, 64, None, None, p, 512, None) != 0
        assert b"null" in lib.esahrnet_last_error()
        assert lib.esahrnet_keypoints_workspace_bytes(h, 1, 64, 64, None) != 0
        assert b"null" in lib.esahrnet_last_error()
    finally:
        lib.esahrnet_destroy(h)


NEW_KERNELS = {
    # no scratch, no spills of any kind
    "strict": ("final_kernelILi11ELi2ELb1E", "final_kernelILi11ELi1ELb1E", "final_kernelILi16ELi1ELb1E", "final_kp_finish_kernel",
               "to_nchw_part_kernelILb0ELb0E", "to_nchw_part_kernelILb1ELb0E", "keypoints_finish_nhwc_kernel"),
    # built from final_kernel<16, 2> / <32, *> whose heat-map instances already keep SGPRs in VGPR lanes: no scratch, no
    # VGPR spills
    "no_scratch": ("final_kernelILi16ELi2ELb1E", "final_kernelILi32ELi1ELb1E", "final_kernelILi32ELi2ELb1E"),
}


def test_new_kernels_keep_their_registers():
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    usage = json.load(open(b.USAGE))
    for kind, names in NEW_KERNELS.items():
        for name in names:
            hits = [k for k in usage if name in k]
            assert hits, name
            for k in hits:
                u = usage[k]
                assert u["scratch"] == 0 and u["vgpr_spill"] == 0, (k, u)
                if kind == "strict":
                    assert u["sgpr_spill"] == 0, (k, u)
