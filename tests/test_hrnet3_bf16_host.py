"""seg_hrnet3 in the single-pass bf16 mode (esahrnet_cfg.precision = 1), without a GPU: the net constructs, the plan
builds for the widths, stem widths and input channel counts the mode serves, and esahrnet_op_desc_get names every launch
(bench.py's roofline leg reads these descriptions)."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_op_descs  # noqa: E402

W32, W48 = make_op_descs.W32, make_op_descs.W48
SPLIT_OR_F32_ONLY = ("stem_fused", "stem_x6_kernel", "head_gather", "conv_x6", "conv_mfma")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


@pytest.mark.parametrize("widths", [W32, W48], ids=["w32", "w48"])
def test_seg_hrnet3_bf16_constructs(widths):
    import torch  # noqa: F401  (first: the library shares torch's HIP runtime)
    from esa_pose_estimation_amd import config, seg_hrnet3
    net = seg_hrnet3.get_seg_model(config.make_config(widths=widths), precision="bf16")
    assert net._cfg_struct.precision == 1 and net._cfg_struct.variant == 1
    assert net.num_keypoints == 30


@pytest.mark.parametrize("widths", [W32, W48], ids=["w32", "w48"])
def test_seg_hrnet3_bf16_describes_every_launch(widths):
    descs = make_op_descs.op_descs("seg_hrnet3", "bf16", widths)
    assert list(descs) == [f"{n},{h},{w}" for n, h, w in make_op_descs.SHAPES]
    for shape, rows in descs.items():
        kernels = [r[1] for r in rows]
        for rc, kernel, label, flops, nbytes in rows:
            assert rc == 0, (shape, label)
            if kernel:
                assert nbytes > 0, (shape, kernel, label)
            else:                               # evaluated by another launch: the label says which
                assert "inside" in label or "merged" in label or "multi-head" in label, (shape, label)
            assert not kernel.startswith(SPLIT_OR_F32_ONLY), (shape, kernel)
        convs3 = [r for r in rows if r[1].startswith("conv_s2c32")]
        assert convs3 and all(r[1].endswith(", true>") for r in convs3), shape     # the BF instantiations
        assert kernels.count("conv_s2c32_f32out_kernel<1, 8, 4, true>") == 1       # output_layer: f32 heat-maps
        out = [r for r in rows if r[1] == "conv_s2c32_f32out_kernel<1, 8, 4, true>"][0]
        assert out[2] == "output_layer.0" and out[3] > 0
        assert kernels[-1] == "f32_to_nchw"
        for name in ("stem_kernel", "stem_kernel(raw)", "last_layer.0", "last_layer.3"):
            assert name in kernels or any(r[2] == name for r in rows), (shape, name)
        assert any(k.startswith(("cbam_spatial", "cbam_jobs", "cbam_apply")) for k in kernels)


def _create(lib, L, stem_width, cin, widths=W32):
    from esa_pose_estimation_amd import config, hrnet
    s = hrnet._cfg_struct(config.make_config(widths=widths), cin, 30, 1, "bf16")
    s.stem_width = stem_width
    h = C.c_void_p()
    rc = lib.esahrnet_create(C.byref(s), 0, C.byref(h))
    return rc, h


@pytest.mark.parametrize("stem_width, cin", [(32, 1), (64, 3), (16, 4), (48, 2)])
def test_seg_hrnet3_bf16_plan_builds_for_stem_width_and_cin(stem_width, cin):
    import torch  # noqa: F401
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    rc, h = _create(lib, L, stem_width, cin)
    assert rc == 0, lib.esahrnet_last_error().decode()
    try:
        descs = {}
        for i in range(lib.esahrnet_conv_count(h)):
            d = L.ConvDesc()
            L.check(lib.esahrnet_conv_desc_get(h, i, C.byref(d)))
            descs[d.name.decode()] = (d.cin, d.cout)
        assert descs["conv1"] == (cin, stem_width) and descs["output_layer.0"] == (30 + stem_width, 30)
        for n, hh, ww in [(2, 64, 80), (1, 256, 256)]:
            for i in range(lib.esahrnet_launch_count(h)):
                d = L.OpDesc()
                assert lib.esahrnet_op_desc_get(h, i, n, hh, ww, C.byref(d)) == 0, lib.esahrnet_last_error().decode()
                assert not d.kernel.decode().startswith(SPLIT_OR_F32_ONLY)
    finally:
        lib.esahrnet_destroy(h)


def test_abi_version_6():
    import torch  # noqa: F401
    from esa_pose_estimation_amd import _lib as L
    assert L.ABI_VERSION == 6
    assert L.lib().esahrnet_abi_version() == L.ABI_VERSION
