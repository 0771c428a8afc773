"""seg_hrnet3 with the W48 widths in the fp32-grade and split-bf16 modes, without a GPU: the plan is made at the bench
shapes and every launch is described.  A CBAM that no kernel serves is refused when the plan is made, with the layer and
its channel count."""
import ctypes as C
import os

import pytest

W48 = (48, 96, 192, 384)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


def _probe(widths, precision):
    import torch  # noqa: F401  (first: the library shares torch's HIP runtime)
    from esa_pose_estimation_amd import config, seg_hrnet3
    net = seg_hrnet3.get_seg_model(config.make_config(widths=widths), precision=precision)
    return net, net._rt._probe


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_hrnet3_w48_plan_is_made_and_described(precision):
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    net, h = _probe(W48, precision)
    for n, hh, ww in [(64, 384, 384), (32, 256, 256), (2, 128, 128), (1, 70, 50)]:
        nbytes = C.c_size_t(0)
        L.check(lib.esahrnet_workspace_bytes(h, n, hh, ww, C.byref(nbytes)))
        assert nbytes.value > 0
        kernels = []
        for i in range(lib.esahrnet_launch_count(h)):
            d = L.OpDesc()
            L.check(lib.esahrnet_op_desc_get(h, i, n, hh, ww, C.byref(d)))
            kernels.append(d.kernel.decode())
        assert any(k in ("pool_partial", "cbam_jobs(pool)") for k in kernels)
        assert kernels[-1].endswith("_to_nchw")       # the heat-maps leave in NCHW


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_unservable_cbam_is_refused_by_the_plan(precision):
    """ca_mlp takes at most 512 (padded) channels: a 520-channel branch has no channel-attention kernel."""
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    net, h = _probe((16, 16, 16, 520), precision)
    nbytes = C.c_size_t(0)
    assert lib.esahrnet_workspace_bytes(h, 2, 64, 64, C.byref(nbytes)) != 0
    err = lib.esahrnet_last_error().decode()
    assert "CBAM channel-attention MLP of 'stage4.0.branches.3.0' at 520 channels" in err, err
    # the same widths below the limit: planned
    net, h = _probe((16, 16, 16, 504), precision)
    L.check(lib.esahrnet_workspace_bytes(h, 2, 64, 64, C.byref(nbytes)))
