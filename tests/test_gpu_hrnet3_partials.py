"""seg_hrnet3 leaves per-tile maxima beside its heat-maps (layout.hip: the heat-map conversion to NCHW, under
esahrnet_forward_partials), in every precision, so heatmaps_to_keypoints(net(x)) finishes over them instead of sweeping the
maps again.  The maps must be the bits esahrnet_forward writes, and the finish must give the bits of the full sweep: ties
keep the first index, NaN counts as the maximum."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = (16, 16, 32, 64)
PRECISIONS = ["fp32", "bf16x3", "bf16"]
SHAPES = [(2, 64, 64), (2, 48, 80), (3, 34, 18)]        # 34 x 18 = 612 pixels: the last tile of a plane is short


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, inference, seg_hrnet3, synth
    from oracle import keypoints_ref
    return dict(lib=_lib.lib(), L=_lib, config=config, inference=inference, seg_hrnet3=seg_hrnet3, synth=synth,
                kref=keypoints_ref)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them; ESAHRNET_NO_PARTIALS: hrnet.py


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _build(env, precision, seed=53):
    net = env["seg_hrnet3"].get_seg_model(env["config"].make_config(widths=WIDTHS), precision=precision)
    sd = env["synth"].make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=seed, gain=0.5)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


def _bits(t):
    return t.contiguous().view(torch.int32)


def _finish_and_sweep(env, heat):
    """(kp, idx) from esahrnet_keypoints_finish over the forward's tile maxima and from esahrnet_keypoints_ex."""
    lib, L = env["lib"], env["L"]
    part, nt, _ = heat._esa_partials
    n, k, hh, ww = heat.shape
    out = []
    for finish in (True, False):
        kp = torch.empty((n, k, 3), dtype=torch.float32, device=heat.device)
        idx = torch.empty((n, k), dtype=torch.int32, device=heat.device)
        if finish:
            L.check(lib.esahrnet_keypoints_finish(heat.data_ptr(), part.data_ptr(), nt, n, k, hh, ww, kp.data_ptr(), idx.data_ptr(),
                                                  _stream()))
        else:
            L.check(lib.esahrnet_keypoints_ex(heat.data_ptr(), n, k, hh, ww, kp.data_ptr(), idx.data_ptr(), _stream()))
        out.append((kp, idx))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hrnet3_reports_tile_maxima(env, precision):
    net, _ = _build(env, precision)
    x = env["synth"].make_crops(1, 1, 64, 64, seed=53).cuda()
    with torch.no_grad():
        net(x)                                            # commits the handle
    h = net._rt._handle_for(net, x.device)
    nt = C.c_int(-1)
    env["L"].check(env["lib"].esahrnet_partial_tiles(h, 64, 64, C.byref(nt)))
    assert nt.value > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hrnet3_partials_equal_the_full_sweep(env, monkeypatch, precision, shape):
    net, _ = _build(env, precision)
    n, hh, ww = shape
    x = env["synth"].make_crops(n, 1, hh, ww, seed=59).cuda()
    inf = env["inference"]
    with torch.no_grad():
        heat = net(x)
        assert getattr(heat, "_esa_partials", None) is not None and heat._esa_partials[1] > 0
        (kp_f, idx_f), (kp_s, idx_s) = _finish_and_sweep(env, heat)
        kp_fast = inf.heatmaps_to_keypoints(heat)
        kp_full = inf.heatmaps_to_keypoints(heat.clone())
        monkeypatch.setenv("ESAHRNET_NO_PARTIALS", "1")        # esahrnet_forward's conversion
        heat_plain = net(x)
    assert getattr(heat_plain, "_esa_partials", None) is None
    assert torch.equal(_bits(heat), _bits(heat_plain))
    assert torch.equal(_bits(kp_f), _bits(kp_s)) and torch.equal(idx_f, idx_s)
    assert torch.equal(kp_fast, kp_full) and torch.equal(kp_fast, kp_f)
    ref = env["kref"].heatmaps_to_keypoints(heat.cpu().numpy())
    assert np.allclose(kp_fast.cpu().numpy(), ref, rtol=0, atol=1e-4)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hrnet3_partials_ties_and_nan(env, precision):
    net, sd = _build(env, precision)
    x = env["synth"].make_crops(3, 1, 48, 80, seed=61)
    x[1, 0, 20:30, 33:40] = float("nan")                  # crop 1: NaN pixels
    x = x.cuda()
    with torch.no_grad():
        heat = net(x)
        (kp_f, idx_f), (kp_s, idx_s) = _finish_and_sweep(env, heat)
    assert torch.isnan(heat[1]).any() and torch.isfinite(heat[0]).all() and torch.isfinite(heat[2]).all()
    assert torch.equal(_bits(kp_f), _bits(kp_s)) and torch.equal(idx_f, idx_s)
    first_nan = torch.isnan(heat[1]).flatten(1).int().argmax(1).int()
    assert torch.equal(idx_f[1], first_nan) and torch.isnan(kp_f[1, :, 2]).all()
    # ties: zero weights in the output layer -> every plane is its constant bias -> first index (0, 0)
    sd0 = {k: v.clone() for k, v in sd.items()}
    sd0["output_layer.0.weight"].zero_()
    net.load_state_dict(sd0)
    with torch.no_grad():
        heat0 = net(x[[0, 2]])
        (kp0, idx0), (kp0_s, idx0_s) = _finish_and_sweep(env, heat0)
    assert bool((heat0 == heat0[:, :, :1, :1]).all())
    assert torch.equal(_bits(kp0), _bits(kp0_s)) and torch.equal(idx0, idx0_s)
    assert bool((idx0 == 0).all()) and bool((kp0[..., :2] == 0).all())
