"""net(x, output="keypoints") (include/esahrnet.h esahrnet_forward_keypoints): keypoints straight from the crops, no heat-map
in caller memory, bit-identical to heatmaps_to_keypoints(net(x)) — for every network, precision and output-layer kernel,
ties and NaNs included, at odd shapes, in a graph, through DataParallel — and within the oracle's tolerance at full size."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NETS = {"seg_hrnet": (3, 32, (16, 32, 64, 128)), "seg_hrnet2": (1, 11, (16, 32, 64, 128)), "seg_hrnet3": (1, 30, (16, 16, 32, 64))}
PRECISIONS = ["fp32", "bf16x3", "bf16"]
SHAPES = {0: [(2, 48, 80), (2, 18, 34), (1, 104, 72), (1, 128, 160)],
          1: [(2, 64, 64), (2, 48, 80), (3, 34, 18)]}
FTW = 32                                    # head.hip: VALU output tile, 32 columns x 8 * RPT rows


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, inference, seg_hrnet, seg_hrnet2, seg_hrnet3, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, inference=inference, synth=synth,
                seg_hrnet=seg_hrnet, seg_hrnet2=seg_hrnet2, seg_hrnet3=seg_hrnet3)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


def _build(env, name, precision="fp32", widths=None, seed=53, gain=0.5):
    cin, k, w = NETS[name]
    net = env[name].get_seg_model(env["config"].make_config(widths=widths or w), precision=precision)
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=seed, gain=gain)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Bit-identical keypoints (NaN rows included: same NaN mask, same bits)."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(_bits(a), _bits(b))


def _heatmap_path(env, net, x):
    heat = net(x)
    kp, idx = env["inference"]._keypoints(heat, True)
    return heat, kp, idx


def _check(env, net, x):
    with torch.no_grad():
        kp, idx = net(x, output="keypoints+index")
        kp1 = net(x, output="keypoints")
        kp2 = net.keypoints(x)
        heat, kp_h, idx_h = _heatmap_path(env, net, x)
    torch.cuda.synchronize()
    assert kp.shape == (x.shape[0], net.num_keypoints, 3) and idx.dtype == torch.int32
    assert _same(kp, kp_h) and torch.equal(idx, idx_h)
    assert _same(kp1, kp_h) and _same(kp2, kp_h)
    return heat, kp, idx


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(NETS))
def test_keypoints_equal_the_heatmap_path(env, name, precision):
    net, _ = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate(SHAPES[1 if name == "seg_hrnet3" else 0]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=60 + i).cuda()
        _check(env, net, x)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["seg_hrnet", "seg_hrnet2"])
def test_valu_output_layer_in_every_format(env, monkeypatch, name, precision):
    """ESAHRNET_FINAL_VALU=1: the VALU output layer (point re-evaluation in the finish) on split-bf16 and bf16 tensors."""
    monkeypatch.setenv("ESAHRNET_FINAL_VALU", "1")
    net, _ = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate(SHAPES[0]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=70 + i).cuda()
        _check(env, net, x)


def test_peaks_on_tile_and_image_borders(env):
    """The finish of the VALU output layer evaluates the refine's neighbours itself: peaks within 2 px of an output-tile
    edge (their neighbours lie in the next tile) and of the image edge (no refinement) must both occur, and agree."""
    near_tile = near_image = 0
    for seed in range(3):
        net, _ = _build(env, "seg_hrnet2", "fp32", seed=80 + seed, gain=1.0)
        for n, hh, ww in [(8, 48, 80), (8, 104, 72)]:
            x = env["synth"].make_crops(n, 1, hh, ww, seed=90 + seed).cuda()
            _, kp, idx = _check(env, net, x)
            py, px = (idx // ww).cpu().numpy(), (idx % ww).cpu().numpy()
            fth = 16                            # K 11, cin 1: two rows per thread, 32 x 16 tiles
            near_tile += int((((px % FTW) < 2) | ((px % FTW) >= FTW - 2) | ((py % fth) < 2) | ((py % fth) >= fth - 2)).sum())
            near_image += int(((px < 2) | (px >= ww - 2) | (py < 2) | (py >= hh - 2)).sum())
    print(f"planes with the peak near a tile edge: {near_tile}, near the image edge: {near_image}")
    assert near_tile > 0 and near_image > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(NETS))
def test_ties_and_nan(env, name, precision):
    net, sd = _build(env, name, precision)
    cin = NETS[name][0]
    x = env["synth"].make_crops(3, cin, 48, 80, seed=61)
    x[1, 0, 20:30, 33:40] = float("nan")                  # crop 1: NaN pixels
    x = x.cuda()
    heat, kp, idx = _check(env, net, x)
    assert torch.isnan(heat[1]).any() and torch.isfinite(heat[0]).all()
    first_nan = torch.isnan(heat[1]).flatten(1).int().argmax(1).int()
    nanplanes = torch.isnan(heat[1]).flatten(1).any(1)
    assert torch.equal(idx[1][nanplanes], first_nan[nanplanes]) and torch.isnan(kp[1, nanplanes, 2]).all()
    # ties: zero output-layer weights -> every plane is its constant bias -> first index (0, 0)
    sd0 = {k: v.clone() for k, v in sd.items()}
    sd0["output_layer.0.weight"].zero_()
    net.load_state_dict(sd0)
    heat0, kp0, idx0 = _check(env, net, x[[0, 2]])
    assert bool((heat0 == heat0[:, :, :1, :1]).all())
    assert bool((idx0 == 0).all()) and bool((kp0[..., :2] == 0).all())


def _golden(golden_dir, tag):
    return np.load(os.path.join(golden_dir, tag + ".npz"), allow_pickle=False)


@pytest.mark.parametrize("name,tag", [("seg_hrnet2", "w32_hrnet2_256"), ("seg_hrnet3", "w32_hrnet3_128")])
def test_full_size_batch32(env, golden_dir, name, tag):
    """W32 256^2 batch 32 fp32: bit-identical to the heat-map path, every crop's keypoints independent of its batch, and the
    golden crops' arg-max where the reference put it."""
    g = _golden(golden_dir, tag)
    net, _ = _build(env, name, "fp32", widths=tuple(int(v) for v in g["widths"]), seed=int(g["seed"]))
    gn, ghw = int(g["n"]), int(g["hw"])
    synth = env["synth"]
    with torch.no_grad():
        xg = synth.make_crops(gn, 1, ghw, ghw, seed=int(g["seed"])).cuda()
        _, kpg, idxg = _check(env, net, xg)
        assert np.array_equal(idxg.cpu().numpy(), g["plane_argmax"])
        x = torch.cat([synth.make_crops(1, 1, 256, 256, seed=0), synth.make_crops(31, 1, 256, 256, seed=123)]).cuda()
        _, kp, idx = _check(env, net, x)
        for i in (0, 7, 31):
            kpi, idxi = net(x[i:i + 1], output="keypoints+index")
            assert _same(kpi[0], kp[i]) and torch.equal(idxi[0], idx[i]), i
    assert bool(torch.isfinite(kp).all())


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_graph_capture_replays_and_weight_edits_are_seen(env, name):
    net, _ = _build(env, name, "fp32")
    x = env["synth"].make_crops(4, 1, 64, 64, seed=2).cuda()
    with torch.no_grad():
        kp0 = net(x, output="keypoints").clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(x, output="keypoints")
        torch.cuda.current_stream().wait_stream(s)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            kpg = net(x, output="keypoints")
        gph.replay()
        torch.cuda.synchronize()
        assert _same(kpg, kp0)
        dict(net.named_parameters())["output_layer.0.weight"].mul_(0.5)
        kp1 = net(x, output="keypoints")
        ref1 = env["inference"].heatmaps_to_keypoints(net(x))
        torch.cuda.synchronize()
        assert not torch.equal(kp1, kp0) and _same(kp1, ref1)


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_no_heatmap_memory(env, name):
    """After a warm-up, a keypoints-only call allocates (peak) less than 1 % of the N*K*H*W floats it does not write."""
    net, _ = _build(env, name, "fp32")
    n, hh, ww = 8, 128, 128
    x = env["synth"].make_crops(n, 1, hh, ww, seed=5).cuda()
    with torch.no_grad():
        net(x, output="keypoints")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        kp = net(x, output="keypoints")
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    heat_bytes = n * net.num_keypoints * hh * ww * 4
    print(f"{name}: peak rise {rise} B, heat-maps {heat_bytes} B")
    assert rise < 0.01 * heat_bytes and kp.shape == (n, net.num_keypoints, 3)


def test_errors_and_data_parallel(env):
    net, _ = _build(env, "seg_hrnet2", "fp32")
    lib, L = env["lib"], env["L"]
    x = env["synth"].make_crops(2, 1, 64, 64, seed=3).cuda()
    with torch.no_grad():
        ref = net(x, output="keypoints")
        dp = torch.nn.DataParallel(net, device_ids=[0])
        assert _same(dp(x, output="keypoints"), ref)
        kp_dp, idx_dp = dp(x, output="keypoints+index")
        assert _same(kp_dp, ref)
    with pytest.raises(ValueError):
        net(x, output="nothing")
    h = net._rt._handle_for(net, x.device)
    need = C.c_size_t()
    L.check(lib.esahrnet_keypoints_workspace_bytes(h, 2, 64, 64, C.byref(need)))
    ws = torch.empty(need.value + 512, dtype=torch.uint8, device=x.device)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    kp = torch.empty((2, 11, 3), dtype=torch.float32, device=x.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.esahrnet_forward_keypoints(h, x.data_ptr(), 2, 64, 64, kp.data_ptr(), None, wp, need.value - 256, stream) != 0
    assert b"too small" in lib.esahrnet_last_error()
    assert lib.esahrnet_forward_keypoints(h, x.data_ptr(), 2, 64, 64, kp.data_ptr(), None, wp + 4, need.value, stream) != 0
    assert b"aligned" in lib.esahrnet_last_error()
    L.check(lib.esahrnet_forward_keypoints(h, x.data_ptr(), 2, 64, 64, kp.data_ptr(), None, wp, need.value, stream))
    torch.cuda.synchronize()
    assert _same(kp, ref)
    # a handle that was never committed
    h2 = C.c_void_p()
    L.check(lib.esahrnet_create(C.byref(net._cfg_struct), 0, C.byref(h2)))
    try:
        assert lib.esahrnet_forward_keypoints(h2, x.data_ptr(), 2, 64, 64, kp.data_ptr(), None, wp, need.value, stream) != 0
        assert b"commit" in lib.esahrnet_last_error()
    finally:
        lib.esahrnet_destroy(h2)
