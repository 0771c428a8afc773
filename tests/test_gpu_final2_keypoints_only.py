"""net(x, output="keypoints", refine="get_final2") runs esahrnet_forward_keypoints_final2 (include/esahrnet.h): kp and idx
bit-identical to esahrnet_forward + esahrnet_keypoints_final2 for every network, precision and output-layer form, at shapes
that are not multiples of any tile, with ties, NaN and peaks at the border, batch-invariant, in a graph, through
DataParallel, and with a workspace that holds no N*K*H*W heat-map where the forward keeps none."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

NETS = {"seg_hrnet": (3, 32, (16, 32, 64, 128)), "seg_hrnet2": (1, 11, (16, 32, 64, 128)), "seg_hrnet3": (1, 30, (16, 16, 32, 64))}
PRECISIONS = ["fp32", "bf16x3", "bf16"]
SHAPES = {0: [(2, 48, 80), (2, 18, 34), (1, 104, 72), (3, 16, 16)], 1: [(2, 48, 80), (3, 34, 18), (1, 104, 72), (2, 64, 64)]}
W48 = (48, 96, 192, 384)
F2V_T = 22                                  # head.hip: the blurring VALU output layer's tiles


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


def _same(a, b):
    """Bit-identical keypoints (NaN rows included: same NaN mask, same bits)."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.contiguous().view(torch.int32),
                                                                      b.contiguous().view(torch.int32))


def _check(env, net, x):
    """The new path against esahrnet_forward + esahrnet_keypoints_final2 (heatmaps_to_keypoints(heat, "get_final2"))."""
    with torch.no_grad():
        kp, idx = net(x, output="keypoints+index", refine="get_final2")
        kp1 = net(x, output="keypoints", refine="get_final2")
        heat = net(x)
        ref, ridx = env["inference"]._keypoints(heat, True, "get_final2")
    torch.cuda.synchronize()
    assert kp.shape == (x.shape[0], net.num_keypoints, 3) and idx.dtype == torch.int32
    assert torch.equal(idx, ridx)
    assert _same(kp, ref) and _same(kp1, ref)
    return heat, kp, idx


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(NETS))
def test_equal_to_forward_plus_keypoints_final2(env, name, precision):
    net, _ = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate(SHAPES[1 if name == "seg_hrnet3" else 0]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=160 + i).cuda()
        _check(env, net, x)


@pytest.mark.parametrize("name", ["seg_hrnet", "seg_hrnet2"])
def test_valu_output_layer_on_split_bf16(env, monkeypatch, name):
    """ESAHRNET_FINAL_VALU=1: the blurring VALU output layer reading split-bf16 tensors."""
    monkeypatch.setenv("ESAHRNET_FINAL_VALU", "1")
    net, _ = _build(env, name, "bf16x3")
    for i, (n, hh, ww) in enumerate(SHAPES[0]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=170 + i).cuda()
        _check(env, net, x)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_seg_hrnet3_w48(env, precision):
    net, _ = _build(env, "seg_hrnet3", precision, widths=W48, seed=7)
    for i, (n, hh, ww) in enumerate([(2, 64, 64), (1, 48, 80)]):
        x = env["synth"].make_crops(n, 1, hh, ww, seed=180 + i).cuda()
        _check(env, net, x)


def test_peaks_on_tile_and_image_borders(env):
    """Peaks within 2 px of the plane's edge (no step taken) and of a 22 x 22 tile's edge (the blur reads the next tile)."""
    near_tile = near_image = 0
    for seed in range(3):
        net, _ = _build(env, "seg_hrnet2", "fp32", seed=80 + seed, gain=1.0)
        for n, hh, ww in [(8, 48, 80), (8, 104, 72), (8, 18, 34)]:
            x = env["synth"].make_crops(n, 1, hh, ww, seed=90 + seed).cuda()
            _, kp, idx = _check(env, net, x)
            py, px = (idx // ww).cpu(), (idx % ww).cpu()
            near_tile += int((((px % F2V_T) < 2) | ((px % F2V_T) >= F2V_T - 2) | ((py % F2V_T) < 2) |
                              ((py % F2V_T) >= F2V_T - 2)).sum())
            border = (px < 2) | (px >= ww - 2) | (py < 2) | (py >= hh - 2)
            near_image += int(border.sum())
            kpc = kp.cpu()
            assert torch.equal(kpc[..., 0][border], px[border].float()) and torch.equal(kpc[..., 1][border], py[border].float())
    print(f"planes with the peak near a tile edge: {near_tile}, near the image edge: {near_image}")
    assert near_tile > 0 and near_image > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(NETS))
def test_ties_and_nan(env, name, precision):
    net, sd = _build(env, name, precision)
    cin = NETS[name][0]
    x = env["synth"].make_crops(3, cin, 48, 80, seed=61)
    x[1, 0, 20:30, 33:40] = float("nan")                  # crop 1: NaN pixels
    x[2, 0, 5:9, 60:66] = float("inf")                    # crop 2: +inf pixels
    x = x.cuda()
    heat, kp, idx = _check(env, net, x)
    assert torch.isnan(heat[1]).any() and torch.isfinite(heat[0]).all()
    # ties: zero output-layer weights -> every plane is its constant bias -> first index (0, 0), no step
    sd0 = {k: v.clone() for k, v in sd.items()}
    sd0["output_layer.0.weight"].zero_()
    net.load_state_dict(sd0)
    heat0, kp0, idx0 = _check(env, net, x[[0, 0]])               # (0 * inf is NaN: the +inf crop has no constant planes)
    assert bool((heat0 == heat0[:, :, :1, :1]).all())
    assert bool((idx0 == 0).all()) and bool((kp0[..., :2] == 0).all())


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_batch_invariance(env, name):
    net, _ = _build(env, name, "fp32")
    x = env["synth"].make_crops(32, 1, 96, 96, seed=5).cuda()
    with torch.no_grad():
        kp, idx = net(x, output="keypoints+index", refine="get_final2")
        for i in range(32):
            kpi, idxi = net(x[i:i + 1], output="keypoints+index", refine="get_final2")
            assert _same(kpi[0], kp[i]) and torch.equal(idxi[0], idx[i]), i


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_graph_capture_and_data_parallel(env, name):
    net, _ = _build(env, name, "fp32")
    x = env["synth"].make_crops(4, 1, 64, 64, seed=2).cuda()
    with torch.no_grad():
        kp0 = net(x, output="keypoints", refine="get_final2").clone()
        ref = env["inference"].heatmaps_to_keypoints(net(x), refine="get_final2")
        assert _same(kp0, ref)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(x, output="keypoints", refine="get_final2")
        torch.cuda.current_stream().wait_stream(s)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            kpg = net(x, output="keypoints", refine="get_final2")
        gph.replay()
        torch.cuda.synchronize()
        assert _same(kpg, kp0)
        dp = torch.nn.DataParallel(net, device_ids=[0])
        assert _same(dp(x, output="keypoints", refine="get_final2"), kp0)
        kp_dp, idx_dp = dp(x, output="keypoints+index", refine="get_final2")
        assert _same(kp_dp, kp0) and idx_dp.dtype == torch.int32


@pytest.mark.parametrize("name,precision", [("seg_hrnet2", "fp32"), ("seg_hrnet3", "fp32"), ("seg_hrnet3", "bf16x3"),
                                            ("seg_hrnet3", "bf16")])
def test_cached_workspace_has_no_heatmap_term(env, name, precision):
    """The workspace net(x, output="keypoints", refine="get_final2") caches obeys the bound of the C query: the get_final
    keypoints-only workspace + 12 B x planes x tiles + 4 KB."""
    net, _ = _build(env, name, precision)
    n, hh, ww = 8, 128, 128
    x = env["synth"].make_crops(n, 1, hh, ww, seed=3).cuda()
    rt = net._rt
    rt.ws_cache("final2").clear()
    with torch.no_grad():
        net(x, output="keypoints", refine="get_final2")
        net(x, output="keypoints")
    torch.cuda.synchronize()
    kw = max(t.numel() for t in rt.ws_cache("keypoints").values())
    planes = n * net.num_keypoints
    bound = kw + 12 * planes * (-(-hh // F2V_T)) * (-(-ww // F2V_T)) + 4096
    f2 = [t.numel() for t in rt.ws_cache("final2").values()]
    assert f2 and max(f2) <= bound, (f2, kw, bound)
    assert max(f2) - kw < planes * hh * ww * 4 // 8           # far from the N*K*H*W*4 bytes of the heat-maps


def test_entry_errors(env):
    lib, L = env["lib"], env["L"]
    net, _ = _build(env, "seg_hrnet2", "fp32")
    x = env["synth"].make_crops(2, 1, 48, 80, seed=4).cuda()
    with torch.no_grad():
        ref = net(x, output="keypoints", refine="get_final2")
    h = net._rt._handle_for(net, x.device)
    need = C.c_size_t()
    L.check(lib.esahrnet_keypoints_final2_forward_workspace_bytes(h, 2, 48, 80, C.byref(need)))
    ws = torch.empty(need.value + 512, dtype=torch.uint8, device="cuda")
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    kp = torch.empty((2, 11, 3), device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = lib.esahrnet_forward_keypoints_final2
    assert f(h, x.data_ptr(), 2, 48, 80, kp.data_ptr(), None, wp, need.value - 256, stream) != 0
    assert b"too small" in lib.esahrnet_last_error()
    assert f(h, x.data_ptr(), 2, 48, 80, kp.data_ptr(), None, wp + 8, need.value, stream) != 0
    assert b"aligned" in lib.esahrnet_last_error()
    assert f(h, x.data_ptr(), 0, 48, 80, kp.data_ptr(), None, wp, need.value, stream) != 0
    assert b"batch" in lib.esahrnet_last_error()
    assert f(h, None, 2, 48, 80, kp.data_ptr(), None, wp, need.value, stream) != 0
    assert b"null" in lib.esahrnet_last_error()
    assert f(h, x.data_ptr(), 2, 48, 80, kp.data_ptr(), None, None, need.value, stream) != 0
    assert b"null" in lib.esahrnet_last_error()
    L.check(f(h, x.data_ptr(), 2, 48, 80, kp.data_ptr(), None, wp, need.value, stream))
    torch.cuda.synchronize()
    assert _same(kp, ref)
