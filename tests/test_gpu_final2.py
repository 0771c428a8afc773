"""refine="get_final2" on the GPU (include/esahrnet.h esahrnet_keypoints_final2, csrc/keypoints_final2.hip): the kernel equals
the host restatement (tests/final2_ref.py) to one f32 ulp with the same step / no-step decisions, its arg-max and peak are
those of esahrnet_keypoints_ex bit for bit, a crop decodes to the same bits at any batch size, the forward's keypoint outputs
equal heatmaps_to_keypoints(net(x), refine="get_final2") bit for bit (eagerly, in a graph, through DataParallel), and
inference.get_final2 matches the reference's own outputs (tests/golden/final2_*.npz)."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import final2_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

NETS = {"seg_hrnet": (3, 32, (16, 32, 64, 128)), "seg_hrnet2": (1, 11, (16, 32, 64, 128)), "seg_hrnet3": (1, 30, (16, 16, 32, 64))}
REF_TOL = 1e-3          # px, against the reference's own outputs (see test_final2_host.py)


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
        monkeypatch.delenv(k)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(_bits(a), _bits(b))


def _planes(rng, k, h, w):
    """k planes of h x w: Gaussians (isotropic and rotated), noise, and the adversarial cases, in turn."""
    out = np.empty((k, h, w), np.float32)
    for j in range(k):
        kind = j % 12
        cx, cy = rng.uniform(0, w - 1), rng.uniform(0, h - 1)
        if kind in (0, 1):
            p = F.gaussian_planes(h, w, [(cx, cy)], rng.uniform(1.5, 3.0), rng.uniform(1.0, 4.0), rng.uniform(0, np.pi))[0]
        elif kind == 2:
            p = rng.standard_normal((h, w)).astype(np.float32)
        elif kind == 3:
            p = F.gaussian_planes(h, w, [(cx, cy)], 2.0)[0] + rng.uniform(0, 0.2, (h, w)).astype(np.float32)
        elif kind == 4:                                     # NaN
            p = F.gaussian_planes(h, w, [(cx, cy)], 2.0)[0]
            p[rng.integers(h), rng.integers(w)] = np.nan
        elif kind == 5:                                     # +Inf
            p = F.gaussian_planes(h, w, [(cx, cy)], 2.0)[0]
            p[rng.integers(h), rng.integers(w)] = np.inf
        elif kind == 6:                                     # -Inf somewhere, a finite peak elsewhere
            p = F.gaussian_planes(h, w, [(cx, cy)], 2.0)[0]
            p[rng.integers(h), rng.integers(w)] = -np.inf
        elif kind == 7:                                     # ties: two equal maxima
            p = rng.uniform(0, 0.5, (h, w)).astype(np.float32)
            p[h // 2, w // 3] = p[h // 3, w // 2] = 1.0
        elif kind == 8:                                     # all negative
            p = F.gaussian_planes(h, w, [(cx, cy)], 2.5)[0] - 3.0
        elif kind == 9:                                     # maximum exactly 0 (blurred maximum can be 0 too)
            p = -rng.uniform(0.1, 1, (h, w)).astype(np.float32)
            p[h // 2, w // 2] = 0.0
        elif kind == 10:                                    # all zero
            p = np.zeros((h, w), np.float32)
        else:                                               # peak on the refine guard / the border
            p = F.gaussian_planes(h, w, [(rng.choice([1.0, 2.0, w - 3.0, w - 2.0]), cy)], 2.0)[0]
        out[j] = p
    return out


@pytest.mark.parametrize("k,h,w", [(1, 64, 64), (11, 48, 80), (30, 16, 16), (32, 70, 40), (11, 33, 65), (12, 100, 130),
                                   (2, 256, 256)])
def test_kernel_equals_the_restatement(env, k, h, w):
    rng = np.random.default_rng(k * 1000 + h + w)
    hm = _planes(rng, 2 * k, h, w).reshape(2, k, h, w)
    t = torch.from_numpy(hm).cuda()
    kp, idx = env["inference"]._keypoints(t, True, "get_final2")
    kp0, idx0 = env["inference"]._keypoints(t, True)                       # esahrnet_keypoints_ex
    torch.cuda.synchronize()
    assert torch.equal(idx, idx0)
    assert _same(kp[..., 2], kp0[..., 2])
    ref, ridx, applied = F.decode(hm)
    g = kp.cpu().numpy()
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(g[..., 2].view(np.int32), ref[..., 2].view(np.int32))
    integer = np.stack([ridx % w, ridx // w], -1).astype(np.float32)
    # no step: exactly the integer arg-max; a step: within one f32 ulp of the restatement
    np.testing.assert_array_equal(g[..., :2][~applied], integer[~applied])
    ulp = np.spacing(np.abs(ref[..., :2]))
    err = np.abs(g[..., :2] - ref[..., :2])
    assert np.all(err <= ulp), (err / ulp).max()
    assert applied.any()
    if applied.size >= 12:
        assert not applied.all()


def test_batch_invariance(env):
    rng = np.random.default_rng(7)
    hm = _planes(rng, 8 * 11, 64, 96).reshape(8, 11, 64, 96)
    t = torch.from_numpy(hm).cuda()
    full = env["inference"].heatmaps_to_keypoints(t, refine="get_final2")
    for i in (0, 3, 7):
        one = env["inference"].heatmaps_to_keypoints(t[i:i + 1].clone(), refine="get_final2")
        assert _same(one[0], full[i]), i
    two = env["inference"].heatmaps_to_keypoints(t[2:5], refine="get_final2")
    assert _same(two, full[2:5])


def test_get_final2_matches_the_reference_fixtures(env, golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "final2_*.npz")))
    assert len(files) >= 7
    for p in files:
        d = np.load(p)
        hm = d["hm"].copy()
        out = env["inference"].get_final2(hm, d["coords"].copy())
        np.testing.assert_array_equal(hm, d["hm"])                 # the caller's array is not modified
        assert out.shape == d["out"].shape and out.dtype == np.float32
        np.testing.assert_allclose(out, d["out"], rtol=0, atol=REF_TOL, err_msg=os.path.basename(p))


def _build(env, name, precision="fp32", seed=53, gain=0.5):
    cin, k, w = NETS[name]
    net = env[name].get_seg_model(env["config"].make_config(widths=w), precision=precision)
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=seed, gain=gain)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


@pytest.mark.parametrize("name,precision", [("seg_hrnet", "fp32"), ("seg_hrnet2", "fp32"), ("seg_hrnet3", "fp32"),
                                            ("seg_hrnet2", "bf16x3"), ("seg_hrnet3", "bf16")])
def test_forward_keypoints_equal_the_heatmap_path(env, name, precision):
    net = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate([(2, 64, 64), (3, 48, 80)]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=90 + i).cuda()
        with torch.no_grad():
            kp, idx = net(x, output="keypoints+index", refine="get_final2")
            kp1 = net(x, output="keypoints", refine="get_final2")
            heat = net(x)
            ref, ridx = env["inference"]._keypoints(heat, True, "get_final2")
            dflt = net(x, output="keypoints")
        torch.cuda.synchronize()
        assert _same(kp, ref) and _same(kp1, ref) and torch.equal(idx, ridx)
        assert _same(kp[..., 2], dflt[..., 2])


def test_graph_capture_and_data_parallel(env):
    net = _build(env, "seg_hrnet2", "fp32")
    x = env["synth"].make_crops(4, 1, 64, 64, seed=2).cuda()
    with torch.no_grad():
        kp0 = net(x, output="keypoints", refine="get_final2").clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(x, output="keypoints", refine="get_final2")
            env["inference"].heatmaps_to_keypoints(net(x), refine="get_final2")
        torch.cuda.current_stream().wait_stream(s)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            kpg = net(x, output="keypoints", refine="get_final2")
            kph = env["inference"].heatmaps_to_keypoints(net(x), refine="get_final2")
        gph.replay()
        torch.cuda.synchronize()
        assert _same(kpg, kp0) and _same(kph, kp0)
        dp = torch.nn.DataParallel(net, device_ids=[0])
        assert _same(dp(x, output="keypoints", refine="get_final2"), kp0)
        kp_dp, _ = dp(x, output="keypoints+index", refine="get_final2")
        assert _same(kp_dp, kp0)


def test_entry_errors(env):
    lib, L = env["lib"], env["L"]
    n, k, h, w = 2, 3, 40, 70
    t = torch.rand((n, k, h, w), device="cuda")
    need = C.c_size_t()
    L.check(lib.esahrnet_keypoints_final2_workspace_bytes(n, k, h, w, C.byref(need)))
    ws = torch.empty(need.value + 512, dtype=torch.uint8, device="cuda")
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    kp = torch.empty((n, k, 3), device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.esahrnet_keypoints_final2(t.data_ptr(), n, k, h, w, kp.data_ptr(), None, wp, need.value - 4, stream) != 0
    assert b"too small" in lib.esahrnet_last_error()
    assert lib.esahrnet_keypoints_final2(t.data_ptr(), n, k, h, w, kp.data_ptr(), None, wp + 8, need.value, stream) != 0
    assert b"aligned" in lib.esahrnet_last_error()
    L.check(lib.esahrnet_keypoints_final2(t.data_ptr(), n, k, h, w, kp.data_ptr(), None, wp, need.value, stream))
    torch.cuda.synchronize()
    assert _same(kp, env["inference"].heatmaps_to_keypoints(t, refine="get_final2"))
