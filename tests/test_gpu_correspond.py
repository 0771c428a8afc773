"""The correspondence stage on the GPU (include/esahrnet.h: esahrnet_keypoints_final2_hess,
esahrnet_forward_keypoints_final2_hess, esahrnet_correspondences, esahrnet_frames_correspondences): the Hessian the get_final2
step used comes out beside bit-identical keypoints and agrees with its f64 restatement and with the analytic Hessian of a
blurred Gaussian blob; every keypoints-only forward form gives the stand-alone decoder's bits; correspond_kernel equals the host
rule (select_keypoints, crop_to_image) bit for bit; the one-call form equals its parts, eagerly and in a graph; and
pipeline.estimate_poses(device_select=True) gives the poses of device_loader=True."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correspond_ref as R  # noqa: E402
import final2_ref as F  # noqa: E402
import test_crops_pipeline as TCP  # noqa: E402  (its scene: BOXES)

pytestmark = pytest.mark.gpu

NETS = {"seg_hrnet2": (1, 11, (16, 32, 64, 128)), "seg_hrnet3": (1, 30, (16, 16, 32, 64))}
# tests/test_gpu_final2.py grants the offsets one f32 ulp of the coordinate, 2^-23 of its magnitude at most; the Hessian gets
# the same relative tolerance, relative to its own scale (its largest entry)
REL_TOL = 2.0 ** -23
# Rotated anisotropic Gaussian blobs (ANISO below): deviation of the f64 restatement (correspond_ref.hessian_plane) from the
# analytic -(Sigma + 4 I)^-1, relative to the Hessian's largest entry, computed on the CPU: 4.79e-3 at worst (the 11-tap blur
# is a truncated, sampled sigma-2 Gaussian, so its variance is a little under 4; the central differences of a quadratic are
# exact).  The CPU restatement is held to that figure, the GPU to twice it.
ANALYTIC_DEV = 4.8e-3
ANISO = [(30.3, 31.6, 1.5, 1.0, 0.3), (20.7, 40.2, 2.5, 1.5, 1.1), (33.5, 28.5, 3.0, 2.0, 2.0), (41.25, 22.75, 2.0, 4.0, 0.7),
         (25.0, 25.0, 3.0, 1.0, 2.6), (36.9, 35.1, 2.0, 2.0, 0.0), (28.4, 33.3, 4.0, 1.5, 1.5708), (31.0, 30.5, 1.0, 3.0, 0.9)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, crops, inference, pipeline, pnp, seg_hrnet2, seg_hrnet3, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, crops=crops, inference=inference, pipeline=pipeline, pnp=pnp, synth=synth,
                seg_hrnet2=seg_hrnet2, seg_hrnet3=seg_hrnet3)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)


def _bits(a, b):
    """Bit-identical tensors (NaN included)."""
    a, b = a.contiguous(), b.contiguous()
    it = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _np_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    it = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(it), b.view(it))


def _build(env, name, precision="fp32", seed=53, gain=0.5, widths=None):
    cin, k, w = NETS[name]
    net = env[name].get_seg_model(env["config"].make_config(widths=widths or w), precision=precision)
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=seed, gain=gain)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


# ---- 1. the decoder's Hessian on the reference's fixtures ---------------------------------------------------------------------
def test_hessian_on_the_reference_fixtures(env, golden_dir):
    inf = env["inference"]
    files = sorted(glob.glob(os.path.join(golden_dir, "final2_*.npz")))
    assert len(files) >= 7
    seen = dict(applied=0, skipped=0)
    for p in files:
        hm = np.load(p)["hm"]
        t = torch.from_numpy(hm).cuda()
        kp0, idx0 = inf._keypoints(t, True, "get_final2")                   # esahrnet_keypoints_final2
        kp, idx, hess = inf._keypoints(t, True, "get_final2", True)        # esahrnet_keypoints_final2_hess
        kp2, hess2 = inf.heatmaps_to_keypoints(t, refine="get_final2", return_hessian=True)
        torch.cuda.synchronize()
        name = os.path.basename(p)
        assert _bits(kp, kp0) and torch.equal(idx, idx0) and _bits(kp2, kp0) and _bits(hess2, hess), name
        assert hess.dtype == torch.float64 and hess.shape == kp.shape
        ref, applied = R.hessian(hm)
        g = hess.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.repeat(~applied[..., None], 3, -1)), name      # NaN exactly where no step
        scale = np.abs(ref[applied]).max(-1, keepdims=True)
        err = np.abs(g[applied] - ref[applied])
        print(name, "applied", int(applied.sum()), "of", applied.size, "max err / scale", float((err / scale).max()) if err.size else 0.0)
        assert np.all(err <= REL_TOL * scale), (name, float((err / scale).max()))
        seen["applied"] += int(applied.sum())
        seen["skipped"] += int((~applied).sum())
    assert seen["applied"] > 20 and seen["skipped"] > 0, seen


# ---- 2. rotated anisotropic Gaussians: the analytic Hessian ---------------------------------------------------------------------
def test_hessian_of_anisotropic_gaussians_is_the_information_matrix(env):
    planes = np.stack([F.gaussian_planes(64, 64, [(cx, cy)], sx, sy, th)[0] for cx, cy, sx, sy, th in ANISO])[None]
    exact = np.stack([R.gaussian_hessian(sx, sy, th) for _, _, sx, sy, th in ANISO])
    scale = np.abs(exact).max(-1, keepdims=True)
    ref, applied = R.hessian(planes)
    assert applied.all()
    cpu_dev = float((np.abs(ref[0] - exact) / scale).max())
    _, hess = env["inference"].heatmaps_to_keypoints(torch.from_numpy(planes).cuda(), refine="get_final2", return_hessian=True)
    gpu_dev = float((np.abs(hess[0].cpu().numpy() - exact) / scale).max())
    print("deviation from -(Sigma + 4 I)^-1, relative: restatement", cpu_dev, "GPU", gpu_dev)
    assert cpu_dev <= ANALYTIC_DEV
    assert gpu_dev <= 2 * ANALYTIC_DEV
    # and -H is positive definite: the weight of mode 1 exists for every one of them
    g = -hess[0].cpu().numpy()
    assert np.all(g[:, 0] > 0) and np.all(g[:, 0] * g[:, 2] - g[:, 1] ** 2 > 0)


# ---- 3. every keypoints-only forward form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("seg_hrnet2", "fp32"), ("seg_hrnet2", "bf16"), ("seg_hrnet3", "fp32")])
def test_forward_forms_equal_forward_then_the_decoder(env, name, precision):
    """seg_hrnet2 fp32: the VALU output layer re-evaluated; bf16: the matrix-core output layer; seg_hrnet3: the NHWC maps."""
    net = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate([(2, 64, 64), (3, 48, 80)]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=90 + i).cuda()
        with torch.no_grad():
            kp, idx, hess = net.keypoints_hessian(x)
            kp1, idx1 = net(x, output="keypoints+index", refine="get_final2")
            rkp, ridx, rhess = env["inference"]._keypoints(net(x), True, "get_final2", True)
        torch.cuda.synchronize()
        assert _bits(kp, rkp) and torch.equal(idx, ridx) and _bits(hess, rhess)
        assert _bits(kp1, rkp) and torch.equal(idx1, ridx)                  # the call without the Hessian: unchanged bits
        print(name, precision, (n, hh, ww), "steps taken:", int(torch.isfinite(hess[..., 0]).sum()), "of", hess[..., 0].numel())


# ---- 4. correspond_kernel against the host rule ---------------------------------------------------------------------------------
def _keypoint_rows(rng, m, k):
    kp = np.empty((m, k, 3), np.float32)
    kp[..., :2] = rng.uniform(0, 255, (m, k, 2)).astype(np.float32)
    kp[..., 2] = rng.uniform(0.0, 1.0, (m, k)).astype(np.float32)
    kp[1, :, 2] = rng.uniform(0.0, 0.5, k)                                   # every peak below the thresholds used: min_k applies
    kp[2, :, 2] = np.float32(0.9)                                            # all equal: index order
    kp[3, ::2, 2] = np.float32(0.85)                                         # ties among the selected ...
    kp[3, 1::2, 2] = np.float32(0.3)                                         # ... and among the rest
    kp[4, :, 2] = rng.uniform(0.81, 1.0, k)                                  # every peak above
    kp[5, [0, k - 1], 2] = np.float32(0.0)                                   # exactly the threshold 0.0: not above it
    kp[6, 1, 2] = kp[6, k - 2, 2] = np.nan                                   # NaN peaks are never selected
    kp[7, :, 2] = [0.0, -0.0] * (k // 2) + [0.0] * (k % 2)                   # +0 == -0: index order
    return kp


@pytest.mark.parametrize("k", [11, 30, 32, 1])
def test_correspond_kernel_equals_the_host_rule(env, k):
    inf = env["inference"]
    rng = np.random.default_rng(40 + k)
    m = 12
    kp = _keypoint_rows(rng, m, k) if k >= 4 else rng.uniform(0, 1, (m, k, 3)).astype(np.float32)
    boxes = np.stack([rng.integers(0, 1700, m), rng.integers(0, 1000, m), rng.integers(0, 1, m), rng.integers(0, 1, m)], 1).astype(np.int32)
    boxes[:, 2:] = boxes[:, :2] + rng.integers(1, 700, (m, 2))
    rates = rng.uniform(0.3, 4.0, m)
    rates[0] = 1.0
    rates[4] = 256 / 367
    valid = np.ones(m, np.int32)
    valid[[8, 11]] = 0                                                       # invalid crops: count 0
    kp[8] = np.nan
    hess = np.empty((m, k, 3))
    th, l1, l2 = rng.uniform(0, np.pi, (m, k)), rng.uniform(0.02, 0.5, (m, k)), rng.uniform(0.02, 0.5, (m, k))
    c, s = np.cos(th), np.sin(th)
    hess[..., 0], hess[..., 1], hess[..., 2] = -(l1 * c * c + l2 * s * s), -(l1 - l2) * c * s, -(l1 * s * s + l2 * c * c)
    hess[0, 0] = np.nan                                                      # no step was taken
    hess[4, k - 1] = [0.1, 0.0, -0.2]                                        # a saddle: dxx > 0
    hess[9, 0] = [-0.1, 0.2, -0.1]                                           # det < 0
    hess[10, 0] = [0.0, 0.0, 0.0]
    dev = lambda a: torch.from_numpy(a).cuda()                               # noqa: E731
    tk, tb, tr, tv, th_ = dev(kp), dev(boxes), dev(rates), dev(valid), dev(hess)
    seen = dict(min_k_applies=0, above=0, all_k=0, zero_w=0)
    for thresh, min_k in ((0.8, 0), (0.8, 5), (0.8, k + 3), (0.0, 0), (0.6, 24), (2.0, 0)):
        count, order, pts, w = inf.keypoints_to_correspondences(tk, tb, tr, tv, thresh=thresh, min_k=min_k)
        count1, order1, pts1, w1 = inf.keypoints_to_correspondences(tk, tb, tr, tv, hess=th_, thresh=thresh, min_k=min_k,
                                                                    weights="hessian")
        torch.cuda.synchronize()
        ec, eo, ep, ew = R.record(kp, boxes, rates, valid, thresh, min_k)
        _, _, _, ew1 = R.record(kp, boxes, rates, valid, thresh, min_k, hess)
        tag = (k, thresh, min_k)
        assert count.dtype == torch.int32 and order.dtype == torch.int32 and pts.dtype == torch.float64
        assert count.cpu().tolist() == ec.tolist(), tag
        assert order.cpu().tolist() == eo.tolist(), tag
        assert _np_bits(pts.cpu().numpy(), ep), tag
        assert _np_bits(w.cpu().numpy(), ew), tag                            # mode 0: bit-exact
        assert torch.equal(count1, count) and torch.equal(order1, order) and _bits(pts1, pts), tag
        g1 = w1.cpu().numpy()
        assert np.array_equal(g1 == 0, ew1 == 0), tag                        # the zero weights, exactly
        assert np.all(np.abs(g1 - ew1) <= 4 * np.spacing(np.abs(ew1))), tag  # mode 1: within 4 f64 ulp of the closed form
        assert ec[8] == 0 and ec[11] == 0 and (eo[8] == -1).all()
        for i in range(m):
            if valid[i]:
                above = int(np.sum(kp[i, :, 2] > thresh))
                seen["min_k_applies"] += above < min_k
                seen["above"] += above > min_k
                seen["all_k"] += ec[i] == k
        seen["zero_w"] += int(np.sum((ew1 == 0).all(-1) & (eo >= 0)))
    assert all(v > 0 for v in seen.values()), seen


def test_correspondences_entry_errors(env):
    lib, L = env["lib"], env["L"]
    m, k = 2, 11
    kp = torch.rand((m, k, 3), device="cuda")
    boxes = torch.zeros((m, 4), dtype=torch.int32, device="cuda")
    rates = torch.ones(m, dtype=torch.float64, device="cuda")
    valid = torch.ones(m, dtype=torch.int32, device="cuda")
    count, order, pts, w, _ = env["inference"].pack_correspondences(m, k, "cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = lambda kk, mode, hess=None: (kp.data_ptr(), hess, boxes.data_ptr(), rates.data_ptr(), valid.data_ptr(), m, kk, 0.8, 4,   # noqa: E731
                                        mode, count.data_ptr(), order.data_ptr(), pts.data_ptr(), w.data_ptr(), stream)
    assert lib.esahrnet_correspondences(*args(33, 0)) != 0 and b"1..32" in lib.esahrnet_last_error()
    assert lib.esahrnet_correspondences(*args(k, 2)) != 0 and b"mode" in lib.esahrnet_last_error()
    assert lib.esahrnet_correspondences(*args(k, 1)) != 0 and b"hess_dev" in lib.esahrnet_last_error()
    L.check(lib.esahrnet_correspondences(*args(k, 0)))
    torch.cuda.synchronize()
    assert count.tolist() == [max(4, int((kp[i, :, 2] > 0.8).sum())) for i in range(m)]
    with pytest.raises(ValueError, match="hess"):
        env["inference"].keypoints_to_correspondences(kp, boxes, rates, valid, weights="hessian")


# ---- 5. the one-call form equals its parts, eagerly and in a graph ----------------------------------------------------------------
def _frames(env, name, n, seed=3):
    return torch.from_numpy(env["synth"].uniform(name, seed, (n, 1200, 1920), 0, 255.99).astype(np.uint8)).cuda()


@pytest.mark.parametrize("name,scale,refine,weights", [("seg_hrnet3", 64, "get_final2", "hessian"), ("seg_hrnet3", 64, "get_final", "peak"),
                                                        ("seg_hrnet2", 128, "get_final2", "hessian"), ("seg_hrnet2", 128, "get_final2", "peak")])
def test_frames_to_correspondences_equals_its_parts(env, name, scale, refine, weights):
    inf, crops = env["inference"], env["crops"]
    net = _build(env, name, widths=(16, 16, 32, 64) if name == "seg_hrnet3" else None, gain=1.0)
    frames = _frames(env, "frames", 3)
    boxes = list(TCP.BOXES[:4]) + [(500, 500, 500, 500)]                      # the last one: an empty box
    fidx = [0, 1, 2, 2, 1]
    kw = dict(frame_idx=fidx, scale=scale, refine=refine)
    sel = dict(thresh=0.1, min_k=6)
    with torch.no_grad():
        out = net.frames_to_correspondences(frames, boxes, weights=weights, **kw, **sel)
        kp, cboxes, rates, valid = net.frames_to_keypoints(frames, boxes, **kw)
        hess = None
        if weights == "hessian":
            x = crops.crop_batch_device(frames, boxes, frame_idx=fidx, scale=scale)[0]
            hess = net.keypoints_hessian(x)[2]
        parts = inf.keypoints_to_correspondences(kp, cboxes, rates, valid, hess=hess, weights=weights, **sel)
        torch.cuda.synchronize()
        assert all(_bits(a, b) for a, b in zip(out[:4], parts)), [(_bits(a, b)) for a, b in zip(out[:4], parts)]
        assert _bits(out[4], kp) and _bits(out[5], cboxes) and _bits(out[6], rates) and _bits(out[7], valid)
        assert out[0].tolist()[4] == 0 and min(out[0].tolist()[:4]) >= 6 and valid.tolist() == [1, 1, 1, 1, 0]
        print(name, refine, weights, "count", out[0].tolist(), "points with a weight:", int((out[3].abs().sum(-1) > 0).sum()))
        # captured once, replayed: the same bits
        fr, det = frames.clone(), torch.tensor(boxes, dtype=torch.int32, device="cuda")
        fi = torch.tensor(fidx, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net.frames_to_correspondences(fr, det, frame_idx=fi, scale=scale, refine=refine, weights=weights, **sel)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = net.frames_to_correspondences(fr, det, frame_idx=fi, scale=scale, refine=refine, weights=weights, **sel)
        g.replay()
        torch.cuda.synchronize()
        assert all(_bits(a, b) for a, b in zip(cap, out))


def test_frames_correspondences_refusals(env):
    net = _build(env, "seg_hrnet3", widths=(16, 16, 32, 64))
    frames = _frames(env, "frames", 1)
    with pytest.raises(ValueError, match="get_final2"):
        net.frames_to_correspondences(frames, [TCP.BOXES[0]], scale=64, weights="hessian")
    with pytest.raises(ValueError, match="weights must be"):
        net.frames_to_correspondences(frames, [TCP.BOXES[0]], scale=64, weights="blur")
    lib = env["lib"]
    need = C.c_size_t()
    net.frames_to_keypoints(frames, [TCP.BOXES[0]], scale=64)                 # makes the handle
    h = net._rt._handle_for(net, frames.device)
    assert lib.esahrnet_frames_correspondences_workspace_bytes(h, 1, 64, 0, 1, C.byref(need)) != 0
    assert b"decoder 1" in lib.esahrnet_last_error()
    assert lib.esahrnet_frames_correspondences_workspace_bytes(h, 1, 64, 1, 1, C.byref(need)) == 0
    hess_bytes = need.value
    assert lib.esahrnet_frames_correspondences_workspace_bytes(h, 1, 64, 1, 0, C.byref(need)) == 0
    assert hess_bytes - need.value == 768                                    # 30 keypoints x 24 bytes, rounded up to 256


# ---- 6. the pipeline --------------------------------------------------------------------------------------------------------------
def _same_poses(a, b):
    return len(a) == len(b) and all(_np_bits(np.asarray(qa, np.float64), np.asarray(qb, np.float64)) and
                                    _np_bits(np.asarray(ta, np.float64), np.asarray(tb, np.float64))
                                    for (qa, ta), (qb, tb) in zip(a, b))


def test_estimate_poses_with_device_select(env):
    pipeline, synth = env["pipeline"], env["synth"]
    net = _build(env, "seg_hrnet2", widths=None, gain=1.0, seed=53)
    n = 16
    scene = synth.make_scene(n, net.num_keypoints, seed=0)
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(n, 1200, 1920), dtype=np.uint8)).cuda()
    kw = dict(scale=128, thresh=0.0, min_k=8, on_fail="nan")
    for refine in ("get_final", "get_final2"):
        ref = pipeline.estimate_poses(net, frames, scene["bboxes"], scene["kp3d"], synth.ESA_CAMERA, refine=refine,
                                      device_loader=True, **kw)
        got = pipeline.estimate_poses(net, frames, scene["bboxes"], scene["kp3d"], synth.ESA_CAMERA, refine=refine,
                                      device_select=True, **kw)
        assert _same_poses(got, ref), refine                                 # "peak": pose for pose, bit for bit
    # an invalid crop and two boxes on one frame
    boxes = scene["bboxes"][:3] + [[700, 700, 700, 700]]
    boxes[2] = scene["bboxes"][1]
    fidx = [0, 1, 1, 2]
    ref = pipeline.estimate_poses(net, frames[:3], boxes, scene["kp3d"], synth.ESA_CAMERA, device_loader=True, frame_idx=fidx, **kw)
    got = pipeline.estimate_poses(net, frames[:3], boxes, scene["kp3d"], synth.ESA_CAMERA, device_select=True, frame_idx=fidx, **kw)
    assert _same_poses(got, ref) and np.isnan(got[3][0]).all()
    with pytest.raises(pipeline.PoseFailure, match=r"\b3\b"):
        pipeline.estimate_poses(net, frames[:3], boxes, scene["kp3d"], synth.ESA_CAMERA, device_select=True, frame_idx=fidx,
                                scale=128, thresh=0.0, min_k=8)
    # the Hessian weights: another refinement of the same RANSAC solution, a row per crop
    hes = pipeline.estimate_poses(net, frames, scene["bboxes"], scene["kp3d"], synth.ESA_CAMERA, refine="get_final2",
                                  device_select=True, weights="hessian", **kw)
    assert len(hes) == n and all(np.asarray(q).shape == (4,) and np.asarray(t).shape == (3,) for q, t in hes)
    with pytest.raises(ValueError, match="get_final2"):
        pipeline.estimate_poses(net, frames, scene["bboxes"], scene["kp3d"], synth.ESA_CAMERA, device_select=True, weights="hessian")
    with pytest.raises(ValueError, match="device_select"):
        pipeline.estimate_poses(net, frames, scene["bboxes"], scene["kp3d"], synth.ESA_CAMERA, refine="get_final2",
                                weights="hessian")
