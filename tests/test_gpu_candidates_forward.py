"""net.candidates(x, M, r) runs esahrnet_forward_keypoints_candidates (include/esahrnet.h): cand and cidx bit-identical to
esahrnet_forward + esahrnet_keypoints_candidates (net(x) followed by inference.heatmaps_to_candidates) for every network,
precision and output-layer form, at 64 x 64 (the one-sweep kernel behind the output layer) and at an odd shape of the
keypoints-only tests whose width is no multiple of 4 (the multi-sweep kernel), batch-invariant, in a graph, whatever the
workspace held on entry; the loader in front of it (esahrnet_frames_keypoints_candidates) through net.frames_to_candidates; and
pipeline.estimate_poses(candidates=3, candidates_path="fused" / "loader") against the heat-map path.

The networks carry the fixtures' synthetic weights on random crops: noisy maps with many local maxima; the pipeline test draws
the wrong-blob scene of tests/test_gpu_candidates.py as frames (_wrong_blob_frames)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_crops_pipeline as TCP  # noqa: E402  (its scene: BOXES)

pytestmark = pytest.mark.gpu

NETS = {"seg_hrnet": (3, 32, (16, 32, 64, 128)), "seg_hrnet2": (1, 11, (16, 32, 64, 128)), "seg_hrnet3": (1, 30, (16, 16, 32, 64))}
PRECISIONS = ["fp32", "bf16x3", "bf16"]
CASES = [(n, p) for n in NETS for p in PRECISIONS]
SHAPES = {0: [(2, 64, 64), (2, 18, 34)], 1: [(2, 64, 64), (3, 34, 18)]}      # seg_hrnet / seg_hrnet2, seg_hrnet3
MR = [(1, 1), (1, 6), (3, 1), (3, 6)]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, crops, inference, pipeline, pnp, seg_hrnet, seg_hrnet2, seg_hrnet3, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, crops=crops, inference=inference, pipeline=pipeline, pnp=pnp, synth=synth,
                seg_hrnet=seg_hrnet, seg_hrnet2=seg_hrnet2, seg_hrnet3=seg_hrnet3)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


def _build(env, name, precision="fp32", seed=53, gain=0.5):
    cin, k, w = NETS[name]
    net = env[name].get_seg_model(env["config"].make_config(widths=w), precision=precision)
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=seed, gain=gain)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _bits(a, b):
    """Bit-identical tensors: the same NaN mask, the same bits."""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point() and not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(env, net, x, mr=MR):
    """The fused call against esahrnet_forward + esahrnet_keypoints_candidates, and candidate 0 against the keypoints-only forward."""
    with torch.no_grad():
        heat = net(x)
        kp, idx = net(x, output="keypoints+index")
        seen = 0
        for M, r in mr:
            rc, ri = env["inference"].heatmaps_to_candidates(heat, M, r, return_index=True)
            cand, cidx = net.candidates(x, M, r, return_index=True)
            only = net.candidates(x, candidates=M, nms_radius=r)
            torch.cuda.synchronize()
            assert cand.shape == (x.shape[0], net.num_keypoints, M, 3) and cidx.dtype == torch.int32 and cidx.shape == cand.shape[:3]
            assert _bits(cand, rc) and torch.equal(cidx, ri) and _bits(only, rc), (M, r)
            assert _bits(cand[:, :, 0], kp) and torch.equal(cidx[:, :, 0], idx), (M, r)
            seen += int((ri[:, :, 1:] >= 0).sum())
    return seen


# ---- 1. every net, precision and output-layer form ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_equal_to_forward_plus_keypoints_candidates(env, name, precision):
    net = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate(SHAPES[1 if name == "seg_hrnet3" else 0]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=260 + i).cuda()
        seen = _check(env, net, x)
        print(name, precision, (n, hh, ww), "runner-ups found:", seen)
        assert seen > 0


@pytest.mark.parametrize("name,precision", [("seg_hrnet2", "bf16x3"), ("seg_hrnet", "bf16")])
def test_valu_output_layer_on_a_matrix_core_precision(env, monkeypatch, name, precision):
    monkeypatch.setenv("ESAHRNET_FINAL_VALU", "1")
    net = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate(SHAPES[0]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=270 + i).cuda()
        assert _check(env, net, x) > 0


# ---- 2. batch invariance and graph replay ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_batch_one_against_the_same_crop_in_batch_three(env, name):
    net = _build(env, name, "fp32")
    x = env["synth"].make_crops(3, 1, 64, 64, seed=5).cuda()
    with torch.no_grad():
        full = net.candidates(x, 3, 6, return_index=True)
        for i in range(3):
            one = net.candidates(x[i:i + 1], 3, 6, return_index=True)
            assert _bits(one[0][0], full[0][i]) and torch.equal(one[1][0], full[1][i]), i


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_graph_replay(env, name):
    net = _build(env, name, "fp32")
    xs = [env["synth"].make_crops(2, 1, 64, 64, seed=s).cuda() for s in (2, 3, 4)]
    x = xs[0].clone()
    with torch.no_grad():
        refs = [[t.clone() for t in net.candidates(xi, 3, 6, return_index=True)] for xi in xs]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net.candidates(x, 3, 6, return_index=True)
        torch.cuda.current_stream().wait_stream(s)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            out = net.candidates(x, 3, 6, return_index=True)
        for i in (1, 2):                                    # replayed twice, each time on another input
            x.copy_(xs[i])
            gph.replay()
            torch.cuda.synchronize()
            assert _bits(out[0], refs[i][0]) and torch.equal(out[1], refs[i][1]), i
        assert not _bits(refs[1][0], refs[2][0])


# ---- 3. the workspace ---------------------------------------------------------------------------------------------------------------
def _raw_call(env, net, x, M, r, ws_fill=None, ws_short=0):
    """esahrnet_forward_keypoints_candidates on buffers of the test's own, the outputs pre-filled with 0xA5: -> (rc, cand, cidx)."""
    lib, L = env["lib"], env["L"]
    n, _, hh, ww = x.shape
    k = net.num_keypoints
    h = net._rt._handle_for(net, x.device)
    need, fwd = C.c_size_t(), C.c_size_t()
    L.check(lib.esahrnet_keypoints_candidates_forward_workspace_bytes(h, n, hh, ww, C.byref(need)))
    L.check(lib.esahrnet_workspace_bytes(h, n, hh, ww, C.byref(fwd)))
    assert need.value == fwd.value + ((n * k * hh * ww * 4 + 255) & ~255)         # the forward's plus the padded heat-maps
    ws = torch.zeros(need.value + 512, dtype=torch.uint8, device="cuda")
    if ws_fill == "nan":
        ws[:(ws.numel() // 4) * 4].view(torch.float32).fill_(float("nan"))
    elif ws_fill is not None:
        ws.fill_(ws_fill)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    cand = torch.empty((n, k, M, 3), dtype=torch.float32, device="cuda")
    cidx = torch.empty((n, k, M), dtype=torch.int32, device="cuda")
    cand.view(torch.uint8).fill_(0xA5)
    cidx.view(torch.uint8).fill_(0xA5)
    rc = lib.esahrnet_forward_keypoints_candidates(h, x.data_ptr(), n, hh, ww, M, r, cand.data_ptr(), cidx.data_ptr(), wp,
                                                   need.value - ws_short, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, cand, cidx


@pytest.mark.parametrize("name,precision", [("seg_hrnet2", "fp32"), ("seg_hrnet2", "bf16x3"), ("seg_hrnet3", "fp32")])
def test_workspace_contents_on_entry_do_not_matter(env, name, precision):
    net = _build(env, name, precision)
    for shape in SHAPES[1 if name == "seg_hrnet3" else 0]:
        x = env["synth"].make_crops(*shape[:1], 1, *shape[1:], seed=4).cuda()
        with torch.no_grad():
            want = env["inference"].heatmaps_to_candidates(net(x), 3, 6, return_index=True)
        for ws_fill in (None, "nan", 0xFF):
            rc, cand, cidx = _raw_call(env, net, x, 3, 6, ws_fill)
            assert rc == 0, env["lib"].esahrnet_last_error()
            assert _bits(cand, want[0]) and torch.equal(cidx, want[1]), (shape, ws_fill)
        # a workspace one byte short of the query: refused, nothing enqueued, the outputs as pre-filled
        rc, cand, cidx = _raw_call(env, net, x, 3, 6, ws_short=1)
        assert rc != 0 and b"too small" in env["lib"].esahrnet_last_error()
        assert bool((cand.view(torch.uint8) == 0xA5).all()) and bool((cidx.view(torch.uint8) == 0xA5).all())


# ---- 4. the loader in front of it ------------------------------------------------------------------------------------------------
def _frames(env, name, n, seed=3):
    return torch.from_numpy(env["synth"].uniform(name, seed, (n, 1200, 1920), 0, 255.99).astype(np.uint8)).cuda()


SCENE_BOXES = [TCP.BOXES[0], TCP.BOXES[1], (500, 500, 500, 500), TCP.BOXES[2], TCP.BOXES[3]]      # position 2: an empty box
SCENE_FIDX = [0, 1, 0, 1, 2]                                                                     # position 4: no such frame
SCENE_VALID = [1, 1, 0, 1, 0]


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_loader_equals_crop_batch_then_candidates(env, name):
    """Gray frames, one val box per frame: what crops.crop_batch and net.candidates give, bit for bit."""
    net = _build(env, name, "fp32", gain=1.0)
    frames = _frames(env, "frames", 3)
    boxes_in = [TCP.BOXES[0], TCP.BOXES[1], TCP.BOXES[2]]
    with torch.no_grad():
        x, rboxes, rrates = env["crops"].crop_batch(frames, boxes_in, 64)
        want = net.candidates(x, 3, 6, return_index=True)
        cand, boxes, rates, valid = net.frames_to_candidates(frames, boxes_in, scale=64, candidates=3, nms_radius=6)
        r = net._loader(env["inference"].LoaderRequest("get_final", (3, 6)), frames, boxes_in, None, 64, "val", None, 0.229, None)
        cand2, cidx = r["cand"], r["cidx"]
    torch.cuda.synchronize()
    assert valid.tolist() == [1, 1, 1] and _bits(cand, want[0]) and _bits(cand2, want[0]) and torch.equal(cidx, want[1])
    assert boxes.tolist() == [[int(v) for v in b] for b in rboxes] and rates.tolist() == [float(r) for r in rrates]


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_loader_with_a_frame_index_and_invalid_crops(env, name):
    inf, crops = env["inference"], env["crops"]
    net = _build(env, name, "fp32", gain=1.0)
    frames = _frames(env, "frames", 2)
    M = 3
    with torch.no_grad():
        x, rboxes, rrates, rvalid = crops.crop_batch_device(frames, SCENE_BOXES, frame_idx=SCENE_FIDX, scale=64)
        rcand, rcidx = net.candidates(x, M, 6, return_index=True)
        r = net._loader(inf.LoaderRequest("get_final", (M, 6)), frames, SCENE_BOXES, SCENE_FIDX, 64, "val", None, 0.229, None)
        cand, boxes, rates, valid, cidx = (r[n] for n in ("cand", "boxes", "rates", "valid", "cidx"))
        (packed, _), = r.records.values()
        four = net.frames_to_candidates(frames, SCENE_BOXES, frame_idx=SCENE_FIDX, scale=64, candidates=M, nms_radius=6)
    torch.cuda.synchronize()
    assert len(four) == 4 and _bits(four[0], cand) and _bits(four[1], boxes) and _bits(four[2].view(torch.int32), rates.view(torch.int32))
    assert valid.tolist() == SCENE_VALID == rvalid.tolist() and _bits(boxes, rboxes) and torch.equal(rates, rrates)
    good, bad = [i for i, v in enumerate(SCENE_VALID) if v], [i for i, v in enumerate(SCENE_VALID) if not v]
    # two boxes on frame 0 and two on frame 1; the rows beside the invalid ones are what the parts give
    assert _bits(cand[good], rcand[good]) and torch.equal(cidx[good], rcidx[good])
    assert bool(torch.isnan(cand[bad]).all()) and bool((cidx[bad] == -1).all())
    # the packed buffer: every output is the view that inference.packed_layout names
    k = net.num_keypoints
    lay = inf.packed_layout(5, k, candidates=M)
    assert packed.dtype == torch.uint8 and packed.numel() == lay["total"][1]
    for name_, t in (("rates", rates), ("cand", cand), ("boxes", boxes), ("valid", valid), ("cidx", cidx)):
        off, nbytes = lay[name_]
        assert t.data_ptr() == packed.data_ptr() + off and t.numel() * t.element_size() == nbytes and t.is_contiguous(), name_
    assert cand.shape == (5, k, M, 3) and cidx.shape == (5, k, M) and cidx.dtype == torch.int32 and rates.dtype == torch.float64


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------
def _same_poses(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(qa, np.float64).view(np.int64), np.asarray(qb, np.float64).view(np.int64)) and
                                    np.array_equal(np.asarray(ta, np.float64).view(np.int64), np.asarray(tb, np.float64).view(np.int64))
                                    for (qa, ta), (qb, tb) in zip(a, b))


CROP = 84              # crops.val_box of an 80 px detector box: 1.05 * 40 = 42 px on either side of its centre, so rate 1.0


def _patterns(k, seed):
    """k sign patterns [k,3,3] whose cross-correlation stays <= 5, at every shift, of the 9 a pattern has with itself."""
    rng = np.random.default_rng(seed)

    def xcorr_max(a, b):
        best = -9
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ya, yb = slice(max(dy, 0), 3 + min(dy, 0)), slice(max(-dy, 0), 3 + min(-dy, 0))
                xa, xb = slice(max(dx, 0), 3 + min(dx, 0)), slice(max(-dx, 0), 3 + min(-dx, 0))
                best = max(best, int((a[ya, xa] * b[yb, xb]).sum()))
        return best
    out = []
    while len(out) < k:
        p = rng.choice([-1.0, 1.0], (3, 3))
        if all(xcorr_max(p, q) <= 5 and xcorr_max(q, p) <= 5 for q in out):
            out.append(p)
    return np.stack(out)


def _wrong_blob_frames(env, n=4, k=11, nbad=2, seed=7):
    """The wrong-blob scene of tests/test_gpu_candidates.py (n images of a k-keypoint model, nbad keypoints per image with
    amplitude 1.0 at a wrong place and 0.7 at the true one) as camera frames that a network with a one-channel input can read:
    keypoint j is drawn as its own 3 x 3 sign pattern, and an output layer whose filter j is that pattern (_pattern_net) answers
    with 9 x the amplitude where pattern j sits and with at most 5 x anywhere else.  The poses are far enough for the model to
    span 56 px, so every crop is the 84 x 84 pixels of the frame, unscaled.  -> dict(kp3d, K, poses [(R, t)], bboxes (integer
    detector boxes), bad [n][nbad], patterns, frames uint8 [n,1200,1920])."""
    pnp, synth = env["pnp"], env["synth"]
    rng = np.random.default_rng(seed)
    K = synth.ESA_CAMERA
    kp3d = rng.uniform(-0.6, 0.6, (k, 3))
    pat = _patterns(k, seed)
    frames = np.full((n, 1200, 1920), 124.0)                # 124 / 255 is the loader's mean: the background of a crop is 0
    poses, det, bads = [], [], []
    for i in range(n):
        R = pnp.rodrigues(rng.uniform(-1.2, 1.2, 3))
        rot = kp3d @ R.T
        z = K[0, 0] * max(np.ptp(rot[:, 0]), np.ptp(rot[:, 1])) / 56.0
        u0, v0 = rng.uniform(300, 1600), rng.uniform(300, 900)
        t = np.array([(u0 - K[0, 2]) * z / K[0, 0], (v0 - K[1, 2]) * z / K[0, 0], z])
        uv = pnp.project(kp3d, R, t, K)
        c0 = np.round((uv.min(0) + uv.max(0)) / 2).astype(int)
        x0, y0 = c0 - CROP // 2
        c = np.round(uv - [x0, y0]).astype(int)             # the pixel each keypoint is drawn at, (x, y) in the crop
        assert c.min() >= 8 and c.max() <= CROP - 9, (c.min(), c.max())
        bad = np.sort(rng.choice(k, nbad, replace=False))
        spots = [(c[j, 0], c[j, 1], j, 0.7 if j in bad else 1.0) for j in range(k)]
        for j in bad:
            while True:
                p = rng.integers(6, CROP - 6, 2)
                if np.abs(p - c[j]).max() >= 14 and np.abs(p - c).max(1).min() >= 5:
                    break
            spots.append((p[0], p[1], j, 1.0))
        for x, y, j, amp in spots:
            frames[i, y0 + y - 1:y0 + y + 2, x0 + x - 1:x0 + x + 2] += 100.0 * amp * pat[j]
        poses.append((R, t))
        det.append([int(c0[0] - 40), int(c0[1] - 40), int(c0[0] + 40), int(c0[1] + 40)])
        bads.append(bad)
    return dict(kp3d=kp3d, K=K, poses=poses, bboxes=det, bad=bads, patterns=pat, frames=np.clip(frames, 0, 255).astype(np.uint8))


def _pattern_net(env, patterns):
    """seg_hrnet2 whose output layer reads the crop alone: heat-map j = 16 + the crop correlated with pattern j (the bias keeps
    every value positive, so that the log of the sub-pixel step sees numbers)."""
    k = len(patterns)
    net = env["seg_hrnet2"].get_seg_model(env["config"].make_config(widths=NETS["seg_hrnet2"][2]), precision="fp32")
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=53, gain=0.5)
    w = sd["output_layer.0.weight"]
    assert w.shape == (k, k + 1, 3, 3)
    w.zero_()
    w[:, k] = torch.from_numpy(patterns.astype(np.float32))   # the channel behind the K up-sampled ones: the raw crop
    sd["output_layer.0.bias"] = torch.full((k,), 16.0)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def test_estimate_poses_on_the_fused_path_and_behind_the_loader(env):
    """The 4-image, 11-keypoint wrong-blob scene as frames and integer boxes.  On the heat-map path every pose is a number, the
    runner-ups that enter the solves are exactly the two wrong-blob keypoints of each image, every image is rescued and meets
    the no-outlier bound of tests/test_pnp_native.py (0.05; a drawn keypoint sits on a whole pixel, up to 0.5 px off its
    projection); the fused path and the loader then give those poses, .used, .rescued and report rows bit for bit."""
    pipeline, pnp = env["pipeline"], env["pnp"]
    sc = _wrong_blob_frames(env)
    n, k = len(sc["poses"]), len(sc["kp3d"])
    net = _pattern_net(env, sc["patterns"])
    frames = torch.from_numpy(sc["frames"]).cuda()
    kw = dict(scale=CROP, on_fail="nan", thresh=0.0, min_k=8, candidates=3, nms_radius=6, return_report=True)
    args = (net, frames, sc["bboxes"], sc["kp3d"], sc["K"])
    poses, rep = pipeline.estimate_poses(*args, **kw)
    want = np.zeros((n, k), np.int32)
    for i, bad in enumerate(sc["bad"]):
        want[i, bad] = 1
    scores = [pnp.speed_score(q, t, pnp.rotation_to_quat_wxyz(R), tt)[0] for (q, t), (R, tt) in zip(poses, sc["poses"])]
    print("SPEED scores with runner-ups:", [round(float(s_), 5) for s_ in scores], "used > 0:", int((rep.used > 0).sum()))
    assert all(np.isfinite(q).all() and np.isfinite(t).all() for q, t in poses)
    assert np.array_equal(rep.used, want) and rep.rescued.all() and (rep.status == 0).all()
    assert max(scores) < 0.05, scores
    one, _ = pipeline.estimate_poses(*args, **dict(kw, candidates=1))
    s1 = [pnp.speed_score(q, t, pnp.rotation_to_quat_wxyz(R), tt)[0] for (q, t), (R, tt) in zip(one, sc["poses"])]
    assert all(not np.isfinite(a) or a > b for a, b in zip(s1, scores)), (s1, scores)      # the arg-max alone is worse
    for path in ("heatmaps", "fused", "loader"):
        got, grep = pipeline.estimate_poses(*args, candidates_path=path, **kw)
        assert _same_poses(got, poses), path
        assert np.array_equal(grep.used, rep.used) and np.array_equal(grep.rescued, rep.rescued), path
        assert np.array_equal(grep.raw.view(np.int64), rep.raw.view(np.int64)), path
    # an invalid box behind the loader: on_fail applies, the report row is that of device_loader=True (status 1, n = 0), no
    # keypoint of that image entered a solve; the other images keep their poses
    boxes = [list(b) for b in sc["bboxes"]]
    boxes[1] = [500, 500, 500, 500]
    bad_args = (net, frames, boxes, sc["kp3d"], sc["K"])
    got, grep = pipeline.estimate_poses(*bad_args, candidates_path="loader", **kw)
    assert np.isnan(got[1][0]).all() and np.isnan(got[1][1]).all() and grep.status[1] == 1 and grep.n[1] == 0
    assert (grep.used[1] == -1).all() and not grep.rescued[1]
    keep = [0, 2, 3]
    assert _same_poses([got[i] for i in keep], [poses[i] for i in keep])
    assert np.array_equal(grep.used[keep], rep.used[keep]) and grep.rescued[keep].all()
    with pytest.raises(pipeline.PoseFailure, match=r"\[1\]"):
        pipeline.estimate_poses(*bad_args, candidates_path="loader", **dict(kw, on_fail="raise"))
