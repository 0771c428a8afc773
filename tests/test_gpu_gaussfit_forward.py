"""net(x, output="keypoints", refine="gaussfit") and net.keypoints_gaussfit(x) run esahrnet_forward_keypoints_gaussfit
(include/esahrnet.h): kp, idx, fit, status and hess bit-identical to esahrnet_forward + esahrnet_keypoints_gaussfit (net(x)
followed by inference.gaussfit_keypoints) for every network, precision and output-layer form, at shapes that are not multiples
of any tile, on blobs with a known centre, with ties and NaN, batch-invariant, in a graph, through DataParallel, whatever the
outputs and the workspace held on entry; and the loader in front of it (esahrnet_frames_keypoints_gaussfit) through
frames_to_keypoints, frames_to_correspondences and pipeline.estimate_poses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gaussfit_ref as G  # noqa: E402
import test_crops_pipeline as TCP  # noqa: E402  (its scene: BOXES)

pytestmark = pytest.mark.gpu

NETS = {"seg_hrnet": (3, 32, (16, 32, 64, 128)), "seg_hrnet2": (1, 11, (16, 32, 64, 128)), "seg_hrnet3": (1, 30, (16, 16, 32, 64))}
PRECISIONS = ["fp32", "bf16x3", "bf16"]
CASES = [(n, p) for n in NETS for p in PRECISIONS] + [("seg_hrnet", "fp16"), ("seg_hrnet2", "fp16")]
SHAPES = {0: [(2, 48, 80), (2, 18, 34), (1, 104, 72), (3, 16, 16)], 1: [(2, 48, 80), (3, 34, 18), (1, 104, 72), (2, 64, 64)]}
W48 = (48, 96, 192, 384)
# (cx, cy, sigma_x, sigma_y, theta) in a 48 x 80 crop: an interior blob on no seam, windows clipped left, bottom-right and to a
# corner, and a peak on the 32-column / 8-row tile seams of final_kernel
BLOBS = [(40.3, 24.6, 2.0, 1.6, 0.7), (3.4, 20.2, 2.0, 2.0, 0.0), (76.8, 44.1, 1.5, 2.5, 0.4), (31.6, 7.5, 2.5, 1.5, 1.1),
         (0.4, 0.3, 2.0, 2.0, 0.0)]


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


def _build(env, name, precision="fp32", widths=None, seed=53, gain=0.5, edit=None):
    cin, k, w = NETS[name]
    net = env[name].get_seg_model(env["config"].make_config(widths=widths or w), precision=precision)
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=seed, gain=gain)
    if edit:
        edit(sd)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


def _bits(a, b):
    """Bit-identical tensors: the same NaN mask, the same bits."""
    a, b = a.contiguous(), b.contiguous()
    it = {4: torch.int32, 8: torch.int64}[a.element_size()]
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point() and not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return torch.equal(a.view(it), b.view(it))


def _reference(env, net, x):
    """esahrnet_forward + esahrnet_keypoints_gaussfit: (kp, fit, status, hess, idx) and the heat-maps."""
    with torch.no_grad():
        heat = net(x)
        return env["inference"]._gaussfit(heat, True), heat


def _check(env, net, x):
    """Every Python form of the fused call against the reference; -> (reference tuple, heat)."""
    (rkp, rfit, rstatus, rhess, ridx), heat = _reference(env, net, x)
    with torch.no_grad():
        kp, fit, status, hess = net.keypoints_gaussfit(x, return_fit=True)
        kp3, status3, hess3 = net.keypoints_gaussfit(x)
        kp2, idx = net(x, output="keypoints+index", refine="gaussfit")
        kp1 = net(x, output="keypoints", refine="gaussfit")
        kp0, hess0 = env["inference"].heatmaps_to_keypoints(heat, refine="gaussfit", return_hessian=True)
    torch.cuda.synchronize()
    assert kp.shape == (x.shape[0], net.num_keypoints, 3) and idx.dtype == torch.int32 and status.dtype == torch.int32
    assert fit.shape == kp.shape[:2] + (8,) and fit.dtype == hess.dtype == torch.float64 and hess.shape == kp.shape
    assert torch.equal(idx, ridx) and torch.equal(status, rstatus) and torch.equal(status3, rstatus)
    assert _bits(kp, rkp) and _bits(fit, rfit) and _bits(hess, rhess)
    assert _bits(kp1, rkp) and _bits(kp2, rkp) and _bits(kp3, rkp) and _bits(hess3, rhess)
    assert _bits(kp0, rkp) and _bits(hess0, rhess)
    # what a status means, on the reference's outputs: an accepted fit is finite, a rejected one NaN with the get_final row
    ok = rstatus == 0
    assert bool(torch.isfinite(rfit[ok]).all()) and bool(torch.isnan(rfit[~ok]).all()) and bool(torch.isnan(rhess[~ok]).all())
    ex = env["inference"].heatmaps_to_keypoints(heat)
    assert _bits(rkp[~ok], ex[~ok]) and _bits(rkp[..., 2], ex[..., 2])
    return (rkp, rfit, rstatus, rhess, ridx), heat


def _counts(status):
    return np.bincount(status.cpu().numpy().ravel() + 1, minlength=5)[1:].tolist()


# ---- 1. every net, precision and output-layer form ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_equal_to_forward_plus_keypoints_gaussfit(env, name, precision):
    net, _ = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate(SHAPES[1 if name == "seg_hrnet3" else 0]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=160 + i).cuda()
        ref, _ = _check(env, net, x)
        print(name, precision, (n, hh, ww), "statuses 0..3", _counts(ref[2]))


def test_reference_path_takes_both_branches(env):
    """Over the nets of the parametrised set the reference accepts fits (status 0) and rejects fits (status 2: the get_final
    row): both ends of the kernels' last branch are compared above."""
    total = np.zeros(4, int)
    for name in NETS:
        net, _ = _build(env, name, "fp32")
        x = env["synth"].make_crops(2, NETS[name][0], 48, 80, seed=160).cuda()
        (_, _, status, _, _), _ = _reference(env, net, x)
        total += np.array(_counts(status))
        print(name, "statuses 0..3", _counts(status))
    assert total[0] > 0 and total[2] > 0, total.tolist()


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["seg_hrnet", "seg_hrnet2"])
def test_valu_output_layer_on_the_other_formats(env, monkeypatch, name, precision):
    """ESAHRNET_FINAL_VALU=1: the VALU form (final_gf_finish_kernel) reading split-bf16 and bf16 tensors."""
    monkeypatch.setenv("ESAHRNET_FINAL_VALU", "1")
    net, _ = _build(env, name, precision)
    for i, (n, hh, ww) in enumerate(SHAPES[0]):
        x = env["synth"].make_crops(n, NETS[name][0], hh, ww, seed=170 + i).cuda()
        _check(env, net, x)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_seg_hrnet3_w48(env, precision):
    net, _ = _build(env, "seg_hrnet3", precision, widths=W48, seed=7)
    for i, (n, hh, ww) in enumerate([(2, 64, 64), (1, 48, 80)]):
        x = env["synth"].make_crops(n, 1, hh, ww, seed=180 + i).cuda()
        _check(env, net, x)


# ---- 2. blobs with a known centre -----------------------------------------------------------------------------------------------
def _blob_edit(name):
    k = NETS[name][1]

    def edit(sd):
        w = sd["output_layer.0.weight"]
        w.zero_()
        for j in range(k):
            w[j, k, 1, 1] = 0.5 + j / k                   # the first channel behind the K up-sampled ones
        sd["output_layer.0.bias"] = torch.linspace(-0.1, 0.1, k)
        if name == "seg_hrnet3":                          # that channel is CBAM(skip) channel 0: 0.25 x
            sd["conv1.weight"].zero_()
            sd["conv1.weight"][0, 0, 1, 1] = 1.0
            for key in ("ca.fc.0.weight", "ca.fc.2.weight", "sa.conv1.weight"):
                sd[key].zero_()
    return edit


@pytest.mark.parametrize("name,precision", CASES)
def test_blobs_with_a_known_centre(env, name, precision):
    """Heat-map k of crop i is (0.5 + k / K) * (1 or 0.25) * blob_i + bias_k.  Bit-identity in every precision; in fp32 every
    plane is accepted and every centre within 1e-5 px of the truth (the f64 oracle with the numpy restatement: 3.9e-7 px, so
    the bound leaves 25 x for the GPU's fma order).  Elsewhere the figures are printed (a bf16-rounded crop: 4.1e-3 px on the
    CPU)."""
    net, _ = _build(env, name, precision, edit=_blob_edit(name))
    cin = NETS[name][0]
    x = torch.zeros(len(BLOBS), cin, 48, 80)
    for i, (cx, cy, sx, sy, th) in enumerate(BLOBS):
        x[i, 0] = torch.from_numpy(G.blob(48, 80, cx, cy, sx, sy, th)[0])
    (kp, fit, status, _, _), _ = _check(env, net, x.cuda())
    truth = torch.tensor([b[:2] for b in BLOBS], dtype=torch.float64)[:, None, :]
    err = (fit[..., 1:3].cpu() - truth).norm(dim=-1)
    ok = (status == 0).cpu()
    worst = float(err[ok].max()) if bool(ok.any()) else float("nan")
    print(name, precision, "statuses 0..3", _counts(status), "largest centre error of an accepted fit [px]", worst)
    if precision == "fp32":
        assert bool(ok.all()), _counts(status)
        assert worst <= 1e-5, worst
        assert float((kp[..., :2].cpu().double() - truth).norm(dim=-1).max()) <= 1e-5 + 80 * 2.0 ** -24     # kp is f32


# ---- 3. ties and values that are not finite -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_ties_and_nan(env, name, precision):
    net, sd = _build(env, name, precision)
    cin = NETS[name][0]
    x = env["synth"].make_crops(3, cin, 48, 80, seed=61)
    x[1, 0, 20:30, 33:40] = float("nan")                  # crop 1: NaN pixels
    x[2, 0, 5:9, 60:66] = float("inf")                    # crop 2: +inf pixels
    x = x.cuda()
    (kp, fit, status, hess, idx), heat = _check(env, net, x)
    assert torch.isnan(heat[1]).any() and torch.isfinite(heat[0]).all()
    nan_peak = torch.isnan(kp[..., 2])
    assert bool(nan_peak.any()) and bool((status[nan_peak] == 3).all())
    bad = status == 3
    assert bool(torch.isnan(fit[bad]).all()) and bool(torch.isnan(hess[bad]).all())
    # ties: zero output-layer weights -> every plane is its constant bias -> first index (0, 0), A = 0: status 2, the get_final row
    sd0 = {k: v.clone() for k, v in sd.items()}
    sd0["output_layer.0.weight"].zero_()
    net.load_state_dict(sd0)
    (kp0, fit0, status0, hess0, idx0), heat0 = _check(env, net, x[[0, 0]])      # (0 * inf is NaN: the +inf crop has no constant planes)
    assert bool((heat0 == heat0[:, :, :1, :1]).all())
    assert bool((idx0 == 0).all()) and bool((kp0[..., :2] == 0).all()) and bool((status0 == 2).all())
    assert bool(torch.isnan(fit0).all()) and bool(torch.isnan(hess0).all())


# ---- 4. batch invariance, graph capture, DataParallel -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_batch_invariance(env, name):
    net, _ = _build(env, name, "fp32")
    x = env["synth"].make_crops(6, 1, 48, 80, seed=5).cuda()
    perm = [4, 2, 0, 5, 1, 3]
    with torch.no_grad():
        full = net.keypoints_gaussfit(x, return_fit=True)
        shuf = net.keypoints_gaussfit(x[perm].contiguous(), return_fit=True)
        for a, b in zip(full, shuf):
            assert _bits(a[perm], b)
        for i in range(6):
            one = net.keypoints_gaussfit(x[i:i + 1], return_fit=True)
            assert all(_bits(a[0], b[i]) for a, b in zip(one, full)), i


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_graph_capture_and_data_parallel(env, name):
    net, _ = _build(env, name, "fp32")
    xs = [env["synth"].make_crops(4, 1, 64, 64, seed=s).cuda() for s in (2, 3, 4)]
    x = xs[0].clone()
    with torch.no_grad():
        refs = [[t.clone() for t in net.keypoints_gaussfit(xi, return_fit=True)] for xi in xs]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net.keypoints_gaussfit(x, return_fit=True)
        torch.cuda.current_stream().wait_stream(s)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            out = net.keypoints_gaussfit(x, return_fit=True)
        for i in (1, 2):                                    # replayed twice, each time on another input
            x.copy_(xs[i])
            gph.replay()
            torch.cuda.synchronize()
            assert all(_bits(a, b) for a, b in zip(out, refs[i])), i
        assert not _bits(refs[1][0], refs[2][0])
        dp = torch.nn.DataParallel(net, device_ids=[0])
        assert _bits(dp(xs[0], output="keypoints", refine="gaussfit"), refs[0][0])
        kp_dp, idx_dp = dp(xs[0], output="keypoints+index", refine="gaussfit")
        assert _bits(kp_dp, refs[0][0]) and idx_dp.dtype == torch.int32


# ---- 5. what the outputs and the workspace held on entry ----------------------------------------------------------------------
def _raw_call(env, net, x, out_fill, ws_fill=None, ws_short=0, ws_shift=0, null=()):
    """esahrnet_forward_keypoints_gaussfit on buffers of the test's own: -> (rc, (kp, idx, fit, status, hess))."""
    lib, L = env["lib"], env["L"]
    n, _, hh, ww = x.shape
    k = net.num_keypoints
    h = net._rt._handle_for(net, x.device)
    need = C.c_size_t()
    L.check(lib.esahrnet_keypoints_gaussfit_forward_workspace_bytes(h, n, hh, ww, C.byref(need)))
    ws = torch.empty(need.value + 512, dtype=torch.uint8, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    outs = dict(kp=torch.empty((n, k, 3), dtype=torch.float32, device="cuda"), idx=torch.empty((n, k), dtype=torch.int32, device="cuda"),
                fit=torch.empty((n, k, 8), dtype=torch.float64, device="cuda"), status=torch.empty((n, k), dtype=torch.int32, device="cuda"),
                hess=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"))
    for t in outs.values():
        t.view(torch.uint8).fill_(out_fill)
    ptr = {name: (None if name in null else t.data_ptr()) for name, t in outs.items()}
    rc = lib.esahrnet_forward_keypoints_gaussfit(h, x.data_ptr(), n, hh, ww, ptr["kp"], ptr["idx"], ptr["fit"], ptr["status"],
                                                 ptr["hess"], wp + ws_shift, need.value - ws_short,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, tuple(outs[n_] for n_ in ("kp", "idx", "fit", "status", "hess"))


@pytest.mark.parametrize("name,precision", [("seg_hrnet2", "fp32"), ("seg_hrnet2", "bf16x3"), ("seg_hrnet3", "fp32"), ("seg_hrnet3", "bf16x3")])
def test_outputs_and_workspace_contents_on_entry_do_not_matter(env, name, precision):
    net, _ = _build(env, name, precision)
    x = env["synth"].make_crops(2, 1, 48, 80, seed=4).cuda()
    (rkp, rfit, rstatus, rhess, ridx), _ = _reference(env, net, x)
    want = (rkp, ridx, rfit, rstatus, rhess)
    for out_fill, ws_fill in ((0xFF, None), (0x00, None), (0x00, 0xFF), (0xFF, 0xFF)):
        rc, got = _raw_call(env, net, x, out_fill, ws_fill)
        assert rc == 0, env["lib"].esahrnet_last_error()
        assert all(_bits(a, b) for a, b in zip(got, want)), (out_fill, ws_fill)
    # idx, fit and hess may be NULL: the others have the same bits and the NULL ones are not touched
    rc, got = _raw_call(env, net, x, 0xFF, 0xFF, null=("idx", "fit", "hess"))
    assert rc == 0 and _bits(got[0], rkp) and torch.equal(got[3], rstatus)
    assert all(bool((got[i].view(torch.uint8) == 0xFF).all()) for i in (1, 2, 4))
    # a workspace one 256-byte unit too small, or misaligned by 8: refused, nothing enqueued, the outputs as pre-filled
    for kw, word in ((dict(ws_short=256), b"too small"), (dict(ws_shift=8), b"aligned")):
        rc, got = _raw_call(env, net, x, 0xFF, **kw)
        assert rc != 0 and word in env["lib"].esahrnet_last_error(), kw
        assert all(bool((t.view(torch.uint8) == 0xFF).all()) for t in got), kw


# ---- 6. the loader in front of it --------------------------------------------------------------------------------------------
def _frames(env, name, n, seed=3):
    return torch.from_numpy(env["synth"].uniform(name, seed, (n, 1200, 1920), 0, 255.99).astype(np.uint8)).cuda()


SCENE_BOXES = [TCP.BOXES[0], TCP.BOXES[1], (500, 500, 500, 500), TCP.BOXES[2], TCP.BOXES[3]]      # position 2: an empty box
SCENE_FIDX = [0, 1, 0, 1, 2]                                                                     # position 4: no such frame
SCENE_VALID = [1, 1, 0, 1, 0]


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_loader_equals_its_parts(env, name):
    inf, crops = env["inference"], env["crops"]
    net, _ = _build(env, name, "fp32", gain=1.0)
    frames = _frames(env, "frames", 2)
    scale = 64
    kw = dict(frame_idx=SCENE_FIDX, scale=scale, refine="gaussfit")
    with torch.no_grad():
        x, rboxes, rrates, rvalid = crops.crop_batch_device(frames, SCENE_BOXES, frame_idx=SCENE_FIDX, scale=scale)
        rkp, ridx = net(x, output="keypoints+index", refine="gaussfit")
        _, rfit, rstatus, rhess = net.keypoints_gaussfit(x, return_fit=True)
        r = net._loader(inf.LoaderRequest("gaussfit"), frames, SCENE_BOXES, SCENE_FIDX, scale, "val", None, 0.229, None)
        kp, boxes, rates, valid, idx, fit, status, hess = (r[n] for n in ("kp", "boxes", "rates", "valid", "idx", "fit", "status", "hess"))
        (packed, _), = r.records.values()
        four = net.frames_to_keypoints(frames, SCENE_BOXES, **kw)
    torch.cuda.synchronize()
    assert len(four) == 4 and _bits(four[0], kp) and _bits(four[1], boxes) and _bits(four[2], rates) and _bits(four[3], valid)
    assert valid.tolist() == SCENE_VALID == rvalid.tolist() and _bits(boxes, rboxes) and _bits(rates, rrates)
    good, bad = [i for i, v in enumerate(SCENE_VALID) if v], [i for i, v in enumerate(SCENE_VALID) if not v]
    assert _bits(kp[good], rkp[good]) and torch.equal(idx[good], ridx[good]) and _bits(fit[good], rfit[good])
    assert torch.equal(status[good], rstatus[good]) and _bits(hess[good], rhess[good])
    assert bool(torch.isnan(kp[bad]).all()) and bool((idx[bad] == -1).all()) and bool((status[bad] == -1).all())
    assert bool(torch.isnan(fit[bad]).all()) and bool(torch.isnan(hess[bad]).all())
    assert packed.dtype == torch.uint8 and packed.numel() == inf.packed_layout(5, net.num_keypoints, True)["total"][1]
    print(name, "statuses -1..3", np.bincount(status.cpu().numpy().ravel() + 1, minlength=5).tolist())
    sel = dict(thresh=0.1, min_k=6)
    for w in ("peak", "hessian"):
        with torch.no_grad():
            out = net.frames_to_correspondences(frames, SCENE_BOXES, weights=w, **kw, **sel)
            parts = inf.keypoints_to_correspondences(kp, boxes, rates, valid, hess=hess if w == "hessian" else None, weights=w, **sel)
        torch.cuda.synchronize()
        assert len(out) == 8 and all(_bits(a, b) for a, b in zip(out[:4], parts)), w
        assert _bits(out[4], kp) and _bits(out[5], boxes) and _bits(out[6], rates) and _bits(out[7], valid)
        assert [out[0].tolist()[i] for i in bad] == [0, 0] and min(out[0].tolist()[i] for i in good) >= 6
        print(name, w, "count", out[0].tolist(), "points with a weight:", int((out[3].abs().sum(-1) > 0).sum()))


def test_loader_in_a_graph(env):
    net, _ = _build(env, "seg_hrnet2", "fp32", gain=1.0)
    f1, f2 = _frames(env, "frames", 2), _frames(env, "frames_b", 2, seed=9)
    fidx = torch.tensor(SCENE_FIDX, dtype=torch.int32, device="cuda")
    det = torch.tensor(SCENE_BOXES, dtype=torch.int32, device="cuda")
    frames = f1.clone()
    kw = dict(frame_idx=fidx, scale=64, refine="gaussfit", weights="hessian", thresh=0.1, min_k=6)
    with torch.no_grad():
        ref2 = [t.clone() for t in net.frames_to_correspondences(f2, det, **kw)]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net.frames_to_correspondences(frames, det, **kw)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = net.frames_to_correspondences(frames, det, **kw)
        frames.copy_(f2)
        g.replay()
        torch.cuda.synchronize()
    assert all(_bits(a, b) for a, b in zip(out, ref2))


def _same_poses(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(qa, np.float64).view(np.int64), np.asarray(qb, np.float64).view(np.int64)) and
                                    np.array_equal(np.asarray(ta, np.float64).view(np.int64), np.asarray(tb, np.float64).view(np.int64))
                                    for (qa, ta), (qb, tb) in zip(a, b))


def test_estimate_poses_with_the_gaussfit_decoder(env):
    pipeline, synth, inf, pnp = env["pipeline"], env["synth"], env["inference"], env["pnp"]
    net, _ = _build(env, "seg_hrnet2", "fp32", gain=1.0)
    n = 6
    scene = synth.make_scene(n, net.num_keypoints, seed=0)
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(n, 1200, 1920), dtype=np.uint8)).cuda()
    sel = dict(thresh=0.0, min_k=8)
    kw = dict(scale=64, on_fail="nan", refine="gaussfit", **sel)
    args = (net, frames, scene["bboxes"], scene["kp3d"], synth.ESA_CAMERA)
    host = pipeline.estimate_poses(*args, **kw)
    assert _same_poses(pipeline.estimate_poses(*args, keypoints_only=True, **kw), host)
    assert _same_poses(pipeline.estimate_poses(*args, device_loader=True, **kw), host)
    assert _same_poses(pipeline.estimate_poses(*args, device_select=True, **kw), host)          # "peak": pose for pose
    # the Hessian weights: the native solver on the record the host path builds from the loader's own outputs
    got = pipeline.estimate_poses(*args, device_select=True, weights="hessian", **kw)
    with torch.no_grad():
        r = net._loader(inf.LoaderRequest("gaussfit"), frames, scene["bboxes"], None, 64, "val", None, 0.229, None)
        kp, boxes, rates, valid, status, hess = (r[n] for n in ("kp", "boxes", "rates", "valid", "status", "hess"))
        count, order, pts, w = (t.cpu().numpy() for t in inf.keypoints_to_correspondences(kp, boxes, rates, valid, hess=hess,
                                                                                          weights="hessian", **sel))
    q, t = pnp.correspondences_to_pose_batch(pts, w, count, order, scene["kp3d"], np.asarray(synth.ESA_CAMERA, np.float64), 0)
    assert _same_poses(got, [(q[i], t[i]) for i in range(n)])
    print("statuses 0..3", _counts(status), "poses that are numbers:", sum(bool(np.isfinite(q_).all()) for q_, _ in got), "of", n)
