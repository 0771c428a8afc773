"""The refined candidates in the fused forward and behind the device loader on the GPU (include/esahrnet.h
esahrnet_forward_keypoints_candidates_refined, esahrnet_frames_keypoints_candidates_refined; net.candidates(refine=...),
net.frames_to_candidates(refine=...), pipeline.candidate_poses(candidates_path="fused" / "loader")).

Every comparison is bits against a chain of entries the stand-alone decoders already have: esahrnet_forward (net(x)) followed by
esahrnet_keypoints_candidates_refined (inference.heatmaps_to_candidates(refine=...)), crops.crop_batch in front of them for the
loader, pipeline.candidate_poses' heat-map path for the poses.  No tolerance anywhere.

The networks are the narrowest the other GPU tests use, with the fixtures' synthetic weights on random crops (noisy maps with many
local maxima); crops of 64 x 64 (the one-sweep search) and 18 x 34 / 34 x 18 (the multi-sweep search, planes narrower than the
13 x 13 fit window's reach and the refiners' guard band); the blob network (an output layer that reads the crop) gives planes with
two real blobs each; the pipeline tests draw the wrong-blob scene of tests/test_gpu_candidates_forward.py as frames."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_crops_pipeline as TCP  # noqa: E402  (its scene: BOXES)
import test_gpu_candidates_forward as TCF  # noqa: E402  (the wrong-blob scene as frames, the loader's scene)

pytestmark = pytest.mark.gpu

NETS = {"seg_hrnet": (3, 32, (8, 16, 32, 64)), "seg_hrnet2": (1, 11, (8, 16, 32, 64)), "seg_hrnet3": (1, 30, (16, 16, 32, 64))}
PRECISIONS = {"seg_hrnet": ("fp32", "bf16x3", "bf16", "fp16"), "seg_hrnet2": ("fp32", "bf16x3", "bf16", "fp16"),
              "seg_hrnet3": ("fp32", "bf16x3", "bf16")}
CASES = [(n, p) for n in NETS for p in PRECISIONS[n]]
# (n, H, W) -> the (M, r) run there: M = 1, 3, 4 with r = 6, and r = 2 on the narrow plane
SHAPES = {(3, 64, 64): ((1, 6), (3, 6), (4, 6)), (3, 18, 34): ((1, 6), (3, 6), (4, 2), (3, 2)), (3, 34, 18): ((3, 6), (4, 6))}
REFINES = ("get_final", "get_final2", "gaussfit")
# the keywords that ask for every output a decoder writes, and the names of what then follows (cand, cidx)
ASK = {"get_final": {}, "get_final2": dict(return_hessian=True),
       "gaussfit": dict(return_fit=True, return_hessian=True, return_cov=True, cov_floor=1e-6)}
OUTS = {"get_final": (), "get_final2": ("hess",), "gaussfit": ("fit", "status", "hess", "cov", "info")}


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


def _build(env, name, precision="fp32", seed=53, gain=0.5, edit=None):
    cin, k, w = NETS[name]
    net = env[name].get_seg_model(env["config"].make_config(widths=w), precision=precision)
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=seed, gain=gain)
    if edit:
        edit(sd)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


def _bits(a, b):
    """Bit-identical tensors: the same NaN mask, the same bits."""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point() and not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return torch.equal(a.view({4: torch.int32, 8: torch.int64}[a.element_size()]), b.view({4: torch.int32, 8: torch.int64}[a.element_size()]))


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert _bits(g, w), (what, i)


def _chain(env, heat, M, r, refine):
    """esahrnet_keypoints_candidates_refined on heat-maps in caller memory: (cand, cidx, *OUTS[refine])."""
    out = env["inference"].heatmaps_to_candidates(heat, M, r, return_index=True, refine=refine, **ASK[refine])
    assert len(out) == 2 + len(OUTS[refine])
    return out


class Seen:
    """What the compared slots held, counted on the two-call chain's outputs: the comparisons are not vacuous if every count is > 0."""

    def __init__(self):
        self.accepted = self.rejected = self.none = self.hess_finite = self.hess_nan = self.runner_up = 0

    def add(self, refine, out):
        cand = out[0]
        self.runner_up += int(torch.isfinite(cand[:, :, 1:, :2]).all(-1).sum())
        named = dict(zip(OUTS[refine], out[2:]))
        if refine == "gaussfit":
            st = named["status"]
            self.accepted += int((st == 0).sum())
            self.rejected += int((st > 0).sum())
            self.none += int((st == -1).sum())
        if refine == "get_final2":
            fin = torch.isfinite(named["hess"]).all(-1)
            self.hess_finite += int(fin.sum())
            self.hess_nan += int(torch.isnan(named["hess"]).all(-1).sum())

    def __repr__(self):
        return (f"accepted fits {self.accepted}, rejected {self.rejected}, slots without a candidate {self.none}, finite Hessian rows "
                f"{self.hess_finite}, NaN rows {self.hess_nan}, finite runner-ups {self.runner_up}")

    def complete(self):
        return min(self.accepted, self.rejected, self.hess_finite, self.hess_nan, self.runner_up) > 0


def _check(env, net, x, mr, seen=None):
    """Every form of the fused call against the chain, for the three decoders."""
    with torch.no_grad():
        heat = net(x)
        for M, r in mr:
            plain = net.candidates(x, M, r, return_index=True)                      # esahrnet_forward_keypoints_candidates
            for refine in REFINES:
                want = _chain(env, heat, M, r, refine)
                got = net.candidates(x, M, r, return_index=True, refine=refine, **ASK[refine])
                torch.cuda.synchronize()
                _same(got, want, (M, r, refine))
                _same(got[:2], plain[:2] if refine == "get_final" else (got[0], plain[1]), (M, r, refine, "the search"))
                assert _bits(got[0][..., 2], plain[0][..., 2]), (M, r, refine)       # the peak column: the raw value at the pixel
                # without the index the pixels stay in the workspace: the same other outputs
                _same(net.candidates(x, M, r, refine=refine, **ASK[refine]) if ASK[refine] else
                      (net.candidates(x, M, r, refine=refine),), (want[0], *want[2:]), (M, r, refine, "no index"))
                if seen is not None:
                    seen.add(refine, want)
            # fewer outputs asked for: the bits of the ones that are
            w2 = env["inference"].heatmaps_to_candidates(heat, M, r, refine="get_final2")
            assert _bits(net.candidates(x, M, r, refine="get_final2"), w2), (M, r)
            w3 = env["inference"].heatmaps_to_candidates(heat, M, r, refine="gaussfit", return_hessian=True)
            _same(net.candidates(x, M, r, refine="gaussfit", return_hessian=True), w3, (M, r, "gaussfit + hess"))


# ---- 1. every net, precision and output-layer form --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", CASES)
def test_equal_to_forward_plus_keypoints_candidates_refined(env, name, precision):
    net = _build(env, name, precision)
    seen = Seen()
    for i, (shape, mr) in enumerate(SHAPES.items()):
        x = env["synth"].make_crops(shape[0], NETS[name][0], *shape[1:], seed=360 + i).cuda()
        _check(env, net, x, mr, seen)
    print(name, precision, seen)
    assert seen.runner_up > 0


@pytest.mark.parametrize("name,precision", [("seg_hrnet2", "bf16x3"), ("seg_hrnet", "bf16")])
def test_valu_output_layer_on_a_matrix_core_precision(env, monkeypatch, name, precision):
    monkeypatch.setenv("ESAHRNET_FINAL_VALU", "1")
    net = _build(env, name, precision)
    for i, (shape, mr) in enumerate(list(SHAPES.items())[:2]):
        x = env["synth"].make_crops(shape[0], NETS[name][0], *shape[1:], seed=370 + i).cuda()
        _check(env, net, x, mr[1:3])


def _blob_edit(sd):
    """seg_hrnet2 whose heat-map j is (0.5 + j / K) * the crop + a small bias: the output layer reads the raw crop alone."""
    w = sd["output_layer.0.weight"]
    k = w.shape[0]
    w.zero_()
    for j in range(k):
        w[j, k, 1, 1] = 0.5 + j / k
    sd["output_layer.0.bias"] = torch.linspace(0.01, 0.1, k)


def _blob_crops(shape):
    """Crops with two Gaussian blobs each, amplitudes 1.0 and 0.7, well apart and off the border where the plane has the room."""
    n, hh, ww = shape
    yy, xx = np.mgrid[0:hh, 0:ww].astype(np.float64)
    x = np.zeros((n, 1, hh, ww), np.float32)
    for i in range(n):
        c1 = (0.3 * ww + 1.3 * i + 0.37, 0.45 * hh + 0.9 * i + 0.21)
        c2 = (0.75 * ww - 1.1 * i + 0.64, 0.55 * hh - 0.7 * i + 0.83)
        for (cx, cy), amp, s in ((c1, 1.0, 2.2), (c2, 0.7, 1.9)):
            x[i, 0] += (amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))).astype(np.float32)
    return torch.from_numpy(x)


def test_the_compared_slots_hold_every_kind_of_result(env):
    """On the chain's outputs (esahrnet_forward + esahrnet_keypoints_candidates_refined): accepted and rejected fits, finite and
    NaN Hessian rows, runner-ups with finite coordinates, over the blob network's planes and a random-weight network's; the fused
    call has their bits on exactly these inputs."""
    seen = Seen()
    net = _build(env, "seg_hrnet2", "fp32", edit=_blob_edit)
    for shape, mr in SHAPES.items():
        _check(env, net, _blob_crops(shape).cuda(), mr, seen)
    print("blob network:", seen)
    blob = (seen.accepted, seen.hess_finite, seen.runner_up)
    assert min(blob) > 0, seen                     # real blobs: fits that are accepted, steps that are taken, a second blob found
    net = _build(env, "seg_hrnet2", "fp32")
    for i, (shape, mr) in enumerate(SHAPES.items()):
        _check(env, net, env["synth"].make_crops(shape[0], 1, *shape[1:], seed=360 + i).cuda(), mr, seen)
    print("with the random-weight network:", seen)
    assert seen.complete(), seen


# ---- 2. batch invariance and graph replay -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_a_crop_alone_against_the_same_crop_in_a_batch_of_three(env, name):
    net = _build(env, name, "fp32")
    for shape in ((3, 64, 64), (3, 18, 34)):
        x = env["synth"].make_crops(3, 1, *shape[1:], seed=5).cuda()
        with torch.no_grad():
            for refine in ("get_final2", "gaussfit"):
                full = net.candidates(x, 3, 6, return_index=True, refine=refine, **ASK[refine])
                for i in range(3):
                    one = net.candidates(x[i:i + 1], 3, 6, return_index=True, refine=refine, **ASK[refine])
                    _same([t[0] for t in one], [t[i] for t in full], (shape, refine, i))


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_graph_replay(env, name):
    net = _build(env, name, "fp32")
    xs = [env["synth"].make_crops(3, 1, 64, 64, seed=s).cuda() for s in (2, 3, 4)]
    for refine in ("get_final2", "gaussfit"):
        x = xs[0].clone()
        call = lambda t: net.candidates(t, 3, 6, return_index=True, refine=refine, **ASK[refine])       # noqa: E731
        with torch.no_grad():
            refs = [[t.clone() for t in call(xi)] for xi in xs]
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                call(x)
            torch.cuda.current_stream().wait_stream(s)
            gph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gph):
                out = call(x)
            for i in (1, 2):                                    # replayed twice, each time on another input
                x.copy_(xs[i])
                gph.replay()
                torch.cuda.synchronize()
                _same(out, refs[i], (refine, i))
            assert not _bits(refs[1][0], refs[2][0])


# ---- 3. the entry on buffers of the test's own: outputs written whole, the workspace ---------------------------------------------
WRITES = {0: ("cand", "cidx", "status"), 1: ("cand", "cidx", "hess", "status"), 2: ("cand", "cidx", "hess", "fit", "status", "cov", "info")}
KINDS = {"cand": (torch.float32, (3,)), "cidx": (torch.int32, ()), "status": (torch.int32, ()), "hess": (torch.float64, (3,)),
         "fit": (torch.float64, (8,)), "cov": (torch.float64, (3,)), "info": (torch.float64, (3,))}


def _raw_call(env, net, x, M, r, dec, ws_fill=None, ws_short=0, skip=()):
    """esahrnet_forward_keypoints_candidates_refined with every output decoder `dec` writes but those in `skip`, pre-filled with
    0xA5: -> (rc, outputs by name)."""
    lib, L = env["lib"], env["L"]
    n, _, hh, ww = x.shape
    k = net.num_keypoints
    h = net._rt._handle_for(net, x.device)
    need, base, at = C.c_size_t(), C.c_size_t(), C.c_size_t()
    L.check(lib.esahrnet_keypoints_candidates_refined_forward_workspace_bytes(h, n, hh, ww, dec, C.byref(need)))
    L.check(lib.esahrnet_keypoints_candidates_forward_workspace_bytes(h, n, hh, ww, C.byref(base)))
    L.check(lib.esahrnet_keypoints_at_workspace_bytes(n, k, hh, ww, dec, C.byref(at)))
    assert need.value == base.value + ((n * k * 4 * 4 + 255) & ~255) + at.value       # the stated formula, on a committed handle
    ws = torch.zeros(need.value + 512, dtype=torch.uint8, device="cuda")
    if ws_fill == "nan":
        ws[:(ws.numel() // 4) * 4].view(torch.float32).fill_(float("nan"))
    elif ws_fill is not None:
        ws.fill_(ws_fill)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    o = {}
    for name in WRITES[dec]:
        if name not in skip:
            dt, tail = KINDS[name]
            o[name] = torch.empty((n, k, M, *tail), dtype=dt, device="cuda")
            o[name].view(torch.uint8).fill_(0xA5)
    p = lambda name: o[name].data_ptr() if name in o else None          # noqa: E731
    rc = lib.esahrnet_forward_keypoints_candidates_refined(h, x.data_ptr(), n, hh, ww, M, r, dec, p("cand"), p("cidx"), p("hess"),
                                                           p("fit"), p("status"), p("cov"), p("info"), 1e-6, wp,
                                                           need.value - ws_short, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, o


def _untouched(t):
    return bool((t.view(torch.uint8) == 0xA5).all())


@pytest.mark.parametrize("name,precision", [("seg_hrnet2", "fp32"), ("seg_hrnet2", "bf16x3"), ("seg_hrnet3", "fp32")])
def test_outputs_are_written_whole_whatever_the_workspace_held(env, name, precision):
    net = _build(env, name, precision)
    err = env["lib"].esahrnet_last_error
    for shape in ((3, 64, 64), (3, 18, 34)):
        x = env["synth"].make_crops(3, 1, *shape[1:], seed=4).cuda()
        M, r = (4, 6) if shape[1] == 64 else (3, 2)
        with torch.no_grad():
            heat = net(x)
            plain = net.candidates(x, M, r, return_index=True)
        for dec, refine in enumerate(REFINES):
            want = dict(zip(("cand", "cidx") + OUTS[refine], _chain(env, heat, M, r, refine)))
            for ws_fill in (None, "nan", 0xFF):
                rc, o = _raw_call(env, net, x, M, r, dec, ws_fill)
                assert rc == 0, err()
                for nm, t in o.items():             # every element: the pre-filled 0xA5 is gone wherever the chain wrote a value
                    if nm in want:
                        assert _bits(t, want[nm]), (shape, dec, ws_fill, nm)
                # status with decoders 0 and 1: 0 where there is a candidate, -1 where there is none
                if dec < 2:
                    assert torch.equal(o["status"] == -1, want["cidx"] == -1) and torch.equal(o["status"] == 0, want["cidx"] >= 0)
            # decoder 0: the bits of esahrnet_forward_keypoints_candidates, with and without a status
            if dec == 0:
                rc, o = _raw_call(env, net, x, M, r, 0, 0xFF, skip=("status",))
                assert rc == 0 and _bits(o["cand"], plain[0]) and torch.equal(o["cidx"], plain[1])
                rc, o = _raw_call(env, net, x, M, r, 0, 0xFF, skip=("status", "cidx"))
                assert rc == 0 and _bits(o["cand"], plain[0])
            # cidx_dev = NULL: the same other outputs
            rc, o = _raw_call(env, net, x, M, r, dec, 0xFF, skip=("cidx",))
            assert rc == 0, err()
            for nm, t in o.items():
                if nm in want:
                    assert _bits(t, want[nm]), (shape, dec, "cidx_dev NULL", nm)
            # optional outputs left out: the bits of the ones that are asked for
            if dec == 2:
                rc, o = _raw_call(env, net, x, M, r, 2, "nan", skip=("cidx", "fit", "cov", "info"))
                assert rc == 0 and _bits(o["cand"], want["cand"]) and _bits(o["hess"], want["hess"]) and torch.equal(o["status"], want["status"])
            # a workspace one byte short of the query: refused, nothing enqueued, the outputs as pre-filled
            rc, o = _raw_call(env, net, x, M, r, dec, ws_short=1)
            assert rc != 0 and b"too small" in err()
            assert all(_untouched(t) for t in o.values())


# ---- 4. the loader in front of it -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_loader_equals_crop_batch_then_candidates(env, name):
    """Gray frames, one val box per frame: what crops.crop_batch and net.candidates(refine=...) give, bit for bit."""
    net = _build(env, name, "fp32", gain=1.0)
    frames = TCF._frames(env, "frames", 3)
    boxes_in = [TCP.BOXES[0], TCP.BOXES[1], TCP.BOXES[2]]
    with torch.no_grad():
        x, rboxes, rrates = env["crops"].crop_batch(frames, boxes_in, 64)
        for refine in REFINES:
            want = net.candidates(x, 3, 6, return_index=True, refine=refine, **ASK[refine])
            got = net.frames_to_candidates(frames, boxes_in, scale=64, candidates=3, nms_radius=6, refine=refine, **ASK[refine])
            torch.cuda.synchronize()
            cand, boxes, rates, valid = got[:4]
            assert valid.tolist() == [1, 1, 1] and _bits(cand, want[0])
            _same(got[4:], want[2:], (refine, "the decoder's outputs"))
            assert boxes.tolist() == [[int(v) for v in b] for b in rboxes] and rates.tolist() == [float(r) for r in rrates]
            # fewer outputs asked for: a shorter tuple of the same tensors' bits
            if refine == "gaussfit":
                four = net.frames_to_candidates(frames, boxes_in, scale=64, candidates=3, nms_radius=6, refine=refine)
                assert len(four) == 4 and _bits(four[0], want[0])
                five = net.frames_to_candidates(frames, boxes_in, scale=64, candidates=3, nms_radius=6, refine=refine, return_hessian=True)
                assert len(five) == 5 and _bits(five[0], want[0]) and _bits(five[4], want[4])


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
@pytest.mark.parametrize("refine,cov", [("get_final2", False), ("gaussfit", False), ("gaussfit", True)])
def test_loader_with_a_frame_index_and_invalid_crops(env, name, refine, cov):
    inf, crops = env["inference"], env["crops"]
    net = _build(env, name, "fp32", gain=1.0)
    frames = TCF._frames(env, "frames", 2)
    M, k = 3, net.num_keypoints
    ask = dict(ASK[refine], return_cov=cov) if refine == "gaussfit" else ASK[refine]
    with torch.no_grad():
        x, rboxes, rrates, rvalid = crops.crop_batch_device(frames, TCF.SCENE_BOXES, frame_idx=TCF.SCENE_FIDX, scale=64)
        want = net.candidates(x, M, 6, return_index=True, refine=refine, **ask)
        out = net._loader(inf.LoaderRequest(refine, (M, 6), 1e-6 if cov else None), frames, TCF.SCENE_BOXES, TCF.SCENE_FIDX, 64, "val",
                          None, 0.229, None)
    torch.cuda.synchronize()
    cand, boxes, rates, valid, cidx = (out[n] for n in ("cand", "boxes", "rates", "valid", "cidx"))
    (packed, _), = out.records.values()
    assert valid.tolist() == TCF.SCENE_VALID == rvalid.tolist() and _bits(boxes, rboxes) and torch.equal(rates, rrates)
    good, bad = [i for i, v in enumerate(TCF.SCENE_VALID) if v], [i for i, v in enumerate(TCF.SCENE_VALID) if not v]
    gauss = refine == "gaussfit"
    fields = inf.record_fields(k, "candidates_refined", gauss, cov, M)
    names = (["cand_fit", "cand_status"] if gauss else []) + ["cand_hess"] + (["cand_cov", "cand_info"] if cov else [])
    assert len(out.views) == 5 + len(names) and list(out.records) == ["candidates_refined"]
    got = dict({n: out[n] for n in names}, cand=cand, cidx=cidx)
    ref = dict(zip(("cand", "cidx") + tuple({"fit": "cand_fit", "status": "cand_status", "hess": "cand_hess", "cov": "cand_cov",
                                             "info": "cand_info"}[n] for n in OUTS[refine] if cov or n not in ("cov", "info")), want))
    assert set(ref) == set(got)
    for nm, t in got.items():
        # two boxes on frame 0 and two on frame 1; the rows beside the invalid ones are what the parts give
        assert _bits(t[good], ref[nm][good]), nm
        if t.is_floating_point():
            assert bool(torch.isnan(t[bad]).all()), nm              # NaN in cand and in every f64 output
        else:
            assert bool((t[bad] == -1).all()), nm                   # -1 in cidx and status
    # the packed buffer: every output is the view that the record's description names
    lay = inf.packed_layout(5, k, gauss, cov, M, kind="candidates_refined")
    assert packed.dtype == torch.uint8 and packed.numel() == lay["total"][1] == 5 * sum(b for _, b in fields)
    views = dict(got, rates=rates, boxes=boxes, valid=valid)
    assert set(views) == {n for n, _ in fields}
    for nm, t in views.items():
        off, nbytes = lay[nm]
        assert t.data_ptr() == packed.data_ptr() + off and t.numel() * t.element_size() == nbytes and t.is_contiguous(), nm
    assert cand.shape == (5, k, M, 3) and got["cand_hess"].shape == (5, k, M, 3) and got["cand_hess"].dtype == torch.float64


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------
def _pattern_net(env, patterns):
    """TCF._pattern_net at this file's widths: heat-map j = 16 + the crop correlated with pattern j."""
    k = len(patterns)
    net = env["seg_hrnet2"].get_seg_model(env["config"].make_config(widths=NETS["seg_hrnet2"][2]), precision="fp32")
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=53, gain=0.5)
    w = sd["output_layer.0.weight"]
    assert w.shape == (k, k + 1, 3, 3)
    w.zero_()
    w[:, k] = torch.from_numpy(patterns.astype(np.float32))
    sd["output_layer.0.bias"] = torch.full((k,), 16.0)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval()


@pytest.fixture(scope="module")
def scene(env):
    sc = TCF._wrong_blob_frames(env)
    return sc, _pattern_net(env, sc["patterns"]), torch.from_numpy(sc["frames"]).cuda()


def _same_report(a, b):
    return (np.array_equal(a.used, b.used) and np.array_equal(a.rescued, b.rescued) and
            np.array_equal(a.raw.view(np.int64), b.raw.view(np.int64)))


@pytest.mark.parametrize("refine,weights,more", [("get_final2", "hessian", {}), ("gaussfit", "hessian", {}),
                                                 ("gaussfit", "covariance", dict(cov_floor=0))])
def test_candidate_poses_on_the_fused_path_and_behind_the_loader(env, scene, refine, weights, more):
    """The wrong-blob scene as frames and integer boxes: the fused path and the loader give the poses, the report rows, .used and
    .rescued of the heat-map path, bit for bit; an invalid box behind the loader follows on_fail."""
    pipeline = env["pipeline"]
    sc, net, frames = scene
    kw = dict(scale=TCF.CROP, on_fail="nan", thresh=0.0, min_k=8, candidates=3, nms_radius=6, return_report=True, refine=refine,
              weights=weights, **more)
    args = (net, frames, sc["bboxes"], sc["kp3d"], sc["K"])
    poses, rep = pipeline.candidate_poses(*args, **kw)
    again, rep2 = pipeline.candidate_poses(*args, candidates_path="heatmaps", **kw)
    assert TCF._same_poses(again, poses) and _same_report(rep2, rep)
    print(refine, weights, "status", rep.status.tolist(), "runner-ups used", int((rep.used > 0).sum()), "rescued", rep.rescued.tolist())
    for path in ("fused", "loader"):
        got, grep = pipeline.candidate_poses(*args, candidates_path=path, **kw)
        assert TCF._same_poses(got, poses), path
        assert _same_report(grep, rep), path
    boxes = [list(b) for b in sc["bboxes"]]
    boxes[1] = [500, 500, 500, 500]
    bad_args = (net, frames, boxes, sc["kp3d"], sc["K"])
    got, grep = pipeline.candidate_poses(*bad_args, candidates_path="loader", **kw)
    assert np.isnan(got[1][0]).all() and np.isnan(got[1][1]).all() and grep.status[1] == 1 and grep.n[1] == 0
    assert (grep.used[1] == -1).all() and not grep.rescued[1]
    keep = [0, 2, 3]
    assert TCF._same_poses([got[i] for i in keep], [poses[i] for i in keep])
    assert np.array_equal(grep.used[keep], rep.used[keep]) and np.array_equal(grep.rescued[keep], rep.rescued[keep])
    assert np.array_equal(grep.raw[keep].view(np.int64), rep.raw[keep].view(np.int64))
    if bool(np.isfinite(np.concatenate([np.r_[q, t] for i, (q, t) in enumerate(poses) if i != 1])).all()):
        with pytest.raises(pipeline.PoseFailure, match=r"\[1\]"):
            pipeline.candidate_poses(*bad_args, candidates_path="loader", **dict(kw, on_fail="raise"))


def test_get_final_with_peak_weights_is_estimate_poses_on_each_path(env, scene):
    pipeline = env["pipeline"]
    sc, net, frames = scene
    kw = dict(scale=TCF.CROP, on_fail="nan", thresh=0.0, min_k=8, candidates=3, nms_radius=6, return_report=True)
    args = (net, frames, sc["bboxes"], sc["kp3d"], sc["K"])
    for path in ("heatmaps", "fused", "loader"):
        want, wrep = pipeline.estimate_poses(*args, candidates_path=path, **kw)
        got, grep = pipeline.candidate_poses(*args, candidates_path=path, refine="get_final", weights="peak", **kw)
        assert TCF._same_poses(got, want) and _same_report(grep, wrep), path
        assert all(np.isfinite(q).all() and np.isfinite(t).all() for q, t in got) and (grep.used > 0).any() and grep.rescued.all(), path
    # get_final2 under peak weights behind the loader: the refined record without a weight taken from it
    want, wrep = pipeline.candidate_poses(*args, refine="get_final2", weights="peak", **kw)
    for path in ("fused", "loader"):
        got, grep = pipeline.candidate_poses(*args, candidates_path=path, refine="get_final2", weights="peak", **kw)
        assert TCF._same_poses(got, want) and _same_report(grep, wrep), path
    # frame_idx and a rule belong to the loader, which takes them
    fidx = list(range(len(sc["bboxes"])))
    want, _ = pipeline.candidate_poses(*args, candidates_path="loader", **kw)
    got, _ = pipeline.candidate_poses(*args, candidates_path="loader", frame_idx=fidx, **kw)
    assert TCF._same_poses(got, want)
