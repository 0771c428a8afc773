"""The candidates' device stage on the GPU (include/esahrnet.h esahrnet_correspondences_cand; net.frames_to_candidate_correspondences,
inference.candidates_to_correspondences, pipeline.candidate_poses(device_select=True, distributed=True)).

Every comparison is bit for bit: each quantity of the record is copied or computed by csrc/correspond.h in f64 without
contraction, and tests/candidate_correspond_ref.py restates it in numpy scalar operations.

  1. correspond_cand_kernel on crafted rows, no network: against the restatement for (m, K, M) = (1, 1, 1), (3, 11, 3), (2, 30, 2),
     (5, 32, 4), into outputs pre-filled with 0xFF; with M = 1 against esahrnet_correspondences; a crop alone against the same crop
     in the batch; one graph capture and replay; no scratch memory.
  2. through the network: net.frames_to_candidate_correspondences against net.frames_to_candidates followed by
     inference.candidates_to_correspondences, with a frame index, an empty box and a frame out of range.
  3. end to end: the wrong-blob scene as frames; candidate_poses(device_select=True) against candidates_path="loader"; an invalid
     box; distributed=True under nccl at world size 1."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import candidate_correspond_ref as R  # noqa: E402
import test_crops_pipeline as TCP  # noqa: E402  (its scene: BOXES)
import test_gpu_candidates_forward as TCF  # noqa: E402  (the wrong-blob scene as frames)
import test_gpu_candidates_refined_forward as TRF  # noqa: E402  (its nets)
import test_records_host as H  # noqa: E402  (the free port)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (3, 11, 3), (2, 30, 2), (5, 32, 4)]
PEAKS = np.array([0.1, 0.3, 0.5, 0.5, 0.5000001, 0.7, 0.7, 0.9], np.float32)      # ties, and values on both sides of thresh = 0.5
THRESH = 0.5


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, crops, inference, parallel, pipeline, pnp, seg_hrnet, seg_hrnet2, seg_hrnet3, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, crops=crops, inference=inference, parallel=parallel, pipeline=pipeline, pnp=pnp,
                synth=synth, seg_hrnet=seg_hrnet, seg_hrnet2=seg_hrnet2, seg_hrnet3=seg_hrnet3)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


# ---- 1. the kernel on crafted rows ----------------------------------------------------------------------------------------------
def crafted(m, K, M, nan_primary=False, finite_primary_xy=False):
    """cand f32 [m,K,M,3], hess f64 [m,K,M,3], crop_boxes int32 [m,4], rates f64 [m], valid int32 [m].  Peaks from PEAKS (equal
    peaks, peaks straddling THRESH); runner-up rows with NaN rows, +inf x, -inf y, NaN y and NaN peaks; a primary with an infinite
    coordinate (unless finite_primary_xy); the last keypoint's primary peak of crop 0 NaN when K > 1 or nan_primary; the middle crop
    of a batch of three or more invalid; Hessians with NaN, zero and indefinite ones (R.random_hessians)."""
    rng = np.random.default_rng(1000 * m + 10 * K + M)
    cand = np.empty((m, K, M, 3), np.float32)
    cand[..., :2] = rng.uniform(-4, 70, (m, K, M, 2))
    cand[..., 2] = rng.choice(PEAKS, (m, K, M))
    flat = cand.reshape(-1, M, 3)
    for i in range(len(flat)):
        for mm in range(1, M):
            what = (i * 3 + mm) % 9
            if what == 0:
                flat[i, mm] = np.nan                        # an absent runner-up
            elif what == 1:
                flat[i, mm, 0] = np.inf
            elif what == 2:
                flat[i, mm, 1] = -np.inf
            elif what == 3:
                flat[i, mm, 1] = np.nan
            elif what == 4:
                flat[i, mm, 2] = np.nan                     # a NaN peak on finite coordinates
    if not finite_primary_xy and K > 2:
        cand[0, 1, 0, 0] = np.inf
        cand[m - 1, 2, 0, 1] = np.nan
    if K > 1 or nan_primary:
        cand[0, K - 1, 0, 2] = np.nan
    hess = R.random_hessians(rng, cand)
    boxes = rng.integers(-50, 1500, (m, 4)).astype(np.int32)
    rates = rng.uniform(0.2, 3.0, m)
    valid = np.ones(m, np.int32)
    if m >= 3:
        valid[m // 2] = 0
    return dict(cand=cand, hess=hess, crop_boxes=boxes, rates=rates, valid=valid)


def selections(K):
    """(thresh, min_k): the threshold alone; min_k > K; min_k = 0 with nothing above the threshold; min_k inside."""
    return [(THRESH, 0), (THRESH, K + 3), (2.0, 0), (THRESH, (K + 1) // 2)]


def run(env, inp, thresh, min_k, mode, M=None, fill=0xFF):
    """esahrnet_correspondences_cand on the device, into outputs every byte of which holds `fill`: -> numpy dict of R.FIELDS."""
    cand = torch.from_numpy(inp["cand"] if M is None else np.ascontiguousarray(inp["cand"][:, :, :M])).cuda()
    hess = torch.from_numpy(inp["hess"] if M is None else np.ascontiguousarray(inp["hess"][:, :, :M])).cuda()
    m, K, mm = cand.shape[:3]
    boxes, rates, valid = (torch.from_numpy(inp[n]).cuda() for n in ("crop_boxes", "rates", "valid"))
    fields = env["inference"].record_fields(K, "candidate_correspondences", candidates=mm)
    packed = torch.full((m * sum(b for _, b in fields),), fill, dtype=torch.uint8, device="cuda")
    v = env["inference"].record_views(packed, m, K, fields)
    rc = env["lib"].esahrnet_correspondences_cand(cand.data_ptr(), hess.data_ptr() if mode else None, boxes.data_ptr(), rates.data_ptr(),
                                                  valid.data_ptr(), m, K, mm, float(thresh), int(min_k), mode, v["count"].data_ptr(),
                                                  v["order"].data_ptr(), v["cpts"].data_ptr(), v["cw"].data_ptr(), v["cpeak"].data_ptr(),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, env["lib"].esahrnet_last_error().decode()
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in v.items()}


def _equal(got, want, what):
    for n in R.FIELDS:
        assert R.same_bits(got[n], want[n]), (what, n)


@pytest.mark.parametrize("m,K,M", SHAPES)
def test_kernel_equals_the_restatement(env, m, K, M):
    seen = dict(count0_valid=0, min_k_over=0, ties=0, nan_primary=0, invalid=0, nan_pts=0, zero_w_mode1=0, swaps_of_order=0)
    for nan_primary in ((False, True) if K == 1 else (False,)):
        inp = crafted(m, K, M, nan_primary)
        for thresh, min_k in selections(K):
            for mode in (0, 1):
                got = run(env, inp, thresh, min_k, mode)
                want = R.record(inp["cand"], inp["hess"], inp["crop_boxes"], inp["rates"], inp["valid"], thresh, min_k, mode)
                _equal(got, want, (nan_primary, thresh, min_k, mode))
                ok = inp["valid"] != 0
                seen["count0_valid"] += int((got["count"][ok] == 0).sum())
                seen["min_k_over"] += int(min_k > K)
                seen["invalid"] += int((~ok).sum())
                seen["nan_pts"] += int(np.isnan(got["cpts"]).any(-1).sum())
                seen["swaps_of_order"] += int(any((np.diff(o[:c]) < 0).any() for o, c in zip(got["order"], got["count"])))
                if mode:
                    live = np.arange(K)[None, :, None] < got["count"][:, None, None]
                    seen["zero_w_mode1"] += int((live & np.isfinite(got["cpts"]).all(-1) & ~got["cw"].any(-1)).sum())
        peaks = inp["cand"][:, :, 0, 2]
        seen["ties"] += int(sum(len(p[~np.isnan(p)]) - len(np.unique(p[~np.isnan(p)])) for p in peaks))
        seen["nan_primary"] += int(np.isnan(peaks[inp["valid"] != 0]).sum())
    print((m, K, M), seen)
    assert seen["count0_valid"] > 0 and seen["min_k_over"] > 0                     # every shape: nothing above 2.0; min_k = K + 3
    assert seen["nan_primary"] > 0                                               # every shape, K = 1 through its own variant
    if K > 2:
        assert seen["ties"] > 0 and seen["swaps_of_order"] > 0 and seen["zero_w_mode1"] > 0
    if M > 1:
        assert seen["nan_pts"] > 0
    if m >= 3:
        assert seen["invalid"] > 0


@pytest.mark.parametrize("m,K,M", SHAPES)
def test_one_candidate_is_esahrnet_correspondences(env, m, K, M):
    """M = 1 (the shape's primaries): count, order, pts and w of esahrnet_correspondences on the same rows, modes 0 and 1."""
    inf = env["inference"]
    inp = crafted(m, K, M, finite_primary_xy=True)
    kp = torch.from_numpy(np.ascontiguousarray(inp["cand"][:, :, 0])).cuda()
    hess = torch.from_numpy(np.ascontiguousarray(inp["hess"][:, :, 0])).cuda()
    boxes, rates, valid = (torch.from_numpy(inp[n]).cuda() for n in ("crop_boxes", "rates", "valid"))
    for thresh, min_k in selections(K):
        for mode, weights in ((0, "peak"), (1, "hessian")):
            got = run(env, inp, thresh, min_k, mode, M=1)
            count, order, pts, w = inf.keypoints_to_correspondences(kp, boxes, rates, valid, hess if mode else None, thresh, min_k, weights)
            torch.cuda.synchronize()
            what = (thresh, min_k, mode)
            assert R.same_bits(got["count"], count.cpu().numpy()) and R.same_bits(got["order"], order.cpu().numpy()), what
            assert R.same_bits(got["cpts"][:, :, 0], pts.cpu().numpy()) and R.same_bits(got["cw"][:, :, 0], w.cpu().numpy()), what
            live = np.arange(K)[None] < got["count"][:, None]
            sel = np.take_along_axis(inp["cand"][:, :, 0, 2], np.maximum(got["order"], 0), 1)
            assert R.same_bits(got["cpeak"][:, :, 0], np.where(live, sel, np.float32(0)).astype(np.float32)), what


@pytest.mark.parametrize("m,K,M", [(3, 11, 3), (5, 32, 4)])
def test_a_crop_alone_is_the_crop_in_the_batch(env, m, K, M):
    inp = crafted(m, K, M)
    for mode in (0, 1):
        batch = run(env, inp, THRESH, 4, mode)
        for c in range(m):
            one = run(env, {n: a[c:c + 1] for n, a in inp.items()}, THRESH, 4, mode)
            for n in R.FIELDS:
                assert R.same_bits(one[n], batch[n][c:c + 1]), (mode, c, n)


def test_wrapper_and_graph_replay(env):
    """inference.candidates_to_correspondences gives the raw call's record; captured once and replayed on new inputs in the same
    buffers it gives theirs."""
    inf = env["inference"]
    a, b = crafted(5, 32, 4), crafted(5, 32, 4)
    b["cand"] = np.ascontiguousarray(a["cand"][::-1])                               # other rows behind the same pointers
    b["hess"] = np.ascontiguousarray(a["hess"][::-1])
    dev = {n: torch.from_numpy(t).cuda() for n, t in a.items()}
    args = lambda: (dev["cand"], dev["crop_boxes"], dev["rates"], dev["valid"], THRESH, 4, "hessian", dev["hess"])   # noqa: E731
    eager = inf.candidates_to_correspondences(*args())
    torch.cuda.synchronize()
    _equal(dict(zip(R.FIELDS, (t.cpu().numpy() for t in eager))), run(env, a, THRESH, 4, 1), "wrapper")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        inf.candidates_to_correspondences(*args())
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = inf.candidates_to_correspondences(*args())
    for n in ("cand", "hess"):
        dev[n].copy_(torch.from_numpy(b[n]))
    for t in cap:
        t.view(torch.uint8).fill_(0xFF)
    g.replay()
    torch.cuda.synchronize()
    _equal(dict(zip(R.FIELDS, (t.cpu().numpy() for t in cap))), run(env, b, THRESH, 4, 1), "replay")
    with pytest.raises(ValueError, match="hess must be"):
        inf.candidates_to_correspondences(dev["cand"], dev["crop_boxes"], dev["rates"], dev["valid"], weights="hessian")
    with pytest.raises(ValueError, match=r"float32 cuda tensor \[m, K, M, 3\]"):
        inf.candidates_to_correspondences(dev["cand"][:, :, 0], dev["crop_boxes"], dev["rates"], dev["valid"])


def test_the_kernel_uses_no_scratch_memory():
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    with open(b.USAGE) as f:
        usage = json.load(f)
    rows = {k: u for k, u in usage.items() if k.startswith("correspond.hip:") and "correspond_cand_kernel" in k}
    assert len(rows) == 1, sorted(usage)
    (u,) = rows.values()
    assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["lds"] == 0, u


# ---- 2. through the network ------------------------------------------------------------------------------------------------------
PAIRS = [("get_final", "peak", {}), ("get_final2", "hessian", {}), ("gaussfit", "hessian", {}), ("gaussfit", "covariance", dict(cov_floor=0))]
# five boxes on three frames: position 2 is an empty box, position 4 names a frame that is not there
NET_BOXES = [TCP.BOXES[0], TCP.BOXES[1], (500, 500, 500, 500), TCP.BOXES[2], TCP.BOXES[3]]
NET_FIDX = [0, 1, 0, 2, 3]
NET_VALID = [1, 1, 0, 1, 0]


@pytest.fixture(scope="module")
def frames3(env):
    return TCF._frames(env, "frames", 3)


@pytest.mark.parametrize("name", ["seg_hrnet2", "seg_hrnet3"])
def test_loader_equals_frames_to_candidates_then_the_stage(env, frames3, name):
    inf = env["inference"]
    net = TRF._build(env, name, "fp32", gain=1.0)
    k, M = net.num_keypoints, 3
    good = [i for i, v in enumerate(NET_VALID) if v]
    bad = [i for i, v in enumerate(NET_VALID) if not v]
    for refine, weights, more in PAIRS:
        ask = dict(return_hessian=weights == "hessian", return_cov=weights == "covariance", **more)
        with torch.no_grad():
            parts = net.frames_to_candidates(frames3, NET_BOXES, frame_idx=NET_FIDX, scale=64, candidates=M, nms_radius=6, refine=refine,
                                             **ask)
            cand, boxes, rates, valid = parts[:4]
            hess = parts[-1] if weights != "peak" else None                          # (return_cov: cov, info -- info weighs)
            assert valid.tolist() == NET_VALID
            prim = cand[good][:, :, 0, 2]
            sel = dict(thresh=float(prim.median()), min_k=4)                         # about half of the keypoints above it
            want = inf.candidates_to_correspondences(cand, boxes, rates, valid, weights=weights, hess=hess, **sel)
            got = net.frames_to_candidate_correspondences(frames3, NET_BOXES, frame_idx=NET_FIDX, scale=64, refine=refine, candidates=M,
                                                          nms_radius=6, weights=weights, **sel, **more)
            request = inf.LoaderRequest(refine, (M, 6), more.get("cov_floor", 1e-6) if weights == "covariance" else None,
                                        (sel["thresh"], sel["min_k"], weights))
            priv = net._loader(request, frames3, NET_BOXES, NET_FIDX, 64, "val", None, 0.229, None)
            # the good boxes alone: their rows must not feel the bad ones beside them
            alone = net.frames_to_candidate_correspondences(frames3, [NET_BOXES[i] for i in good], frame_idx=[NET_FIDX[i] for i in good],
                                                            scale=64, refine=refine, candidates=M, nms_radius=6, weights=weights, **sel,
                                                            **more)
        torch.cuda.synchronize()
        what = (name, refine, weights)
        assert len(got) == 9 and list(priv.records) == [request.second, request.main[0]]
        TRF._same(got[:5], want, what)
        TRF._same(got[5:], parts[:4], what)
        TRF._same([priv[n] for n in R.FIELDS + ("cand", "boxes", "rates", "valid")], got, what)
        cpts, cw, cpeak, count, order = got[:5]
        assert cpts.shape == (5, k, M, 2) and cw.shape == (5, k, M, 3) and cpeak.shape == (5, k, M) and order.shape == (5, k)
        assert count[bad].tolist() == [0, 0] and bool((order[bad] == -1).all())
        assert not bool(cpts[bad].any()) and not bool(cw[bad].any()) and not bool(cpeak[bad].any())
        for g, a in zip(got[:5], alone[:5]):
            assert TRF._bits(g[good], a), what
        cs = count[good].tolist()
        assert all(4 <= c <= k for c in cs) and any(c < k for c in cs), cs           # a true selection
        if weights != "peak":
            live = torch.arange(k, device="cuda")[None, :, None] < count[:, None, None]
            assert bool((cw[..., 0] > 0)[live.expand_as(cw[..., 0])].any()), what     # some point carries a Hessian weight
        # the packed record: the five views where the description says
        lay = inf.packed_layout(5, k, candidates=M, kind="candidate_correspondences")
        ccpacked = priv.records["candidate_correspondences"][0]
        assert ccpacked.dtype == torch.uint8 and ccpacked.numel() == lay["total"][1]
        for n, t in ((n, priv[n]) for n in R.FIELDS):
            assert t.data_ptr() == ccpacked.data_ptr() + lay[n][0] and t.numel() * t.element_size() == lay[n][1], n


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(env):
    sc = TCF._wrong_blob_frames(env)
    return sc, TRF._pattern_net(env, sc["patterns"]), torch.from_numpy(sc["frames"]).cuda()


def _kw(refine, weights, more):
    return dict(scale=TCF.CROP, on_fail="nan", thresh=0.0, min_k=8, candidates=3, nms_radius=6, return_report=True, refine=refine,
                weights=weights, **more)


@pytest.mark.parametrize("refine,weights,more", PAIRS)
def test_candidate_poses_device_select_equals_the_loader_path(env, scene, refine, weights, more):
    pipeline = env["pipeline"]
    sc, net, frames = scene
    kw = _kw(refine, weights, more)
    args = (net, frames, sc["bboxes"], sc["kp3d"], sc["K"])
    want, wrep = pipeline.candidate_poses(*args, candidates_path="loader", **kw)
    got, grep = pipeline.candidate_poses(*args, device_select=True, **kw)
    print(refine, weights, "status", grep.status.tolist(), "runner-ups used", int((grep.used > 0).sum()), "rescued", grep.rescued.tolist())
    assert TCF._same_poses(got, want) and TRF._same_report(grep, wrep)
    assert grep.rescued.all() and (grep.status == 0).all()                          # every image rescued: the swap path ran
    plain = pipeline.candidate_poses(*args, device_select=True, **dict(kw, return_report=False))
    assert TCF._same_poses(plain, want)
    # a frame index is the loader's to take
    again, _ = pipeline.candidate_poses(*args, device_select=True, frame_idx=list(range(len(sc["bboxes"]))), **kw)
    assert TCF._same_poses(again, want)
    # an invalid box follows on_fail
    boxes = [list(b) for b in sc["bboxes"]]
    boxes[1] = [500, 500, 500, 500]
    bad_args = (net, frames, boxes, sc["kp3d"], sc["K"])
    want, wrep = pipeline.candidate_poses(*bad_args, candidates_path="loader", **kw)
    got, grep = pipeline.candidate_poses(*bad_args, device_select=True, **kw)
    assert TCF._same_poses(got, want) and TRF._same_report(grep, wrep)
    assert np.isnan(got[1][0]).all() and np.isnan(got[1][1]).all() and grep.status[1] == 1 and grep.n[1] == 0
    assert (grep.used[1] == -1).all() and not grep.rescued[1] and grep.rescued[[0, 2, 3]].all()
    with pytest.raises(pipeline.PoseFailure, match=r"\[1\]"):
        pipeline.candidate_poses(*bad_args, device_select=True, **dict(kw, on_fail="raise"))


def test_distributed_under_nccl_at_world_size_1(env, scene, monkeypatch):
    pipeline, par = env["pipeline"], env["parallel"]
    sc, net, frames = scene
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(H._free_port()))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    refine, weights, more = PAIRS[1]
    kw = _kw(refine, weights, more)
    boxes = [list(b) for b in sc["bboxes"]]
    boxes[2] = [500, 500, 500, 500]
    args = (net, frames, boxes, sc["kp3d"], sc["K"])
    want = {path: pipeline.candidate_poses(*args, **dict(kw, **path_kw)) for path, path_kw in
            (("select", dict(device_select=True)), ("loader", dict(candidates_path="loader")))}
    sel = dict(scale=TCF.CROP, refine=refine, candidates=3, nms_radius=6, thresh=0.0, min_k=8, weights=weights)
    with torch.no_grad():
        want_c = net.frames_to_candidate_correspondences(frames, boxes, **sel)[:5]
        want_r = net.frames_to_candidates(frames, boxes, scale=TCF.CROP, candidates=3, nms_radius=6, refine=refine, return_hessian=True)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        assert dist.get_backend() == "nccl"
        with torch.no_grad():
            got = par.sharded_frames_to_candidate_correspondences(net, frames, boxes, **sel)
            assert len(got) == 5 and all(t.is_cuda for t in got)
            TRF._same(got, want_c, "sharded record")
            got = par.sharded_frames_to_candidates(net, frames, boxes, scale=TCF.CROP, candidates=3, nms_radius=6, refine=refine,
                                                   return_hessian=True)
            TRF._same(got, want_r, "sharded candidates")
        for path, path_kw in (("select", dict(device_select=True)), ("loader", dict(candidates_path="loader"))):
            got, grep = pipeline.candidate_poses(*args, distributed=True, **dict(kw, **path_kw))
            assert TCF._same_poses(got, want[path][0]) and TRF._same_report(grep, want[path][1]), path
        assert TCF._same_poses(want["select"][0], want["loader"][0])
    finally:
        dist.destroy_process_group()
