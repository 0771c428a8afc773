"""The packed records of the device path across ranks, without a GPU: inference.record_fields against the two layouts it
describes (inference.packed_layout, inference.pack_correspondences); the slicing form of the exchange
(parallel.gather_records_slicing) on hand-built blocks with poisoned padding; parallel.sharded_frames_to_correspondences under
gloo at world size 2 with a stub net; pipeline.estimate_poses(distributed=True) with the device loader and the device
selection; and the refusals of esahrnet_gather_records, all of which come before anything is enqueued."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from esa_pose_estimation_amd import inference, parallel

LAYOUTS = [(False, False), (True, False), (True, True)]          # every (gaussfit, cov) packed_layout accepts


# ---- 1. the record description ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 32])
@pytest.mark.parametrize("k", [1, 11, 30, 32])
def test_record_fields_rebuild_both_layouts(m, k):
    for gaussfit, cov in LAYOUTS:
        lay = inference.packed_layout(m, k, gaussfit, cov)
        fields = inference.record_fields(k, "keypoints", gaussfit, cov)
        assert [n for n, _ in fields] == [n for n in lay if n != "total"]         # memory order (packed_layout's dict order)
        off = 0
        for name, b in fields:
            assert b > 0 and b % 4 == 0
            assert lay[name] == (off, m * b), (name, gaussfit, cov)
            off += m * b
        assert lay["total"] == (0, off)
    count, order, pts, w, packed = inference.pack_correspondences(m, k, "cpu")
    views = {"count": count, "order": order, "pts": pts, "w": w}
    fields = inference.record_fields(k, "correspondences")
    off = 0
    for name, b in fields:
        assert b > 0 and b % 4 == 0
        t = views.pop(name)
        assert t.data_ptr() - packed.data_ptr() == off and t.numel() * t.element_size() == m * b, name
        off += m * b
    assert not views and off == packed.numel()
    # the typed views: the tensors pack_correspondences hands out
    again = inference.record_views(packed, m, k, fields)
    for name, t in (("count", count), ("order", order), ("pts", pts), ("w", w)):
        assert again[name].data_ptr() == t.data_ptr() and again[name].shape == t.shape and again[name].dtype == t.dtype
    # the candidates form: the third kind against the third layout
    forms = [fields] + [inference.record_fields(k, "keypoints", gaussfit, cov) for gaussfit, cov in LAYOUTS]
    for M in (1, 2, 3, 4):
        lay = inference.packed_layout(m, k, candidates=M)
        fields = inference.record_fields(k, "candidates", candidates=M)
        assert [n for n, _ in fields] == [n for n in lay if n != "total"] == ["rates", "cand", "boxes", "valid", "cidx"]
        off = 0
        for name, b in fields:
            assert b > 0 and b % 4 == 0
            assert lay[name] == (off, m * b), (name, M)
            off += m * b
        assert lay["total"] == (0, off)
        forms.append(fields)
    # the numpy form of the views, all three kinds: the offsets, shapes and types of the torch views, on the same bytes
    for fields in forms:
        packed = torch.randint(0, 256, (m * sum(b for _, b in fields),), dtype=torch.uint8, generator=torch.Generator().manual_seed(k))
        host = packed.numpy().copy()
        tv, nv = inference.record_views(packed, m, k, fields), inference.record_views(host, m, k, fields)
        assert list(tv) == list(nv) == [n for n, _ in fields]
        for name, t in tv.items():
            a = nv[name]
            assert isinstance(a, np.ndarray) and np.shares_memory(a, host)                        # a view, no copy
            assert a.ctypes.data - host.ctypes.data == t.data_ptr() - packed.data_ptr()
            assert a.shape == tuple(t.shape) and a.dtype == t.numpy().dtype and a.tobytes() == t.numpy().tobytes()
        if "cand" in tv:
            M = fields[1][1] // (12 * k)
            assert tv["cand"].shape == (m, k, M, 3) and tv["cidx"].shape == (m, k, M)             # M from the field's bytes
        with pytest.raises(ValueError, match="bytes"):
            inference.record_views(host[:-4], m, k, fields)


def test_record_fields_refuses_what_the_layouts_refuse():
    with pytest.raises(ValueError):
        inference.record_fields(11, "keypoints", gaussfit=False, cov=True)
    with pytest.raises(ValueError):
        inference.record_fields(11, "poses")
    with pytest.raises(ValueError):
        inference.record_fields(11, "correspondences", gaussfit=True)
    with pytest.raises(ValueError):
        inference.record_fields(0, "keypoints")


# ---- 2. the slicing form on hand-built blocks ------------------------------------------------------------------------------
def hand_built_blocks(full: np.ndarray, world: int, n_total: int, fb, poison=0xFF):
    """The unsharded record `full` (uint8, n_total crops, fields of fb bytes per crop) -> what an all-gather of the ranks' blocks
    would leave: crop by crop and field by field, written down from the issue's formula, everything else `poison`."""
    n_max = -(-n_total // world)
    per = sum(fb)
    out = np.full(world * n_max * per, poison, np.uint8)
    for r in range(world):
        lo, hi = parallel.shard_bounds(n_total, world, r)
        for i in range(lo, hi):
            before = 0
            for b in fb:
                src = n_total * before + i * b
                dst = r * n_max * per + n_max * before + (i - lo) * b
                out[dst:dst + b] = full[src:src + b]
                before += b
    return out


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n_total", [1, 2, 5, 8, 9])
def test_slicing_form_reproduces_the_unsharded_record(world, n_total):
    rng = np.random.default_rng(100 * world + n_total)
    for fields in (inference.record_fields(11, "keypoints", True, True), inference.record_fields(11, "correspondences"),
                   inference.record_fields(1, "keypoints")):
        fb = [b for _, b in fields]
        full = rng.integers(0, 255, size=n_total * sum(fb), dtype=np.uint8)        # never 0xFF: poison read would show
        blocks = torch.from_numpy(hand_built_blocks(full, world, n_total, fb))
        got = parallel.gather_records_slicing(blocks, world, n_total, fields)
        assert got.dtype == torch.uint8 and torch.equal(got, torch.from_numpy(full))
        assert torch.equal(parallel.gather_records_slicing(blocks, world, n_total, fb), got)      # bare byte counts too


def test_gather_records_without_a_group():
    fields = inference.record_fields(11, "correspondences")
    per = sum(b for _, b in fields)
    buf = torch.zeros(4 * per, dtype=torch.uint8)
    assert parallel.gather_records(buf, 4, 4, fields) is buf
    with pytest.raises(ValueError, match="no process group but shard size != batch size"):
        parallel.gather_records(buf, 4, 5, fields)
    with pytest.raises(ValueError):
        parallel.gather_records(buf[:-4], 4, 4, fields)
    with pytest.raises(ValueError):
        parallel.gather_records_slicing(buf, 3, 4, fields)                        # 3 blocks of 2 crops are more bytes


# ---- 3. the sharded calls with a stub net -----------------------------------------------------------------------------------
class StubNet:
    """Stands in for the GPU model: its _loader fills the two records from the box values, the frame each box lies on
    (read THROUGH the frame index it was given, so a wrong index shows) and the keypoint number; CPU tensors."""

    def __init__(self, k):
        self.num_keypoints = k
        self.calls = []

    def _keypoint_record(self, frames, boxes, idx, gaussfit=False, cov=False):
        m, k = len(boxes), self.num_keypoints
        idx = list(range(m)) if idx is None else [int(i) for i in idx]
        lay = inference.packed_layout(m, k, gaussfit, cov)
        packed = torch.zeros(lay["total"][1], dtype=torch.uint8)

        def part(name, dtype, *shape):
            o, b = lay[name]
            return packed[o:o + b].view(dtype).view(*shape)

        b = torch.tensor([list(x) for x in boxes], dtype=torch.float64)
        frame = torch.tensor([float(frames[i].reshape(-1)[0]) if 0 <= i < frames.shape[0] else -1.0 for i in idx], dtype=torch.float64)
        ks = torch.arange(k, dtype=torch.float64)
        v = b[:, 0, None] * 100.0 + frame[:, None] * 10000.0 + ks[None]                       # [m, k]
        rates, kp, cb = part("rates", torch.float64, m), part("kp", torch.float32, m, k, 3), part("boxes", torch.int32, m, 4)
        valid, ix = part("valid", torch.int32, m), part("idx", torch.int32, m, k)
        rates.copy_(b[:, 1] + 0.5)
        kp.copy_(torch.stack([v, v + 0.25, v + 0.5], 2))
        cb.copy_(b + 1)
        valid.copy_(frame >= 0)
        ix.copy_(v + 7)
        extra = ()
        if gaussfit:
            fit, status, hess = part("fit", torch.float64, m, k, 8), part("status", torch.int32, m, k), part("hess", torch.float64, m, k, 3)
            fit.copy_(v[..., None] + torch.arange(8) / 16)
            status.copy_(v % 4)
            hess.copy_(-v[..., None] - torch.arange(3))
            extra = (fit, status, hess)
        if cov:
            cv, info = part("cov", torch.float64, m, k, 3), part("info", torch.float64, m, k, 3)
            cv.copy_(v[..., None] * 2 + torch.arange(3))
            info.copy_(v[..., None] * 3 + torch.arange(3))
            extra += (cv, info)
        return (kp, cb, rates, valid, ix, packed) + extra, v

    def _loader(self, request, frames, boxes, idx, scale, rule, mean, std, pixel_format):
        self.calls.append(("kp" if request.select is None else "corr", len(boxes)))
        m, k = len(boxes), self.num_keypoints
        _, gaussfit, cov, _ = request.main
        out, v = self._keypoint_record(frames, boxes, idx, gaussfit, cov)
        records = {"keypoints": (out[5], inference.record_fields(k, "keypoints", gaussfit, cov))}
        if request.select is not None:
            count, order, pts, w, cpacked = inference.pack_correspondences(m, k, "cpu")
            count.copy_(v[:, 0] % (k + 1))
            order.copy_((v + 3) % k)
            pts.copy_(torch.stack([v + 0.125, v + 0.375], 2))
            w.copy_(torch.stack([v, -v, v * 2], 2))
            records["correspondences"] = (cpacked, inference.record_fields(k, "correspondences"))
        return inference.LoaderResult(m, k, records)


CORR = ("count", "order", "pts", "w", "kp", "boxes", "rates", "valid")       # sharded_frames_to_correspondences' returns, by name


def _request(refine, weights=None, cov_floor=None):
    """The request of the correspondences (weights given) or of the keypoints, as the public calls build it."""
    if weights is None:
        return inference.LoaderRequest(refine, None, cov_floor)
    return inference.LoaderRequest(refine, None, 1e-6 if weights == "covariance" else None, (0.8, 24, weights))


def _named(r, names):
    return tuple(r[n] for n in names)


def _same_result(a, b):
    """Two loader results: the same records, byte for byte, and the same typed views of them under the same names."""
    kinds, names = sorted(a.records), sorted(a.views)
    return (a.m, a.k, kinds, names) == (b.m, b.k, sorted(b.records), sorted(b.views)) and \
        all(a.records[kind][1] == b.records[kind][1] for kind in kinds) and \
        _same([a.records[kind][0] for kind in kinds], [b.records[kind][0] for kind in kinds]) and \
        _same([a[n] for n in names], [b[n] for n in names])


def _batch(n_total):
    """n_total boxes on n_total frames; frame f holds the value f + 1, so the stub reads the frame's number off the frame."""
    frames = (torch.arange(n_total, dtype=torch.uint8) + 1).view(-1, 1, 1).expand(n_total, 2, 2).contiguous()
    boxes = [(3 * i + 1, 2 * i + 5, 3 * i + 40, 2 * i + 50) for i in range(n_total)]
    return frames, boxes


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_total, k, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lo, hi = parallel.shard_bounds(n_total, world, rank)
        frames, boxes = _batch(n_total)
        ok = True
        for refine, weights in (("get_final", "peak"), ("get_final2", "hessian"), ("gaussfit", "covariance")):
            want = StubNet(k)._loader(_request(refine, weights), frames, boxes, None, 64, "val", None, 0.229, None)
            kw = dict(scale=64, refine=refine, weights=weights)
            # (a) every rank holds the whole batch's frames
            net = StubNet(k)
            got = parallel._sharded_loader(net, _request(refine, weights), frames, boxes, None, None, 0, 64, "val", None, 0.229, None)
            ok = ok and _same_result(got, want) and net.calls == ([("corr", hi - lo)] if hi > lo else [])
            ok = ok and _same(parallel.sharded_frames_to_correspondences(StubNet(k), frames, boxes, **kw), _named(want, CORR))
            # (b) a rank holds only its own frames: frame_base = lo, indices rebased
            ok = ok and _same(parallel.sharded_frames_to_correspondences(StubNet(k), frames[lo:hi], boxes, frame_base=lo, **kw),
                              _named(want, CORR))
            # (c) explicit frame indices, several boxes on one frame
            fidx = [i // 2 for i in range(n_total)]
            want_f = StubNet(k)._loader(_request(refine, weights), frames, boxes, fidx, 64, "val", None, 0.229, None)
            ok = ok and _same(parallel.sharded_frames_to_correspondences(StubNet(k), frames, boxes, fidx, **kw), _named(want_f, CORR))
            ok = ok and _same(parallel.sharded_frames_to_correspondences(StubNet(k), frames, boxes,
                                                                         torch.tensor(fidx, dtype=torch.int32), **kw), _named(want_f, CORR))
        # the keypoint form, with every extra output
        want = StubNet(k)._loader(_request("gaussfit", cov_floor=1e-6), frames, boxes, None, 64, "val", None, 0.229, None)
        got = parallel.sharded_frames_to_keypoints(StubNet(k), frames, boxes, scale=64, refine="gaussfit", return_cov=True)
        ok = ok and _same(got, _named(want, CORR[4:] + ("fit", "status", "hess", "cov", "info")))
        want = StubNet(k)._loader(_request("get_final"), frames, boxes, None, 64, "val", None, 0.229, None)
        ok = ok and _same(parallel.sharded_frames_to_keypoints(StubNet(k), frames, boxes, scale=64), _named(want, CORR[4:]))
        # a wrong shard size: gather_keypoints' message
        try:
            parallel.gather_records(torch.zeros(4 * (hi - lo + 1), dtype=torch.uint8), hi - lo + 1, n_total, [4])
            ok = False
        except ValueError as e:
            ok = ok and str(e) == f"rank {rank}: shard has {hi - lo + 1} crops, expected {hi - lo}"
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_total", [8, 7, 1])          # even split, uneven tail, an EMPTY shard on rank 1
def test_sharded_frames_to_correspondences_world2(n_total):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_total, 11, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(res) == [(0, True), (1, True)]


# ---- 4. the pipeline ---------------------------------------------------------------------------------------------------------
def _poses_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(qa, qb, equal_nan=True) and np.array_equal(ta, tb, equal_nan=True)
                                    for (qa, ta), (qb, tb) in zip(a, b))


def test_estimate_poses_distributed_takes_the_device_path():
    """distributed=True with device_select=True / device_loader=True used to be refused ("runs on one device"); without a process
    group the sharded call is the net's own call, so the poses are those of distributed=False."""
    from esa_pose_estimation_amd import pipeline, synth
    k, n = 11, 4
    frames, boxes = _batch(n)
    kp3d = synth.make_scene(n, k, seed=0)["kp3d"]
    args = (frames, boxes, kp3d, synth.ESA_CAMERA)
    kw = dict(scale=64, on_fail="nan", thresh=0.8, min_k=4)
    net = StubNet(k)
    got = pipeline.estimate_poses(net, *args, distributed=True, device_select=True, **kw)
    assert net.calls == [("corr", n)] and len(got) == n
    assert _poses_equal(got, pipeline.estimate_poses(StubNet(k), *args, device_select=True, **kw))
    got = pipeline.estimate_poses(StubNet(k), *args, distributed=True, device_select=True, refine="gaussfit", weights="covariance", **kw)
    assert _poses_equal(got, pipeline.estimate_poses(StubNet(k), *args, device_select=True, refine="gaussfit", weights="covariance", **kw))
    net = StubNet(k)
    got = pipeline.estimate_poses(net, *args, distributed=True, device_loader=True, **kw)
    assert net.calls == [("kp", n)] and _poses_equal(got, pipeline.estimate_poses(StubNet(k), *args, device_loader=True, **kw))
    # the messages that stay
    with pytest.raises(ValueError, match="native=False has no entry"):
        pipeline.estimate_poses(StubNet(k), *args, distributed=True, device_select=True, native=False, **kw)
    with pytest.raises(ValueError, match="belongs to device_select=True"):
        pipeline.estimate_poses(StubNet(k), *args, distributed=True, device_loader=True, weights="hessian", refine="get_final2", **kw)


# ---- 5. the library's refusals ---------------------------------------------------------------------------------------------
def test_gather_records_refusals():
    """Every refusal is made on the host before a launch: the pointers are never touched (they point nowhere)."""
    from esa_pose_estimation_amd import _lib
    lib = _lib.lib()
    good = (C.c_int * 4)(176, 264, 4, 44)
    p, o = C.c_void_p(0x10000), C.c_void_p(0x20000)

    def refused(gathered, world, n_total, fields, nfields, out, words):
        rc = lib.esahrnet_gather_records(gathered, world, n_total, fields, nfields, out, None)
        msg = lib.esahrnet_last_error().decode()
        assert rc != 0 and msg.startswith("gather_records:") and all(w in msg for w in words), (rc, msg)

    refused(p, 0, 5, good, 4, o, ["world"])
    refused(p, -1, 5, good, 4, o, ["world"])
    refused(p, 2, 0, good, 4, o, ["n_total"])
    refused(p, 2, -3, good, 4, o, ["n_total"])
    refused(p, 2, 5, (C.c_int * 4)(176, 0, 4, 44), 4, o, ["field 1", "multiple of 4"])
    refused(p, 2, 5, (C.c_int * 4)(176, 264, -4, 44), 4, o, ["field 2", "multiple of 4"])
    refused(p, 2, 5, (C.c_int * 4)(176, 264, 4, 42), 4, o, ["field 3", "multiple of 4"])
    refused(None, 2, 5, good, 4, o, ["null"])
    refused(p, 2, 5, good, 4, None, ["null"])
    refused(p, 2, 5, None, 4, o, ["null"])
    refused(C.c_void_p(0x10004), 2, 5, good, 4, o, ["8-byte aligned"])
    refused(p, 2, 5, good, 4, C.c_void_p(0x20004), ["8-byte aligned"])
    refused(p, 2, 5, good, 0, o, ["fields"])
    refused(p, 2, 5, (C.c_int * 17)(*([4] * 17)), 17, o, ["fields"])
    # 2^20 crops per block x 2048 bytes = 2^31 bytes: one past the limit
    refused(p, 2, 2 ** 21, (C.c_int * 1)(2048), 1, o, ["2^31"])
    refused(p, 1, 2 ** 20, (C.c_int * 2)(1024, 1024), 2, o, ["2^31"])
    with pytest.raises(_lib.EsaHrnetError, match="gather_records: world"):
        _lib.check(lib.esahrnet_gather_records(p, 0, 5, good, 4, o, None))
