"""CPU: the runner-up repair on image-pixel points (include/esahrnet.h esahrnet_correspondences_cand,
esahrnet_pnp_batch_cand_pts).  No device is touched.

  * the header declares the two entries, the library exports them, _lib binds them, the ABI stays 6;
  * every refusal of both entries, in the order the header states: each case also sets off a LATER check, so the order is pinned;
  * the record kind "candidate_correspondences": field order, bytes per crop and alignment as literals, the views round-trip, and
    the four older kinds still equal tests/golden/record_layouts.json;
  * the solver: the numpy restatement tests/candidate_correspond_ref.py turns (cand, hess, boxes, rates, valid) into the record,
    and esahrnet_pnp_batch_cand_pts on it gives the bits of esahrnet_pnp_batch_cand_w / _cand on the rows: q, t, all 33 report
    doubles and used, for 1, 2 and 4 threads;
  * pipeline.candidate_poses: the new argument errors, and with a stub net under gloo at world size 2 distributed=True returns the
    single-process poses on both ranks (even split, uneven tail, empty shard)."""
import ctypes as C
import json
import multiprocessing as mp
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import candidate_correspond_ref as R  # noqa: E402
import candidates_ref as CR  # noqa: E402

from esa_pose_estimation_amd import _lib, inference, parallel, pipeline, pnp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esahrnet_correspondences_cand", "esahrnet_pnp_batch_cand_pts")


# ---- 1. header and bindings ------------------------------------------------------------------------------------------------
def test_header_library_and_bindings():
    with open(os.path.join(ROOT, "include", "esahrnet.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in _lib._SIGS and getattr(L, name).argtypes == _lib._SIGS[name][1]
    assert len(_lib._SIGS["esahrnet_correspondences_cand"][1]) == 17 and len(_lib._SIGS["esahrnet_pnp_batch_cand_pts"][1]) == 16
    assert re.search(r"#define ESAHRNET_ABI_VERSION 6\b", header) and L.esahrnet_abi_version() == 6 == _lib.ABI_VERSION


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------
def _err():
    return _lib.lib().esahrnet_last_error().decode()


def test_refusals_of_correspondences_cand_in_their_order():
    """The pointers are host memory the entry never reads: every case is refused before anything is enqueued."""
    L = _lib.lib()
    buf = (C.c_double * 64)()
    base = C.addressof(buf)
    assert base % 8 == 0

    def call(cand=base, hess=base, crop=base, rates=base, valid=base, m=1, k=11, M=3, mode=0, count=base, order=base, cpts=base,
             cw=base, cpeak=base):
        return L.esahrnet_correspondences_cand(cand, hess, crop, rates, valid, m, k, M, 0.8, 24, mode, count, order, cpts, cw, cpeak,
                                               None)

    cases = [
        # 1. a NULL pointer, with m <= 0 behind it
        *[(dict({name: None}, m=0), "null argument") for name in ("cand", "crop", "rates", "valid", "count", "order", "cpts", "cw",
                                                                   "cpeak")],
        (dict(hess=None, mode=1, m=0), "null argument"),
        # 2. m <= 0, with a bad k behind it
        (dict(m=0, k=33), "number of crops must be positive (got 0)"), (dict(m=-2, k=0), "number of crops must be positive (got -2)"),
        # 3. k outside 1..32, with a bad M behind it
        (dict(k=0, M=5), "0 keypoints per crop unsupported (1..32"), (dict(k=33, M=0), "33 keypoints per crop unsupported (1..32"),
        # 4. M outside 1..4, with a bad mode behind it
        (dict(M=0, mode=2), "0 candidates per keypoint unsupported (1..4)"), (dict(M=5, mode=-1), "5 candidates per keypoint unsupported (1..4)"),
        # 5. mode outside 0..1, with a misaligned pointer behind it
        (dict(mode=2, cpts=base + 4), "mode=2 unknown"), (dict(mode=-1, cand=base + 2), "mode=-1 unknown"),
        # 6. alignment: 4 bytes for f32 / int32, 8 for f64
        *[(dict({name: base + 2}), "4-byte aligned") for name in ("cand", "crop", "valid", "count", "order", "cpeak")],
        *[(dict({name: base + 4}), "8-byte aligned") for name in ("rates", "cpts", "cw")],
        (dict(hess=base + 4, mode=1), "8-byte aligned"),
    ]
    for kw, text in cases:
        assert call(**kw) == 1, kw
        assert _err().startswith("correspondences_cand: ") and text in _err(), (kw, _err())
    # hess_dev is not looked at with mode 0: NULL and a misaligned one pass the checks ... which a test without a device cannot
    # let through to the launch; the order above has shown that both are examined only under mode 1 (the two mode-1 cases)


def test_refusals_of_pnp_batch_cand_pts_in_their_order():
    L = _lib.lib()
    k, M = 11, 3
    z = np.zeros(2 * k * M * 3)
    zf = np.zeros(2 * k * M, np.float32)
    count = np.array([4, 5], np.int32)
    order = np.tile(np.arange(k, dtype=np.int32), (2, 1))
    out = np.zeros(128)
    used = np.zeros(2 * k, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)               # noqa: E731

    def call(cpts=z, cw=z, cpeak=zf, count=count, order=order, m=2, k=k, M=M, kp3d=z, K9=z, ratio=0.3, q=out, t=out, rep=out,
             used=used):
        return L.esahrnet_pnp_batch_cand_pts(p(cpts), p(cw), p(cpeak), p(count), p(order), m, k, M, p(kp3d), p(K9), ratio, 1, p(q),
                                             p(t), p(rep), p(used))

    bad_count, bad_order = count.copy(), order.copy()
    bad_count[1] = k + 1
    bad_order[1, 4] = k                                     # among the first count[1] = 5
    cases = [
        *[(dict({name: None}, m=-1), "null argument") for name in ("cpts", "cw", "cpeak", "count", "order", "kp3d", "K9", "q", "t",
                                                                   "used")],
        (dict(m=-1, k=0), "negative image count -1"),
        (dict(k=0, M=5), "0 keypoints per image unsupported (1..64)"), (dict(k=65, M=0), "65 keypoints per image unsupported (1..64)"),
        (dict(M=0, ratio=-1.0), "0 candidates per keypoint unsupported (1..4)"), (dict(M=5, ratio=-1.0), "5 candidates per keypoint unsupported"),
        (dict(ratio=-0.5, count=bad_count), "min_ratio"), (dict(ratio=float("nan"), count=bad_count), "min_ratio"),
        (dict(count=bad_count, order=bad_order), f"count[1] = {k + 1} outside 0..{k}"),
        (dict(count=np.array([4, -1], np.int32), order=bad_order), f"count[1] = -1 outside 0..{k}"),
        (dict(order=bad_order), f"order[1][4] = {k} is no keypoint index (0..{k - 1})"),
    ]
    for kw, text in cases:
        assert call(**kw) == 1, kw
        assert _err().startswith("pnp_batch_cand_pts: ") and text in _err(), (kw, _err())
    # a bad order entry BEYOND count is not looked at, and a null report is allowed
    beyond = order.copy()
    beyond[1, 5] = -7
    assert call(order=beyond, rep=None) == 0


# ---- 3. the record kind -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_record_kind_candidate_correspondences(m, M):
    assert "candidate_correspondences" in inference.RECORD_KINDS
    for k in (1, 11, 32):
        fields = inference.record_fields(k, "candidate_correspondences", candidates=M)
        assert fields == (("cpts", 16 * k * M), ("cw", 24 * k * M), ("cpeak", 4 * k * M), ("count", 4), ("order", 4 * k))
        lay = inference.packed_layout(m, k, candidates=M, kind="candidate_correspondences")
        assert lay == {"cpts": (0, 16 * k * M * m), "cw": (16 * k * M * m, 24 * k * M * m), "cpeak": (40 * k * M * m, 4 * k * M * m),
                       "count": (44 * k * M * m, 4 * m), "order": (44 * k * M * m + 4 * m, 4 * k * m),
                       "total": (0, (44 * k * M + 4 + 4 * k) * m)}
        assert lay["cpts"][0] % 8 == 0 and lay["cw"][0] % 8 == 0                    # the f64 fields, for every m
        cpts, cw, cpeak, count, order, packed = inference.pack_candidate_correspondences(m, k, M, "cpu")
        assert packed.dtype == torch.uint8 and packed.numel() == lay["total"][1]
        want = {"cpts": (torch.float64, (m, k, M, 2)), "cw": (torch.float64, (m, k, M, 3)), "cpeak": (torch.float32, (m, k, M)),
                "count": (torch.int32, (m,)), "order": (torch.int32, (m, k))}
        for name, t in zip(R.FIELDS, (cpts, cw, cpeak, count, order)):
            assert (t.dtype, tuple(t.shape)) == want[name] and t.data_ptr() - packed.data_ptr() == lay[name][0], name
        # round trip: written through the torch views, read through the numpy views of the copied bytes
        rng = np.random.default_rng(m * 100 + M)
        vals = {name: rng.integers(-50, 50, shape).astype(inference._NUMPY_TYPES[dt]) for name, (dt, shape) in want.items()}
        for name, t in zip(R.FIELDS, (cpts, cw, cpeak, count, order)):
            t.copy_(torch.from_numpy(vals[name]))
        back = inference.record_views(packed.numpy().copy(), m, k, fields)
        assert list(back) == list(R.FIELDS) and all(R.same_bits(back[n], vals[n]) for n in R.FIELDS)
    for bad in (None, 0, 5):
        with pytest.raises(ValueError, match="candidates"):
            inference.record_fields(11, "candidate_correspondences", candidates=bad)
    with pytest.raises(ValueError, match="gaussfit and cov belong"):
        inference.record_fields(11, "candidate_correspondences", True, candidates=3)


def test_the_four_older_kinds_keep_their_recorded_layouts():
    import test_record_layout_host as T
    with open(T.GOLDEN) as f:
        golden = json.load(f)
    now = T.recorded(inference, pipeline)
    for part in ("packed_layout", "record_fields", "pack_correspondences"):
        assert now[part] == golden[part], part
    # (the record holds keypoints, correspondences and candidates; candidates_refined, younger than it, as literals)
    assert set(inference.RECORD_KINDS) == {"keypoints", "correspondences", "candidates", "candidates_refined", "candidate_correspondences"}
    k, M = 11, 3
    assert inference.record_fields(k, "candidates_refined", True, True, M) == (
        ("rates", 8), ("cand_fit", 64 * k * M), ("cand_hess", 24 * k * M), ("cand_cov", 24 * k * M), ("cand_info", 24 * k * M),
        ("cand", 12 * k * M), ("boxes", 16), ("valid", 4), ("cidx", 4 * k * M), ("cand_status", 4 * k * M))
    assert inference.record_fields(k, "candidates_refined", candidates=M) == (
        ("rates", 8), ("cand_hess", 24 * k * M), ("cand", 12 * k * M), ("boxes", 16), ("valid", 4), ("cidx", 4 * k * M))


# ---- 4. the solver on the record against the solver on the rows -------------------------------------------------------------
MIN_RATIO = 0.3


def _wrong_blob_inputs():
    """tests/candidates_ref.py's scene through its numpy decoder: n = 4, K = 11, M = 3, 64 x 64 crops."""
    sc = CR.wrong_blob_scene()
    cand, _ = CR.candidates(CR.wrong_blob_heatmaps(sc).numpy(), 3, 6)
    boxes = np.array([(x, y, x + 1, y + 1) for x, y in sc["boxes"]], np.int32)
    return dict(kp3d=sc["kp3d"], K=sc["K"], cand=cand, crop_boxes=boxes, rates=np.asarray(sc["rates"], np.float64)), 0.5, 0


def _random_inputs():
    return R.random_scene(np.random.default_rng(4321), 10, 32, 6, M=4), 0.45, 12


def _classes(cand, hess, rates, used, min_ratio):
    """How often each class of input the comparison must contain occurs."""
    finite = np.isfinite(cand[..., 0]) & np.isfinite(cand[..., 1])
    runner = finite.copy()
    runner[:, :, 0] = False
    ratio_ok = cand[..., 2].astype(np.float64) >= min_ratio * cand[:, :, :1, 2].astype(np.float64)
    not_pd = 0
    if hess is not None:
        for idx in np.argwhere(finite & np.isfinite(hess).all(-1)):
            i = tuple(idx)
            not_pd += int(not R.hessian_weight(hess[i], rates[i[0]]).any())
    return {"absent runner-up": int((~finite[:, :, 1:]).sum()), "runner-up below min_ratio": int((runner & ~ratio_ok).sum()),
            "Hessian not positive definite": not_pd, "swap taken": int((used > 0).sum()),
            "swap not taken": int(((runner & ratio_ok).any(2) & (used == 0)).sum())}


@pytest.fixture(scope="module", params=["wrong-blob", "random"])
def solved(request):
    """One scene, its Hessians, the record the restatement makes of them (modes 0 and 1) and the rows' solves at one thread."""
    sc, thresh, min_k = _wrong_blob_inputs() if request.param == "wrong-blob" else _random_inputs()
    assert np.isfinite(sc["cand"][:, :, 0]).all()           # primary peaks are numbers: the host sort has no order for NaN
    hess = R.random_hessians(np.random.default_rng(99), sc["cand"])
    valid = np.ones(len(sc["cand"]), np.int32)
    rec = {mode: R.record(sc["cand"], hess if mode else None, sc["crop_boxes"], sc["rates"], valid, thresh, min_k, mode) for mode in (0, 1)}
    rows = {mode: pnp.candidates_to_pose_batch(sc["cand"], sc["kp3d"], sc["K"], sc["crop_boxes"][:, :2], sc["rates"], thresh, min_k,
                                               MIN_RATIO, 1, report=True, hess=hess if mode else None) for mode in (0, 1)}
    return request.param, sc, hess, rec, rows


@pytest.mark.parametrize("threads", [1, 2, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_solver_on_the_record_equals_the_solver_on_the_rows(solved, mode, threads):
    name, sc, hess, rec, rows = solved
    r = rec[mode]
    q, t, used, rep = pnp.candidate_correspondences_to_pose_batch(r["cpts"], r["cw"], r["cpeak"], r["count"], r["order"], sc["kp3d"],
                                                                  sc["K"], MIN_RATIO, threads, report=True)
    q0, t0, used0, rep0 = rows[mode]
    assert rep.raw.shape == (len(q), 33)
    for what, a, b in (("q", q, q0), ("t", t, t0), ("report", rep.raw, rep0.raw), ("used", used, used0)):
        assert R.same_bits(a, b), (name, mode, threads, what)
    assert np.array_equal(rep.rescued, rep0.rescued)
    # without a report: the same poses
    q1, t1, used1 = pnp.candidate_correspondences_to_pose_batch(r["cpts"], r["cw"], r["cpeak"], r["count"], r["order"], sc["kp3d"],
                                                                sc["K"], MIN_RATIO, threads)
    assert R.same_bits(q1, q) and R.same_bits(t1, t) and R.same_bits(used1, used)
    if name == "wrong-blob":
        assert rep.rescued.all() and (rep.status == 0).all()                        # every image rescued: the swap path ran


def test_the_inputs_hold_every_class():
    total = {}
    for make in (_wrong_blob_inputs, _random_inputs):
        sc, thresh, min_k = make()
        hess = R.random_hessians(np.random.default_rng(99), sc["cand"])
        _, _, used = pnp.candidates_to_pose_batch(sc["cand"], sc["kp3d"], sc["K"], sc["crop_boxes"][:, :2], sc["rates"], thresh, min_k,
                                                  MIN_RATIO, 1, hess=hess)
        got = _classes(sc["cand"], hess, sc["rates"], used, MIN_RATIO)
        print(make.__name__, got, "selected", int((used >= 0).sum()), "of", used.size)
        for name, n in got.items():
            total[name] = total.get(name, 0) + n
        if make is _random_inputs:
            assert (used == -1).any() and all(n > 0 for n in got.values()), got    # a true subset is selected; all classes here
    assert all(n > 0 for n in total.values()), total


def test_count_zero_and_nan_slots():
    """count = 0 (an invalid crop): the NaN pose and a report row of status 1 with n = 0; M = 1: the plain weighted solve."""
    sc, thresh, min_k = _random_inputs()
    valid = np.ones(len(sc["cand"]), np.int32)
    valid[[0, 3]] = 0
    r = R.record(sc["cand"], None, sc["crop_boxes"], sc["rates"], valid, thresh, min_k, 0)
    assert (r["count"][[0, 3]] == 0).all() and not r["cpts"][[0, 3]].any() and (r["order"][[0, 3]] == -1).all()
    q, t, used, rep = pnp.candidate_correspondences_to_pose_batch(*(r[n] for n in R.FIELDS), sc["kp3d"], sc["K"], MIN_RATIO, 2, report=True)
    for i in (0, 3):
        assert np.isnan(q[i]).all() and np.isnan(t[i]).all() and (used[i] == -1).all() and not rep.rescued[i]
        assert rep.raw[i, 0] == 1.0 and rep.raw[i, 2] == 0.0 and np.isnan(np.delete(rep.raw[i], [0, 2])).all()
    keep = [i for i in range(len(valid)) if valid[i]]
    q0, t0, used0, rep0 = pnp.candidates_to_pose_batch(sc["cand"], sc["kp3d"], sc["K"], sc["crop_boxes"][:, :2], sc["rates"], thresh,
                                                       min_k, MIN_RATIO, 1, report=True)
    assert R.same_bits(q[keep], q0[keep]) and R.same_bits(rep.raw[keep], rep0.raw[keep]) and R.same_bits(used[keep], used0[keep])
    # M = 1: esahrnet_pnp_batch_w_ex on the primaries
    one = R.record(sc["cand"][:, :, :1], None, sc["crop_boxes"], sc["rates"], valid, thresh, min_k, 0)
    q1, t1, used1, rep1 = pnp.candidate_correspondences_to_pose_batch(*(one[n] for n in R.FIELDS), sc["kp3d"], sc["K"], MIN_RATIO, 2,
                                                                      report=True)
    qw, tw, repw = pnp.correspondences_to_pose_batch(one["cpts"][:, :, 0], one["cw"][:, :, 0], one["count"], one["order"], sc["kp3d"],
                                                     sc["K"], 2, report=True)
    assert R.same_bits(q1, qw) and R.same_bits(t1, tw) and R.same_bits(rep1.raw, repw.raw) and set(np.unique(used1)) <= {0, -1}


# ---- 5. pipeline.candidate_poses ---------------------------------------------------------------------------------------------
def test_candidate_poses_argument_errors():
    a = (None, None, None, None, None)
    for path in ("fused", "loader"):
        with pytest.raises(ValueError, match="does not go with device_select=True"):
            pipeline.candidate_poses(*a, device_select=True, candidates_path=path)
    for path in ("heatmaps", "fused"):
        with pytest.raises(ValueError, match="distributed=True belongs to device_select=True or candidates_path='loader'"):
            pipeline.candidate_poses(*a, distributed=True, candidates_path=path)
    # the older checks still speak first, and frame_idx / rule are now accepted with device_select=True (the loader)
    with pytest.raises(ValueError, match="candidates_path must be one of"):
        pipeline.candidate_poses(*a, device_select=True, candidates_path="device")
    with pytest.raises(ValueError, match="weights='hessian' needs refine"):
        pipeline.candidate_poses(*a, device_select=True, refine="get_final")
    with pytest.raises(ValueError, match="frame_idx and rule belong to candidates_path='loader'"):
        pipeline.candidate_poses(*a, frame_idx=[0])
    import inspect
    sig = inspect.signature(pipeline.candidate_poses).parameters
    assert sig["device_select"].default is False and sig["distributed"].default is False
    assert "not built" not in pipeline.candidate_poses.__doc__


class StubNet:
    """Stands in for the GPU model: box i of the batch is (i, ...), and the record of a box is the restatement's record of scene
    image i, so the poses are real ones.  Image BAD is a crop the loader could not make.  CPU tensors."""
    BAD = 2

    def __init__(self, n_total, k=11, M=3):
        self.num_keypoints = k
        self.sc = R.random_scene(np.random.default_rng(77), max(n_total, 1), k, 2, M=M, side=64.0)
        self.hess = R.random_hessians(np.random.default_rng(78), self.sc["cand"])
        self.calls = []

    def _rows(self, boxes):
        ids = [int(b[0]) for b in boxes]
        valid = np.array([i != self.BAD for i in ids], np.int32)
        cand, hess = self.sc["cand"][ids].copy(), self.hess[ids].copy()
        cand[valid == 0] = np.nan
        hess[valid == 0] = np.nan
        return ids, valid, cand, hess

    def _loader(self, request, frames, boxes, idx, scale, rule, mean, std, pixel_format):
        """The one record the caller goes on with: the candidate correspondences of a request with a select, else the candidates."""
        ids, valid, cand, hess = self._rows(boxes)
        m, k = len(ids), self.num_keypoints
        if request.select is not None:
            self.calls.append(("ccorr", len(boxes)))
            thresh, min_k, _ = request.select
            r = R.record(cand, hess, self.sc["crop_boxes"][ids], self.sc["rates"][ids], valid, thresh, min_k, request.mode)
            out = inference.pack_candidate_correspondences(m, k, cand.shape[2], "cpu")
            for t, name in zip(out, R.FIELDS):
                t.copy_(torch.from_numpy(r[name]))
            fields = inference.record_fields(k, "candidate_correspondences", candidates=cand.shape[2])
            return inference.LoaderResult(m, k, {"candidate_correspondences": (out[5], fields)})
        self.calls.append(("cand", len(boxes)))
        assert request.refine == "get_final2" and request.cov_floor is None
        fields = inference.record_fields(k, "candidates_refined", False, False, cand.shape[2])
        packed = torch.zeros(m * sum(b for _, b in fields), dtype=torch.uint8)
        v = inference.record_views(packed, m, k, fields)
        for name, a in (("rates", self.sc["rates"][ids]), ("cand_hess", hess), ("cand", cand), ("boxes", self.sc["crop_boxes"][ids]),
                        ("valid", valid)):
            v[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return inference.LoaderResult(m, k, {"candidates_refined": (packed, fields)})


def _stub_poses(n_total, **kw):
    net = StubNet(n_total)
    frames = torch.zeros((max(n_total, 1), 2, 2), dtype=torch.uint8)
    boxes = [(i, 0, i + 10, 10) for i in range(n_total)]
    poses, rep = pipeline.candidate_poses(net, frames, boxes, net.sc["kp3d"], net.sc["K"], candidates=3, refine="get_final2",
                                          weights="hessian", thresh=0.45, min_k=6, on_fail="nan", return_report=True, threads=1, **kw)
    return net, np.array([np.concatenate(p) for p in poses]).reshape(n_total, 7), rep


def test_stub_device_select_equals_the_loader_path_without_a_group():
    """The glue of the two paths, no device: the solver's own row for the invalid crop equals the loader path's patched row."""
    n = 5
    net, want, wrep = _stub_poses(n, candidates_path="loader")
    assert net.calls == [("cand", n)]
    for kw in (dict(device_select=True), dict(device_select=True, distributed=True), dict(candidates_path="loader", distributed=True)):
        net, got, rep = _stub_poses(n, **kw)
        assert net.calls == [("cand" if "candidates_path" in kw else "ccorr", n)]
        assert R.same_bits(got, want) and R.same_bits(rep.raw, wrep.raw) and R.same_bits(rep.used, wrep.used), kw
        assert np.array_equal(rep.rescued, wrep.rescued)
    assert np.isnan(want[StubNet.BAD]).all() and wrep.raw[StubNet.BAD, 0] == 1.0 and wrep.raw[StubNet.BAD, 2] == 0.0
    assert wrep.rescued.any() and np.isfinite(np.delete(want, StubNet.BAD, 0)).all()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_total, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lo, hi = parallel.shard_bounds(n_total, world, rank)
        ok = True
        for kw, call in ((dict(device_select=True), "ccorr"), (dict(candidates_path="loader"), "cand")):
            _, want, wrep = _stub_poses(n_total, **kw)                              # distributed=False: the whole batch on this rank
            net, got, rep = _stub_poses(n_total, distributed=True, **kw)
            ok = ok and net.calls == ([(call, hi - lo)] if hi > lo else [])         # an empty shard makes no call
            ok = ok and R.same_bits(got, want) and R.same_bits(rep.raw, wrep.raw) and R.same_bits(rep.used, wrep.used)
            ok = ok and bool(np.array_equal(rep.rescued, wrep.rescued))
        # the sharded call itself: the record of the whole batch, as views
        net = StubNet(n_total)
        boxes = [(i, 0, i + 10, 10) for i in range(n_total)]
        frames = torch.zeros((n_total, 2, 2), dtype=torch.uint8)
        a = (frames, boxes, None, 64, "val", None, 0.229, None)
        want = StubNet(n_total)._loader(inference.LoaderRequest("get_final2", (3, 6), None, (0.45, 6, "hessian")), *a)
        got = parallel.sharded_frames_to_candidate_correspondences(net, frames, boxes, scale=64, refine="get_final2", candidates=3,
                                                                   thresh=0.45, min_k=6, weights="hessian")
        ok = ok and len(got) == 5 and all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and x.shape == y.shape
                                          for x, y in zip(got, [want[n] for n in R.FIELDS]))
        wantc = StubNet(n_total)._loader(inference.LoaderRequest("get_final2", (3, 6)), *a)
        gotc = parallel.sharded_frames_to_candidates(StubNet(n_total), frames, boxes, scale=64, candidates=3, refine="get_final2",
                                                     return_hessian=True)
        ok = ok and len(gotc) == 5 and all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and x.shape == y.shape
                                           for x, y in zip(gotc, [wantc[n] for n in ("cand", "boxes", "rates", "valid", "cand_hess")]))
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_total", [6, 5, 1])          # even split, uneven tail, an EMPTY shard on rank 1
def test_candidate_poses_distributed_world2(n_total):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_total, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(res) == [(0, True), (1, True)]
