"""Data-parallel crop sharding over the GPUs of one node (one process per GPU, RCCL/xGMI).

The reference's only multi-GPU mechanism is single-process nn.DataParallel, which gathers the
full [N,K,H,W] heatmaps onto GPU 0 (main.py:254, val.py:382; 92 MB per rank at batch 32).  Crops
are independent through the whole path, so here every rank runs its contiguous
slice of the batch and the ONLY exchange is one all-gather of the per-rank [n_local, K, 3]
keypoints (132 B per crop at K=11) before the host-side PnP — latency-bound, no ring tuning.
Uneven tails are padded to the largest shard and trimmed after the gather.

The device path (net.frames_to_keypoints / net.frames_to_correspondences: loader, decoder, top-k rule and back-projection
on the device) is sharded the same way, by boxes: sharded_frames_to_keypoints / sharded_frames_to_correspondences run a
rank's boxes through the net's one-call entry points and exchange the PACKED RECORD those calls write (inference.record_fields)
with one all-gather of bytes per record; the field-major blocks are put in batch order by one kernel
(esahrnet_gather_records, gather_records).  The candidates go the same way: sharded_frames_to_candidates gathers the candidates
record, sharded_frames_to_candidate_correspondences the one record the repairing solve consumes (one all-gather, one kernel).
Nothing of this has run on more than one GPU yet, and no time has been measured.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.distributed as dist

from .crops import STD


def shard_bounds(n_total: int, world_size: int, rank: int):
    """Contiguous split; the first (n_total % world_size) ranks get one extra crop."""
    base, extra = divmod(n_total, world_size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def gather_keypoints(local_kp: torch.Tensor, n_total: int, group=None) -> torch.Tensor:
    """local_kp [n_local, K, 3] (this rank's shard, rank order = crop order) -> [n_total, K, 3]
    on every rank.  One all_gather (RCCL on GPU tensors, gloo on CPU tensors)."""
    if not (dist.is_available() and dist.is_initialized()):
        if local_kp.shape[0] != n_total:
            raise ValueError("no process group but shard size != batch size")
        return local_kp
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    lo, hi = shard_bounds(n_total, world, rank)
    if local_kp.shape[0] != hi - lo:
        raise ValueError(f"rank {rank}: shard has {local_kp.shape[0]} crops, expected {hi - lo}")
    n_max = -(-n_total // world)
    k = local_kp.shape[1]
    padded = local_kp.new_zeros((n_max, k, 3))
    padded[: hi - lo] = local_kp
    flat = local_kp.new_empty((world * n_max, k, 3))
    dist.all_gather_into_tensor(flat, padded.contiguous(), group=group)
    out = flat.view(world, n_max, k, 3)
    parts = []
    for r in range(world):
        a, b = shard_bounds(n_total, world, r)
        parts.append(out[r, : b - a])
    return torch.cat(parts, 0)


def sharded_keypoints(net, crops: torch.Tensor, group=None, keypoints_fn=None, keypoints_only: bool = False,
                      refine: str = "get_final") -> torch.Tensor:
    """Every rank holds (or can index) the full batch `crops` [N,Cin,H,W]; each runs its slice
    through `net` + the fused keypoint kernel and all ranks return the full [N,K,3].
    `keypoints_fn` (default: inference.heatmaps_to_keypoints, GPU only) maps the rank's heat-maps to [n,K,3].
    keypoints_only=True: the rank's slice goes through net(x, output="keypoints") (no heat-maps; keypoints_fn unused).
    refine="get_final2": the second decoder (inference.get_final2), passed on as refine= to the net or to keypoints_fn;
    refine="gaussfit": the Gaussian-fit decoder, passed on the same way."""
    from .inference import check_refine
    check_refine(refine)
    rk = {} if refine == "get_final" else {"refine": refine}
    if keypoints_fn is None:
        from .inference import heatmaps_to_keypoints as keypoints_fn
    heatmaps_to_keypoints = keypoints_fn
    n_total = crops.shape[0]
    if dist.is_available() and dist.is_initialized():
        lo, hi = shard_bounds(n_total, dist.get_world_size(group), dist.get_rank(group))
    else:
        lo, hi = 0, n_total
    k = net.num_keypoints
    if hi > lo and keypoints_only:
        kp = net(crops[lo:hi], output="keypoints", **rk)
    elif hi > lo:
        kp = heatmaps_to_keypoints(net(crops[lo:hi]), **rk)
    else:
        kp = crops.new_zeros((0, k, 3))
    return gather_keypoints(kp, n_total, group)


# ---- the device path: shard the boxes, gather the packed records -----------------------------------------------------------
def _field_bytes(fields):
    """fields as inference.record_fields gives them, ((name, bytes per crop), ...), or bare byte counts -> [bytes per crop]."""
    fb = [int(f[1]) if isinstance(f, (tuple, list)) else int(f) for f in fields]
    if not fb or any(b < 4 or b % 4 for b in fb):
        raise ValueError(f"every field of a record is a positive multiple of 4 bytes per crop, got {fb}")
    return fb


def _check_gathered(gathered, world, n_total, fb):
    n_max = -(-n_total // world)
    if not (isinstance(gathered, torch.Tensor) and gathered.dtype == torch.uint8 and gathered.dim() == 1 and
            gathered.is_contiguous() and gathered.numel() == world * n_max * sum(fb)):
        raise ValueError(f"expected {world} blocks of {n_max} crops x {sum(fb)} bytes in one contiguous uint8 tensor")
    return n_max


def gather_records_slicing(gathered: torch.Tensor, world: int, n_total: int, fields) -> torch.Tensor:
    """`world` blocks, each a packed record laid out for n_max = ceil(n_total / world) crops with rank r's shard in the first
    hi_r - lo_r slots of every field (what all_gather_into_tensor leaves behind) -> the packed record of the n_total crops, by
    plain slicing: world x fields small copies.  The form the CPU (gloo) path uses, and the statement esahrnet_gather_records
    is held to.  Padding slots and the blocks of empty shards are not read."""
    fb = _field_bytes(fields)
    if world < 1 or n_total < 1:
        raise ValueError(f"world = {world}, n_total = {n_total}: both at least 1")
    n_max = _check_gathered(gathered, world, n_total, fb)
    per = sum(fb)
    blocks = gathered.view(world, n_max * per)
    out = gathered.new_empty(n_total * per)
    before = 0
    for b in fb:
        for r in range(world):
            lo, hi = shard_bounds(n_total, world, r)
            if hi > lo:
                out[n_total * before + lo * b:n_total * before + hi * b] = blocks[r, n_max * before:n_max * before + (hi - lo) * b]
        before += b
    return out


def gather_records_device(gathered: torch.Tensor, world: int, n_total: int, fields) -> torch.Tensor:
    """gather_records_slicing on the device: ONE launch of gather_records_kernel (include/esahrnet.h esahrnet_gather_records)
    on the current stream, whatever world and the number of fields; byte-identical to the slicing form."""
    from . import _lib
    fb = _field_bytes(fields)
    if not (isinstance(gathered, torch.Tensor) and gathered.is_cuda):
        raise RuntimeError("gather_records_device runs on the GPU only (gather_records_slicing is the host form)")
    if world >= 1 and n_total >= 1:
        _check_gathered(gathered, world, n_total, fb)
    arr = (C.c_int * len(fb))(*fb)
    with torch.cuda.device(gathered.device):
        out = torch.empty(max(n_total, 0) * sum(fb), dtype=torch.uint8, device=gathered.device)
        stream = torch.cuda.current_stream(gathered.device).cuda_stream
        _lib.check(_lib.lib().esahrnet_gather_records(gathered.data_ptr(), int(world), int(n_total), arr, len(fb), out.data_ptr(),
                                                      C.c_void_p(stream)))
    return out


def _repack(local, n_local, n_max, fb):
    """A record laid out for n_local crops -> a block laid out for n_max crops (the padding slots stay uninitialised: nobody
    reads them).  esahrnet_gather_records maps n_max-blocks to the n_total layout, and with world = 1 those two are the same
    layout, so it cannot widen a record: this is plain slicing, one small copy per field, and only on the ranks whose shard is
    one short of the largest (a rank with n_local == n_max sends its buffer as it is)."""
    if n_local == n_max:
        return local
    block = local.new_empty(n_max * sum(fb))
    before = 0
    for b in fb:
        block[n_max * before:n_max * before + n_local * b] = local[n_local * before:n_local * before + n_local * b]
        before += b
    return block


def gather_records(local_packed, n_local: int, n_total: int, fields, group=None, device=None) -> torch.Tensor:
    """This rank's packed record (uint8, laid out for its n_local crops as `fields` = inference.record_fields(...) says; None
    when n_local == 0) -> the packed record of the whole batch on every rank, crops in rank order.  Without a process group the
    input is returned.  With one: the record is widened to the largest shard's layout, ONE all_gather_into_tensor of uint8
    moves it (RCCL on GPU tensors, gloo on CPU tensors), and the gathered blocks are put in batch order by one kernel launch on
    GPU tensors (gather_records_device) or by slicing on CPU tensors (gather_records_slicing).  `device`: where an empty
    shard's block lives (default: the current GPU under the nccl backend, else the CPU)."""
    fb = _field_bytes(fields)
    per = sum(fb)
    if local_packed is not None and not (isinstance(local_packed, torch.Tensor) and local_packed.dtype == torch.uint8 and
                                         local_packed.dim() == 1 and local_packed.numel() == n_local * per):
        raise ValueError(f"a record of {n_local} crops is a uint8 tensor of {n_local * per} bytes")
    if not (dist.is_available() and dist.is_initialized()):
        if n_local != n_total or local_packed is None:
            raise ValueError("no process group but shard size != batch size")
        return local_packed
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    lo, hi = shard_bounds(n_total, world, rank)
    if n_local != hi - lo or (local_packed is None) != (n_local == 0):
        raise ValueError(f"rank {rank}: shard has {n_local} crops, expected {hi - lo}")
    n_max = -(-n_total // world)
    if local_packed is None:
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
        block = torch.empty(n_max * per, dtype=torch.uint8, device=device)
    else:
        block = _repack(local_packed.contiguous(), n_local, n_max, fb)
    flat = block.new_empty(world * n_max * per)
    dist.all_gather_into_tensor(flat, block, group=group)
    if flat.is_cuda:
        return gather_records_device(flat, world, n_total, fb)
    return gather_records_slicing(flat, world, n_total, fb)


def _shard_of(n_total, group):
    if dist.is_available() and dist.is_initialized():
        return shard_bounds(n_total, dist.get_world_size(group), dist.get_rank(group))
    return 0, n_total


def _shard_args(det_boxes, frame_idx, lo, hi, n_total, frame_base):
    """The boxes of this rank and the frame of each, counted from the first frame the rank holds.  frame_idx=None means
    "box i lies on frame i of the BATCH", so a shard names its frames: lo .. hi - 1."""
    if (lo, hi, frame_base) == (0, n_total, 0):
        return det_boxes, frame_idx                         # the whole batch on this rank: the net's own call
    if frame_idx is None:
        idx = list(range(lo - frame_base, hi - frame_base))
    elif isinstance(frame_idx, torch.Tensor):
        idx = frame_idx[lo:hi] - frame_base
    else:
        idx = [int(f) - frame_base for f in frame_idx[lo:hi]]
    return det_boxes[lo:hi], idx


def _sharded_loader(net, request, frames, det_boxes, frame_idx, group, frame_base, scale, rule, mean, std, pixel_format, gather=None):
    """net._loader over the ranks of `group` -> the LoaderResult of the whole batch on every rank: rank r runs boxes [lo_r, hi_r)
    through net._loader, one call (none on an empty shard), and each record named in `gather` (default: every record of the
    request) is exchanged by one gather_records.  The request has made its checks before any shard work starts."""
    from .inference import LoaderResult
    k, n_total = net.num_keypoints, len(det_boxes)
    fields = request.fields(k)
    lo, hi = _shard_of(n_total, group)
    local = None
    if hi > lo:
        boxes, idx = _shard_args(det_boxes, frame_idx, lo, hi, n_total, frame_base)
        local = net._loader(request, frames, boxes, idx, scale, rule, mean, std, pixel_format)
    return LoaderResult(n_total, k, {kind: (gather_records(None if local is None else local.records[kind][0], hi - lo, n_total,
                                                           fields[kind], group, device=frames.device), fields[kind])
                                     for kind in (request.kinds if gather is None else gather)})


def sharded_frames_to_keypoints(net, frames, det_boxes, frame_idx=None, *, group=None, frame_base: int = 0, scale: int = 256,
                                rule: str = "val", refine: str = "get_final", mean=None, std: float = STD, pixel_format=None,
                                return_cov: bool = False, cov_floor: float = 1e-6):
    """net.frames_to_keypoints over the ranks of `group`: EVERY rank passes the full list of boxes (and frame indices); rank r
    runs boxes [lo_r, hi_r) (shard_bounds) through net._loader, one library call, and the packed records are
    gathered (gather_records: one all-gather, one kernel).  Every rank returns the whole batch's (kp f32 [m,K,3], crop_boxes
    int32 [m,4], rates f64 [m], valid int32 [m]) as views of one packed buffer, the bits the single-device call gives;
    refine="gaussfit" appends (fit f64 [m,K,8], status int32 [m,K], hess f64 [m,K,3]) and return_cov=True (gaussfit only)
    (cov, info) f64 [m,K,3] behind them.  frame_idx=None: box i lies on frame i of the batch.  `frames`: the whole batch's
    frames, or only the frames this rank holds with frame_base = b: frames[0] is batch frame b and the indices are rebased by
    -b; an index that falls outside gives valid = 0 and NaN rows, as it does on one device.  Other keywords as
    net.frames_to_keypoints.  An empty shard makes no library call."""
    from .inference import LoaderRequest
    if return_cov and refine != "gaussfit":
        raise ValueError("return_cov=True needs refine='gaussfit': only the Gaussian fit has a parameter covariance")
    request = LoaderRequest(refine, None, cov_floor if return_cov else None)
    r = _sharded_loader(net, request, frames, det_boxes, frame_idx, group, int(frame_base), scale, rule, mean, std, pixel_format)
    return tuple(r[n] for n in ("kp", "boxes", "rates", "valid", "fit", "status", "hess", "cov", "info") if n in r)


def sharded_frames_to_correspondences(net, frames, det_boxes, frame_idx=None, *, group=None, frame_base: int = 0,
                                      scale: int = 256, rule: str = "val", refine: str = "get_final", thresh: float = 0.8,
                                      min_k: int = 24, weights: str = "peak", mean=None, std: float = STD, pixel_format=None,
                                      cov_floor: float = 1e-6):
    """net.frames_to_correspondences over the ranks of `group`, under the contract of sharded_frames_to_keypoints (full box
    list on every rank, rank r runs boxes [lo_r, hi_r), frame_idx=None and frame_base as there): -> (count int32 [m], order
    int32 [m,K], pts f64 [m,K,2], w f64 [m,K,3], kp, crop_boxes, rates, valid) of the whole batch on every rank, the bits of the
    single-device call.  TWO records are gathered, the correspondence record (the first four) and the keypoint record (the
    last four): two all-gathers and two kernel launches per step."""
    from .inference import LoaderRequest
    request = LoaderRequest(refine, None, cov_floor if weights == "covariance" else None, (thresh, min_k, weights))
    r = _sharded_loader(net, request, frames, det_boxes, frame_idx, group, int(frame_base), scale, rule, mean, std, pixel_format)
    return r["count"], r["order"], r["pts"], r["w"], r["kp"], r["boxes"], r["rates"], r["valid"]


def sharded_frames_to_candidates(net, frames, det_boxes, frame_idx=None, *, group=None, frame_base: int = 0, scale: int = 256,
                                 rule: str = "val", candidates: int = 3, nms_radius: int = 6, mean=None, std: float = STD,
                                 pixel_format=None, refine: str = "get_final", return_hessian: bool = False,
                                 return_fit: bool = False, return_cov: bool = False, cov_floor: float = 1e-6):
    """net.frames_to_candidates over the ranks of `group`, under the contract of sharded_frames_to_keypoints (full box list on
    every rank, rank r runs boxes [lo_r, hi_r), frame_idx=None and frame_base as there, no library call on an empty shard): the
    "candidates" record, or with a refine other than "get_final" the "candidates_refined" record, is gathered (one all-gather, one
    kernel) and every rank returns what net.frames_to_candidates returns for the whole batch, the bits of the single-device call."""
    from . import inference
    inference._check_at_outputs(refine, return_hessian, return_fit, return_cov, cov_floor)
    request = inference.LoaderRequest(refine, (candidates, nms_radius), cov_floor if return_cov else None)
    r = _sharded_loader(net, request, frames, det_boxes, frame_idx, group, int(frame_base), scale, rule, mean, std, pixel_format)
    return inference.candidate_returns(r, return_hessian, return_fit, return_cov)


def sharded_frames_to_candidate_correspondences(net, frames, det_boxes, frame_idx=None, *, group=None, frame_base: int = 0,
                                                scale: int = 256, rule: str = "val", refine: str = "get_final",
                                                candidates: int = 3, nms_radius: int = 6, thresh: float = 0.8, min_k: int = 24,
                                                weights: str = "peak", mean=None, std: float = STD, pixel_format=None,
                                                cov_floor: float = 1e-6):
    """net.frames_to_candidate_correspondences over the ranks of `group`, under the contract of sharded_frames_to_keypoints: ->
    (cpts f64 [m,K,M,2], cw f64 [m,K,M,3], cpeak f32 [m,K,M], count int32 [m], order int32 [m,K]) of the whole batch on every rank,
    the bits of the single-device call.  ONE record is gathered, the one pnp.candidate_correspondences_to_pose_batch consumes: one
    all-gather and one kernel launch per step; the candidates record stays on the rank that decoded it."""
    from .inference import LoaderRequest, check_cov_floor
    request = LoaderRequest(refine, (candidates, nms_radius), cov_floor if weights == "covariance" else None,
                            (thresh, min_k, weights))
    check_cov_floor(cov_floor)              # (refused whatever the weights, as on one device)
    r = _sharded_loader(net, request, frames, det_boxes, frame_idx, group, int(frame_base), scale, rule, mean, std, pixel_format,
                        gather=("candidate_correspondences",))
    return r["cpts"], r["cw"], r["cpeak"], r["count"], r["order"]


# ---- the measurement protocol of bench.py, importable so that the N > 1 branch runs under gloo on the CPU too ----
def make_sharded_step(local_step, n_total: int, group=None):
    """step() = this rank's shard through `local_step` (eager forward + keypoints, or a HIP-graph replay that
    returns its static output tensor), then the path's one exchange: the keypoint all-gather."""
    def step():
        return gather_keypoints(local_step(), n_total, group)
    return step


def timed_steps(step, steps: int, warmup: int, sync=None, device=None, group=None):
    """W untimed steps, then exactly K steps bracketed by (device sync + barrier) on both sides; returns
    (elapsed seconds = MAX over ranks, output of the last step).  `sync`: callable draining the device
    (torch.cuda.synchronize on a GPU, nothing on the CPU)."""
    import time
    sync = sync or (lambda: None)
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    out = None
    for _ in range(warmup):
        out = step()
    sync()
    if multi:
        dist.barrier(group)
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    sync()
    if multi:
        dist.barrier(group)
    elapsed = time.perf_counter() - t0
    if multi:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        elapsed = float(t.item())
    return elapsed, out
