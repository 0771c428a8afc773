"""Batch-N evaluation / submission driver (SURVEY.md §8f NEXT-4).

Reference being mirrored: the per-image loop of val.py:136-233 (batch 1, >=150 blocking .item() reads
per image) and submission.py:6-52.  Here: frames and detector boxes in, poses out, N crops at a time:
  crops.crop_batch -> net -> inference.heatmaps_to_keypoints -> (parallel.gather_keypoints) -> ONE D2H
  copy of [N, K, 3] -> host: top-k, back-projection, EPnP + RANSAC, peak-weighted refinement, quaternion.
`SubmissionWriter` keeps the reference's API and CSV format (filename, q0..q3, r0..r2, sorted by name).
"""
from __future__ import annotations

import contextlib
import csv
import logging
import os
from concurrent.futures import ProcessPoolExecutor
from datetime import datetime

import numpy as np
import torch

from . import crops, inference, parallel, pnp

logger = logging.getLogger(__name__)


class SubmissionWriter:
    """Collects (filename, q, r) rows and writes the ESA submission CSV.

    Same interface and same file, byte for byte, as the reference's writer (submission.py:6-52; pinned by
    tests/golden/submission_*.csv, which tests/golden/make_submission_golden.py produced by running the
    reference's class): one row `filename,q0,q1,q2,q3,r0,r1,r2` per image, the synthetic test set first and the
    real test set after it, each sorted by filename (stable, so duplicates keep their insertion order), values
    written with csv's default str() formatting, '\n' line ends.  `run_submission` only needs the two append
    methods, so the reference's own writer object can be passed in its place."""

    def __init__(self):
        self._rows = {False: [], True: []}          # real? -> [(filename, [q0..q3, r0..r2])]

    # the reference exposes the two lists; keep them readable for callers that look at them
    @property
    def test_results(self):
        return [{'filename': f, 'q': v[:4], 'r': v[4:]} for f, v in self._rows[False]]

    @property
    def real_test_results(self):
        return [{'filename': f, 'q': v[:4], 'r': v[4:]} for f, v in self._rows[True]]

    def append_test(self, filename, q, r):
        self._rows[False].append((filename, list(q) + list(r)))

    def append_real_test(self, filename, q, r):
        self._rows[True].append((filename, list(q) + list(r)))

    def export(self, out_dir='', suffix=None):
        if suffix is None:
            suffix = datetime.now().strftime("%Y%m%d-%H%M")
        path = os.path.join(out_dir, f'submission_{suffix}.csv')
        with open(path, 'w') as f:
            out = csv.writer(f, lineterminator='\n')
            for real in (False, True):
                for name, values in sorted(self._rows[real], key=lambda row: row[0]):
                    out.writerow([name, *values])
        return path


def _blas_single_thread():
    """The PnP stage is thousands of 6x6 .. 12x12 LAPACK calls: a multi-threaded BLAS spends its time waking
    threads (measured 62 ms vs 4.5 ms per image with OpenBLAS on 8 cores), so it runs single-threaded."""
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1)
    except Exception:                                   # noqa: BLE001 - optional dependency
        return contextlib.nullcontext()


def _pose_job(args):
    kp, kp3d, K, xy, rate, thresh, min_k = args
    with _blas_single_thread():
        q, t, _ = pnp.keypoints_to_pose(kp, kp3d, K, xy, rate, thresh=thresh, min_k=min_k)
    return q, t


def poses_from_keypoints(kp, boxes, rates, kp3d, K, thresh: float = 0.8, min_k: int = 24, pool=None,
                         native: bool = True, threads: int = 0, report: bool = False):
    """Host stage of val.py:172-224 for a batch: kp [N,K,3] (numpy) -> list of (q [w,x,y,z], t).
    native=True: the C++ solver of the library (`esahrnet_pnp_batch`, `threads` worker threads, ~100 us per image
    and thread); native=False: the numpy restatement it is tested against (optionally over a process `pool`).
    report=True (native only): -> (poses, pnp.PoseReport)."""
    K = np.asarray(K, np.float64)
    if report:
        if not native:
            raise ValueError("the pose report comes from the native solver (native=False has none)")
        q, t, rep = pnp.keypoints_to_pose_batch(kp, kp3d, K, [(b[0], b[1]) for b in boxes], rates, thresh, min_k, threads, report=True)
        return [(q[i], t[i]) for i in range(len(boxes))], rep
    if native:
        q, t = pnp.keypoints_to_pose_batch(kp, kp3d, K, [(b[0], b[1]) for b in boxes], rates, thresh, min_k, threads)
        return [(q[i], t[i]) for i in range(len(boxes))]
    jobs = [(kp[i], kp3d, K, (boxes[i][0], boxes[i][1]), rates[i], thresh, min_k) for i in range(len(boxes))]
    if pool is not None:
        return list(pool.map(_pose_job, jobs, chunksize=max(1, len(jobs) // 32)))
    return [_pose_job(j) for j in jobs]


def pose_pool(workers: int):
    """Process pool for the host PnP stage (images are independent)."""
    return ProcessPoolExecutor(max_workers=workers)


FALLBACK_POSE = ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 10.0))   # identity attitude, 10 m down the boresight


CANDIDATES_PATHS = ("heatmaps", "fused", "loader")


class PoseFailure(ValueError):
    """No pose for an image (fewer than 4 usable keypoints, RANSAC found no consensus, or a gate of estimate_poses withdrew it)."""


def estimate_poses(net, frames: torch.Tensor, bboxes, kp3d, K, scale: int = 256, thresh: float = 0.8,
                   min_k: int = 24, distributed: bool = False, pool=None, native: bool = True,
                   on_fail: str = "raise", keypoints_only: bool = False, refine: str = "get_final",
                   device_loader: bool = False, frame_idx=None, rule: str = "val", device_select: bool = False,
                   weights: str = "peak", threads: int = 0, cov_floor: float = 1e-6, return_report: bool = False,
                   max_rms_px=None, min_inliers=None, candidates: int = 1, nms_radius: int = 6, min_ratio: float = 0.3,
                   candidates_path: str = "heatmaps"):
    """One batch of the val.py:136-233 loop.  frames uint8 cuda [N,H,W]; bboxes N x (x, y, x2, y2);
    kp3d [K3, 3] model keypoints; K camera matrix.  -> list of (q [w,x,y,z], t) per image.
    An image without a solution (the native solver reports it as a NaN row; the reference would die inside
    cv2.solvePnPRansac) raises PoseFailure, or with on_fail="nan" is returned as the NaN row for the caller to
    deal with — it is never passed on silently.  keypoints_only=True: the net goes straight to keypoints
    (net(x, output="keypoints"): the same bits, no heat-maps written).  refine="get_final2": the reference's second
    decoder (inference.get_final2: blur + full-Hessian step) instead of get_final.
    device_loader=True: net.frames_to_keypoints does the box rule (`rule`: "val" / "train"), the crops, the forward and the
    decoder in one library call; keypoints, crop boxes, rates and valid flags come back in ONE device->host copy of one
    packed buffer.  bboxes are integers then, several may lie on one frame (frame_idx[i] = frame of box i; frames may be RGB
    [N,H,W,3]), and a crop the loader could not make (empty box, frame index out of range) has no pose: on_fail applies.
    device_select=True (implies the device loader): net.frames_to_correspondences also does the top-k rule, the ordering and
    the back-projection of val.py:172-180 on the device; ONE device->host copy of the correspondence record (count, order,
    image points, 2x2 weights), then the native solver on it (pnp.correspondences_to_pose_batch).  `threads`: worker threads of
    the native solver on every path (0: one per available CPU, at most 16).
    weights="peak" (default): the poses of device_loader=True, bit for bit.  weights="hessian" (device_select=True and
    refine="get_final2" or "gaussfit"): the refinement weighs each point by the decoder's Hessian, rate * (-H)^(1/2), the
    anisotropic weight uncertainty_pnp.cpp:30-31 takes, instead of the scalar peak.  refine="gaussfit": the Gaussian-fit decoder
    (inference.gaussfit_keypoints) on every path; device_loader=True still fetches one packed buffer (the decoder's fit, Hessian
    and status ride in it, inference.packed_layout).  weights="covariance" (device_select=True and refine="gaussfit"): each point
    is weighed by the covariance of its fitted centre, rate * cov^(-1/2) (inv(sqrtm(covar)) of the reference's
    evaluation.py:471-487), which grows with the residual noise of the fit and not only with the blob's width; a point with
    cov[0] < cov_floor or without a covariance gets weight zero.
    distributed=True with device_loader=True or device_select=True: every rank passes the whole batch (frames, bboxes,
    frame_idx), runs its contiguous shard of the boxes through the same library call and the packed records are all-gathered
    (parallel.sharded_frames_to_keypoints / sharded_frames_to_correspondences); every rank returns all poses.
    return_report=True (native paths): -> (poses, report), report a pnp.PoseReport with one entry per image: status, inliers,
    RANSAC and LM iterations, final cost, rms / max reprojection error in pixels, minimal depth and the 6x6 covariance of the
    pose (report.covariance()); the poses are the ones of the call without it, bit for bit.  Gates: a solved pose whose rms_px
    exceeds max_rms_px or whose inliers are fewer than min_inliers is treated exactly like "no pose" — a NaN row, on_fail
    applies — while its report row keeps the real numbers and report.gated marks it; both default to None (no gate).  With
    device_loader=True a crop the loader could not make has a report row of status 1 with n = 0.
    candidates=M > 1 (heat-map path, native solver, refine="get_final"): the decoder keeps the M best peaks of every heat-map
    (inference.heatmaps_to_candidates, `nms_radius` pixels apart), ONE device->host copy of them, and the native solve swaps a
    runner-up with at least `min_ratio` of the primary's peak in where the RANSAC consensus pose says the primary is wrong
    (pnp.candidates_to_pose_batch; the report then carries .used and .rescued).  It is refused together with keypoints_only,
    device_loader, device_select, distributed, native=False and any other refine; candidates=1 leaves every path as it is.
    candidates_path (with candidates > 1 only) says where the runner-ups are decoded: "heatmaps" (default) as above; "fused":
    host crops, then net.candidates(x, M, nms_radius), the decoder in the forward, no heat-map tensor in caller memory; "loader":
    net._loader does the box rule, the crops, the forward and the candidate decoder in one library call and ONE device->host
    copy of its packed buffer feeds the solve — bboxes are integers, frame_idx and rule are accepted and an invalid crop has no
    pose, as with device_loader=True.  The poses, .used and .rescued are those of "heatmaps", bit for bit."""
    inference.check_refine(refine)
    inference.check_weights(weights, refine)
    want = return_report or max_rms_px is not None or min_inliers is not None
    if candidates_path not in CANDIDATES_PATHS:
        raise ValueError(f"candidates_path must be one of {CANDIDATES_PATHS}, got {candidates_path!r}")
    if candidates == 1 and candidates_path != "heatmaps":
        raise ValueError(f"candidates_path={candidates_path!r} belongs to candidates > 1 (candidates=1 decodes no runner-up)")
    if candidates != 1:
        for name, on in (("keypoints_only", keypoints_only), ("device_loader", device_loader), ("device_select", device_select),
                         ("distributed", distributed), ("native=False", not native), (f"refine='{refine}'", refine != "get_final")):
            if on:
                raise ValueError(f"candidates={candidates} is not available with {name}: runner-up peaks are decoded on the "
                                 "heat-map path (get_final) and solved by the native entry")
    if want and not native:
        raise ValueError("return_report and the max_rms_px / min_inliers gates read the native solver's report (native=False has none)")
    if weights != "peak" and not device_select:
        raise ValueError(f"weights='{weights}' belongs to device_select=True (the host selection weighs by the peak)")
    if device_select and not native:
        raise ValueError("device_select=True hands its record to the native solver (native=False has no entry for it)")

    # the solve on decoded rows, solve(rows, boxes, rates) -> (poses, report or None); the paths differ in where the rows come from
    def keypoint_poses(kp, boxes, rates):
        poses = poses_from_keypoints(kp, boxes, rates, kp3d, K, thresh, min_k, pool, native, threads, report=want)
        return poses if want else (poses, None)

    def candidate_poses(cand, boxes, rates):
        q, t, _, *rep = pnp.candidates_to_pose_batch(cand, kp3d, np.asarray(K, np.float64), [(b[0], b[1]) for b in boxes], rates,
                                                     thresh, min_k, min_ratio, threads, report=want)
        return [(q[i], t[i]) for i in range(len(boxes))], rep[0] if want else None

    solve = keypoint_poses if candidates == 1 else candidate_poses
    if device_select:
        poses, rep = _device_select_poses(net, frames, bboxes, frame_idx, distributed, scale, rule, refine, thresh, min_k, weights,
                                          cov_floor, kp3d, K, threads, want)
    elif device_loader:
        poses, rep = _device_loader_poses(net, frames, bboxes, frame_idx, distributed, scale, rule, refine, solve)
    elif candidates != 1 and candidates_path == "loader":
        poses, rep = _loader_candidates_poses(net, frames, bboxes, frame_idx, scale, rule, candidates, nms_radius, "get_final", "peak",
                                              None, lambda rows, boxes, rates, hess: solve(rows, boxes, rates))
    else:
        poses, rep = _host_crops_poses(net, frames, bboxes, frame_idx, scale, rule, refine, distributed, keypoints_only,
                                       candidates, nms_radius, candidates_path, solve)
    if want:
        poses = _gated_poses(poses, rep, max_rms_px, min_inliers)
    poses = _checked_poses(poses, on_fail)
    return (poses, rep) if return_report else poses


def candidate_poses(net, frames: torch.Tensor, bboxes, kp3d, K, candidates: int = 3, refine: str = "get_final2",
                    weights: str = "hessian", nms_radius: int = 6, min_ratio: float = 0.3, scale: int = 256, thresh: float = 0.8,
                    min_k: int = 24, on_fail: str = "raise", return_report: bool = False, max_rms_px=None, min_inliers=None,
                    cov_floor: float = 1e-6, threads: int = 0, candidates_path: str = "heatmaps", frame_idx=None, rule: str = "val",
                    device_select: bool = False, distributed: bool = False):
    """Runner-up repair AND anisotropic weights, the combination estimate_poses refuses (its candidates=M is get_final with peak
    weights; its weights="hessian" / "covariance" know the arg-max only).  frames, bboxes, kp3d, K, scale, thresh, min_k, on_fail,
    the report and the gates as in estimate_poses -> list of (q, t) per image[, report with .used and .rescued].
    Host crops as on the "heatmaps" path (crops.crop_batch), then inference.heatmaps_to_candidates(net(x), candidates, nms_radius,
    refine=refine, ...): every candidate of every heat-map is refined by `refine` at its own pixel and carries the decoder's
    Hessian (weights="hessian": refine "get_final2" or "gaussfit") or the information of its fitted centre (weights="covariance":
    refine="gaussfit"), ONE device->host copy of candidates and weights, then pnp.candidates_to_pose_batch(..., hess=...): the
    repair step of estimate_poses(candidates=M), with every point, a swapped-in runner-up included, weighed by
    rate * (-H)^(1/2) in the refinement.  weights="peak" passes no Hessian; with refine="get_final" that is
    estimate_poses(..., candidates=M), bit for bit.
    candidates_path says where the candidates are decoded, as in estimate_poses: "heatmaps" (default) as above; "fused": host
    crops, then net.candidates(x, candidates, nms_radius, refine=refine, ...), search and refinement inside the forward's one
    library call, no heat-map tensor in caller memory; "loader": net._loader (candidates=(M, nms_radius), refine=refine) does the box rule,
    the crops, the forward and the refined candidates in one library call and ONE device->host copy of its packed record
    (inference.record_fields(K, "candidates_refined", ...)) feeds the same solve with the loader's boxes and rates -- bboxes are
    integers, frame_idx and rule are accepted, and a crop the loader could not make has the NaN pose: on_fail applies, its report
    row is that of "fewer than 4" with n = 0.  The poses, the report, .used and .rescued are those of "heatmaps", bit for bit.
    device_select=True (implies the loader; candidates_path stays at its default): net._loader, asked for a select, also
    does the top-k rule, the ordering, the back-projection and the 2x2 weight of EVERY candidate on the device
    (esahrnet_correspondences_cand behind the loader's call), ONE device->host copy of that one record
    (inference.record_fields(K, "candidate_correspondences", candidates=M)), then pnp.candidate_correspondences_to_pose_batch: the
    same solve and repair on image points.  bboxes, frame_idx and rule as with "loader"; a crop the loader could not make has
    count 0, so the solver itself answers the NaN pose and the report row of status 1 with n = 0.  The poses, the report, .used and
    .rescued are those of candidates_path="loader", bit for bit.
    distributed=True (with device_select=True or candidates_path="loader"): every rank passes the whole batch, runs its contiguous
    shard of the boxes and the packed record is all-gathered (parallel.sharded_frames_to_candidate_correspondences /
    sharded_frames_to_candidates: one record, one all-gather); every rank returns all poses."""
    inference.check_refine(refine)
    mode = inference.check_weights(weights, refine)
    cov_floor = inference.check_cov_floor(cov_floor)
    if candidates_path not in CANDIDATES_PATHS:
        raise ValueError(f"candidates_path must be one of {CANDIDATES_PATHS}, got {candidates_path!r}")
    if device_select and candidates_path != "heatmaps":
        raise ValueError(f"candidates_path={candidates_path!r} does not go with device_select=True, which decodes in the loader and "
                         "selects on the device: leave candidates_path at its default")
    if distributed and not (device_select or candidates_path == "loader"):
        raise ValueError("distributed=True belongs to device_select=True or candidates_path='loader' (the sharded paths gather the "
                         "loader's packed records)")
    if candidates_path != "loader" and not device_select and (frame_idx is not None or rule != "val"):
        raise ValueError("frame_idx and rule belong to candidates_path='loader' (crops.crop_batch: one val box per frame)")
    want = return_report or max_rms_px is not None or min_inliers is not None
    ask = {"return_hessian": weights == "hessian", "return_cov": weights == "covariance", "cov_floor": cov_floor}

    def solve(cand, boxes, rates, hess):
        q, t, _, *rep = pnp.candidates_to_pose_batch(cand, kp3d, np.asarray(K, np.float64), [(b[0], b[1]) for b in boxes], rates,
                                                     thresh, min_k, min_ratio, threads, report=want, hess=hess)
        return [(q[i], t[i]) for i in range(len(boxes))], rep[0] if want else None

    if device_select:
        poses, rep = _device_select_candidate_poses(net, frames, bboxes, frame_idx, distributed, scale, rule, refine, candidates,
                                                    nms_radius, thresh, min_k, weights, cov_floor, kp3d, K, min_ratio, threads, want)
    elif candidates_path == "loader":
        poses, rep = _loader_candidates_poses(net, frames, bboxes, frame_idx, scale, rule, candidates, nms_radius, refine, weights,
                                              cov_floor, solve, distributed)
    else:
        x, boxes, rates = crops.crop_batch(frames, bboxes, scale)
        with torch.no_grad():
            if candidates_path == "fused":
                out = net.candidates(x, candidates, nms_radius, refine=refine, **ask)
            else:
                out = inference.heatmaps_to_candidates(net(x), candidates, nms_radius, refine=refine, **ask)
        cand, hess = (out[0], out[-1]) if mode else (out, None)        # (return_cov: cov, info — info is what weighs)
        if mode:                                        # the only device->host copy: one buffer, hess | cand (the f64 part first)
            n, k, mm = cand.shape[:3]
            host = torch.cat([hess.reshape(-1).view(torch.uint8), cand.reshape(-1).view(torch.uint8)]).cpu().numpy()
            hess = host[:n * k * mm * 24].view(np.float64).reshape(n, k, mm, 3)
            cand = host[n * k * mm * 24:].view(np.float32).reshape(n, k, mm, 3)
        else:
            cand = cand.cpu().numpy()
        poses, rep = solve(cand, boxes, rates, hess)
    if want:
        poses = _gated_poses(poses, rep, max_rms_px, min_inliers)
    poses = _checked_poses(poses, on_fail)
    return (poses, rep) if return_report else poses


def _load(net, request, frames, bboxes, frame_idx, distributed, scale, rule, gather=None):
    """The loader's result for `request`: the net's own call, or with distributed=True every rank its shard of the boxes and the
    records of `gather` (default: all of the request's) gathered, all crops on all ranks."""
    with torch.no_grad():
        if distributed:
            return parallel._sharded_loader(net, request, frames, bboxes, frame_idx, None, 0, scale, rule, None, crops.STD, None,
                                            gather=gather)
        return net._loader(request, frames, bboxes, frame_idx, scale, rule, None, crops.STD, None)


def _solve_valid_crops(rows, v, solve):
    """solve(rows, boxes, rates) -> (poses, report or None) on the rows (kp [m,K,3] or cand [m,K,M,3]) of a loader's fetched
    record `v`, with the crops the loader could not make (valid == 0: NaN rows) kept away from it: their rows go in as zeros with
    rate 1.0, their poses come back as the NaN row that "no solution" is, their report rows are those of "fewer than 4" with
    n = 0 (status 1, the rest NaN), and in a candidates report no keypoint of theirs entered a solve (.used -1, .rescued False)."""
    bad = v["valid"] == 0
    rates = [1.0 if b else float(r) for r, b in zip(v["rates"], bad)]
    poses, rep = solve(np.where(bad.reshape(-1, *[1] * (rows.ndim - 1)), np.float32(0), rows), v["boxes"].tolist(), rates)
    if rep is not None and bad.any():
        raw = rep.raw.copy()
        raw[bad] = np.nan
        raw[bad, 0], raw[bad, 2] = 1.0, 0.0
        fixed = pnp.PoseReport(raw)
        if rep.used is not None:
            fixed.used, fixed.rescued = rep.used.copy(), rep.rescued.copy()
            fixed.used[bad], fixed.rescued[bad] = -1, False
        rep = fixed
    return [(np.full(4, np.nan), np.full(3, np.nan)) if b else p for p, b in zip(poses, bad)], rep


def _device_select_poses(net, frames, bboxes, frame_idx, distributed, scale, rule, refine, thresh, min_k, weights, cov_floor, kp3d, K,
                         threads, want):
    """device_select=True: the correspondence record's one copy, then the solve on it."""
    request = inference.LoaderRequest(refine, None, cov_floor if weights == "covariance" else None, (thresh, min_k, weights))
    r = _load(net, request, frames, bboxes, frame_idx, distributed, scale, rule)
    v = r.host("correspondences")
    q, t, *rep = pnp.correspondences_to_pose_batch(v["pts"], v["w"], v["count"], v["order"], kp3d, np.asarray(K, np.float64), threads,
                                                   report=want)
    return [(q[i], t[i]) for i in range(r.m)], rep[0] if want else None


def _device_loader_poses(net, frames, bboxes, frame_idx, distributed, scale, rule, refine, solve):
    """device_loader=True."""
    v = _load(net, inference.LoaderRequest(refine), frames, bboxes, frame_idx, distributed, scale, rule).host("keypoints")
    return _solve_valid_crops(v["kp"], v, solve)


def _device_select_candidate_poses(net, frames, bboxes, frame_idx, distributed, scale, rule, refine, candidates, nms_radius, thresh,
                                   min_k, weights, cov_floor, kp3d, K, min_ratio, threads, want):
    """candidate_poses with device_select=True: the record's one copy, then the solve on it."""
    request = inference.LoaderRequest(refine, (candidates, nms_radius), cov_floor if weights == "covariance" else None,
                                      (thresh, min_k, weights))
    r = _load(net, request, frames, bboxes, frame_idx, distributed, scale, rule, gather=(request.second,))
    v = r.host(request.second)
    q, t, _, *rep = pnp.candidate_correspondences_to_pose_batch(v["cpts"], v["cw"], v["cpeak"], v["count"], v["order"], kp3d,
                                                                np.asarray(K, np.float64), min_ratio, threads, report=want)
    return [(q[i], t[i]) for i in range(r.m)], rep[0] if want else None


def _loader_candidates_poses(net, frames, bboxes, frame_idx, scale, rule, candidates, nms_radius, refine, weights, cov_floor, solve,
                             distributed=False):
    """candidates_path="loader": solve(cand, boxes, rates, hess or None) on the fetched record of the (refined) candidates."""
    request = inference.LoaderRequest(refine, (candidates, nms_radius), cov_floor if weights == "covariance" else None)
    v = _load(net, request, frames, bboxes, frame_idx, distributed, scale, rule).host(request.main[0])
    hess = {"peak": None, "hessian": v.get("cand_hess"), "covariance": v.get("cand_info")}[weights]
    if hess is not None:                # (the rows of an invalid crop are NaN: zeros go in, like its candidates)
        hess = np.where((v["valid"] == 0).reshape(-1, 1, 1, 1), 0.0, hess)
    return _solve_valid_crops(v["cand"], v, lambda rows, boxes, rates: solve(rows, boxes, rates, hess))


def _host_crops_poses(net, frames, bboxes, frame_idx, scale, rule, refine, distributed, keypoints_only, candidates, nms_radius,
                      candidates_path, solve):
    """Crops made by crops.crop_batch: the keypoint form, and candidates > 1 with candidates_path "heatmaps" or "fused"."""
    if frame_idx is not None or rule != "val":
        raise ValueError("frame_idx and rule belong to device_loader=True (crops.crop_batch: one val box per frame)")
    rk = {} if refine == "get_final" else {"refine": refine}
    x, boxes, rates = crops.crop_batch(frames, bboxes, scale)
    with torch.no_grad():
        if candidates != 1 and candidates_path == "fused":
            rows = net.candidates(x, candidates, nms_radius)
        elif candidates != 1:
            rows = inference.heatmaps_to_candidates(net(x), candidates, nms_radius)
        elif distributed:
            rows = parallel.sharded_keypoints(net, x, keypoints_only=keypoints_only, **rk)
        elif keypoints_only:
            rows = net(x, output="keypoints", **rk)
        else:
            rows = inference.heatmaps_to_keypoints(net(x), **rk)
    rows = rows.cpu().numpy()                               # the only device->host copy: N*K*3 floats (N*K*M*3 with candidates)
    return solve(rows, boxes, rates)


def _gated_poses(poses, rep, max_rms_px, min_inliers):
    """Solved poses that miss a gate become the NaN row of "no pose"; rep.gated marks them, their report rows stay."""
    gated = np.zeros(len(poses), bool)
    if max_rms_px is not None:
        gated |= (rep.status == 0) & (rep.rms_px > max_rms_px)
    if min_inliers is not None:
        gated |= (rep.status == 0) & (rep.inliers < min_inliers)
    rep.gated = gated
    return [(np.full(4, np.nan), np.full(3, np.nan)) if g else p for p, g in zip(poses, gated)]


def _checked_poses(poses, on_fail):
    if on_fail == "raise":
        bad = [i for i, (q, t) in enumerate(poses) if not (np.all(np.isfinite(q)) and np.all(np.isfinite(t)))]
        if bad:
            raise PoseFailure(f"no pose for batch positions {bad}")
    return poses


def run_submission(net, batches, kp3d, K, writer, real: bool = False, on_fail: str = "fallback", **kw):
    """`batches` yields (names, frames_u8_cuda, bboxes); appends every pose to `writer` (ours or the reference's
    SubmissionWriter: anything with append_test / append_real_test).  A submission needs a finite row for every
    image, so an image without a solution gets FALLBACK_POSE and is logged and listed in `writer.failed`
    (on_fail="fallback"), or stops the run (on_fail="raise").  `kw` goes to estimate_poses (keypoints_only=,
    refine="get_final2", ...).  With a gate in `kw` (max_rms_px=, min_inliers=) a solved pose that misses it is such a failure:
    it gets FALLBACK_POSE and is listed in `writer.failed`."""
    failed = []
    for names, frames, bboxes in batches:
        poses = estimate_poses(net, frames, bboxes, kp3d, K, on_fail="nan", **kw)
        if kw.get("return_report"):
            poses = poses[0]
        for name, (q, t) in zip(names, poses):
            if not (np.all(np.isfinite(q)) and np.all(np.isfinite(t))):
                if on_fail == "raise":
                    raise PoseFailure(f"no pose for {name}")
                logger.warning("no pose for %s: writing the fallback pose", name)
                failed.append(name)
                q, t = FALLBACK_POSE
            (writer.append_real_test if real else writer.append_test)(name, q, t)
    try:
        writer.failed = getattr(writer, "failed", []) + failed
    except AttributeError:
        pass
    return writer
