"""Heatmaps -> keypoints, the drop-in for the reference's inference.py + caller glue.

Reference being replaced:
  * demo.py:172-185 / val.py:151-164   two-stage torch.max + per-keypoint .cpu().item() loop
  * inference.py:22-51                 get_max_preds
  * inference.py:136-152, 75-94        get_final -> my_taylor
  * inference.py:154-169, 96-111, 54-73  get_final2 -> gaussian_blur + taylor (refine="get_final2")
  * val.py:172-180 / demo.py:195-200   top-k by peak value, crop -> image coordinates

`heatmaps_to_keypoints` is the fused GPU path ([N,K,H,W] on the device -> [N,K,3] on the
device, one kernel, no host sync); `get_max_preds` / `get_final` keep the reference's names
and numpy-in/numpy-out contract for callers that are not rewritten, but run the same kernel.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import heapq
import math

import numpy as np
import torch

from . import _lib


REFINES = ("get_final", "get_final2", "gaussfit")


def check_refine(refine):
    """The sub-pixel step: "get_final" (default, inference.py:136-152), "get_final2" (inference.py:154-169) or "gaussfit" (the
    2-D Gaussian fit of the reference's test.py, gaussfit_keypoints)."""
    if not isinstance(refine, str) or refine not in REFINES:
        raise ValueError(f"refine must be one of {REFINES}, got {refine!r}")
    return refine


def final2_workspace(n: int, k: int, h: int, w: int, device):
    """Scratch of esahrnet_keypoints_final2 (per-tile maxima only), 256-byte aligned: (tensor, pointer, bytes)."""
    nbytes = C.c_size_t()
    _lib.check(_lib.lib().esahrnet_keypoints_final2_workspace_bytes(n, k, h, w, C.byref(nbytes)))
    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256, nbytes.value


def _keypoints_final2(heat: torch.Tensor, want_index: bool, want_hessian: bool = False):
    heat = heat.contiguous()
    n, k, h, w = heat.shape
    kp = torch.empty((n, k, 3), dtype=torch.float32, device=heat.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=heat.device) if want_index else None
    stream = torch.cuda.current_stream(heat.device).cuda_stream
    with torch.cuda.device(heat.device):
        ws, ws_ptr, ws_bytes = final2_workspace(n, k, h, w, heat.device)
        if want_hessian:
            hess = torch.empty((n, k, 3), dtype=torch.float64, device=heat.device)
            _lib.check(_lib.lib().esahrnet_keypoints_final2_hess(heat.data_ptr(), n, k, h, w, kp.data_ptr(),
                                                                 idx.data_ptr() if want_index else None, hess.data_ptr(),
                                                                 ws_ptr, ws_bytes, C.c_void_p(stream)))
            return kp, idx, hess
        _lib.check(_lib.lib().esahrnet_keypoints_final2(heat.data_ptr(), n, k, h, w, kp.data_ptr(),
                                                        idx.data_ptr() if want_index else None, ws_ptr, ws_bytes,
                                                        C.c_void_p(stream)))
    return kp, idx


def _keypoints(heat: torch.Tensor, want_index: bool, refine: str = "get_final", want_hessian: bool = False):
    check_refine(refine)
    if want_hessian and refine == "get_final":
        raise ValueError("return_hessian=True needs refine='get_final2' or 'gaussfit': get_final computes no Hessian")
    if not isinstance(heat, torch.Tensor) or heat.dim() != 4:
        raise ValueError("expected a 4-D tensor [N, K, H, W]")
    if not heat.is_cuda:
        raise RuntimeError("heatmaps_to_keypoints runs on the GPU only (no CPU fallback)")
    if heat.dtype != torch.float32:
        raise TypeError(f"expected float32 heatmaps, got {heat.dtype}")
    if refine == "get_final2":
        return _keypoints_final2(heat, want_index, want_hessian)
    if refine == "gaussfit":
        kp, _, _, hess, idx = _gaussfit(heat, want_index)
        return (kp, idx, hess) if want_hessian else (kp, idx)
    # heat-maps that come straight out of a forward carry the per-tile maxima their output-layer kernel found
    # (hrnet._Runtime.forward): finishing over those gives the same bits without reading the maps again.  The note is
    # honoured only for this very tensor object, unmodified since (views, clones and in-place edits take the full sweep).
    note = getattr(heat, "_esa_partials", None)
    if note is not None:
        try:
            fresh = note[2] == heat._version
        except RuntimeError:                # inference tensor: no version counter
            fresh = False
        if not fresh or not heat.is_contiguous() or note[0].device != heat.device:
            note = None
    heat = heat.contiguous()
    n, k, h, w = heat.shape
    kp = torch.empty((n, k, 3), dtype=torch.float32, device=heat.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=heat.device) if want_index else None
    stream = torch.cuda.current_stream(heat.device).cuda_stream
    with torch.cuda.device(heat.device):
        if note is not None:
            _lib.check(_lib.lib().esahrnet_keypoints_finish(heat.data_ptr(), note[0].data_ptr(), note[1], n, k, h, w,
                                                            kp.data_ptr(), idx.data_ptr() if want_index else None,
                                                            C.c_void_p(stream)))
        else:
            _lib.check(_lib.lib().esahrnet_keypoints_ex(heat.data_ptr(), n, k, h, w, kp.data_ptr(),
                                                        idx.data_ptr() if want_index else None, C.c_void_p(stream)))
    return kp, idx


def heatmaps_to_keypoints(heat: torch.Tensor, refine: str = "get_final", return_hessian: bool = False):
    """f32 cuda [N,K,H,W] -> f32 cuda [N,K,3] = (x, y, peak); x=col, y=row, 0-based; peak is the raw maximum.
    refine="get_final" (default): sub-pixel refined exactly as inference.my_taylor does.  refine="get_final2": as
    get_final2 does (11x11 Gaussian blur rescaled to the raw peak, log, full-Hessian Newton step; include/esahrnet.h
    esahrnet_keypoints_final2), same arg-max and peak; the blurred maps are never stored and `heat` is not modified.
    return_hessian=True (get_final2 only): -> (kp, hess f64 cuda [N,K,3] = (dxx, dxy, dyy)), the Hessian of the blurred
    log heat-map each step used, NaN where no step was taken (esahrnet_keypoints_final2_hess); kp has the same bits.
    refine="gaussfit": the kp of gaussfit_keypoints (an accepted fit's centre, else the get_final row); with
    return_hessian=True (kp, hess = (-2a, -2b, -2c) of the fit, NaN where it was rejected)."""
    out = _keypoints(heat, False, refine, return_hessian)
    return (out[0], out[2]) if return_hessian else out[0]


def _check_at_outputs(refine, return_hessian, return_fit, return_cov, cov_floor):
    """What refine_at and heatmaps_to_candidates(refine=...) may be asked for: -> (decoder of esahrnet_keypoints_at, cov_floor)."""
    check_refine(refine)
    if return_hessian and refine == "get_final":
        raise ValueError("return_hessian=True needs refine='get_final2' or 'gaussfit': get_final computes no Hessian")
    if (return_fit or return_cov) and refine != "gaussfit":
        raise ValueError("return_fit=True and return_cov=True need refine='gaussfit': only the Gaussian fit has parameters and a covariance")
    return REFINES.index(refine), check_cov_floor(cov_floor)


def _at_outputs(shape, decoder, return_hessian, return_fit, return_cov, device):
    """The optional outputs of esahrnet_keypoints_at for slots of `shape`: name -> tensor or None."""
    new = lambda dt, *tail: torch.empty((*shape, *tail), dtype=dt, device=device)      # noqa: E731
    return {"fit": new(torch.float64, 8) if return_fit else None,
            "status": new(torch.int32) if decoder == 2 else None,
            "hess": new(torch.float64, 3) if return_hessian else None,
            "cov": new(torch.float64, 3) if return_cov else None,
            "info": new(torch.float64, 3) if return_cov else None}


def _at_workspace(n, k, h, w, decoder, device):
    """Scratch of esahrnet_keypoints_at, 256-byte aligned: (tensor or None, pointer or None, bytes)."""
    nbytes = C.c_size_t()
    _lib.check(_lib.lib().esahrnet_keypoints_at_workspace_bytes(n, k, h, w, decoder, C.byref(nbytes)))
    if not nbytes.value:
        return None, None, 0
    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=device)
    return ws, ws.data_ptr() + (-ws.data_ptr()) % 256, nbytes.value


def _at_returns(o, return_hessian, return_fit, return_cov):
    return (*((o["fit"], o["status"]) if return_fit else ()), *((o["hess"],) if return_hessian else ()),
            *((o["cov"], o["info"]) if return_cov else ()))


def refine_at(heat: torch.Tensor, at: torch.Tensor, refine: str = "get_final", return_hessian: bool = False,
              return_fit: bool = False, return_cov: bool = False, cov_floor: float = 1e-6):
    """The decoders at pixels the caller names (include/esahrnet.h esahrnet_keypoints_at): heat f32 cuda [N,K,H,W], at int32 cuda
    [N,K] or [N,K,M] = row * W + column (the index heatmaps_to_candidates(return_index=True) and the decoders' idx hold) -> kp f32
    cuda of at's shape + (3,) = (x, y, raw value at the pixel), refined by `refine` AT that pixel: "get_final" a row of the
    reference's get_final(hm, coords); "get_final2" its get_final2(hm, coords), the rescale factor still the whole plane's;
    "gaussfit" the Gaussian fit on the window around the pixel (a rejected fit keeps the get_final row).  At a plane's arg-max these
    are the rows of heatmaps_to_keypoints / gaussfit_keypoints, bit for bit.  A pixel outside the plane (-1: no candidate) gives NaN
    rows and status -1.  The optional outputs follow kp in the order of the existing decoders' returns, each of at's shape + its
    own: return_fit (gaussfit) fit f64 (8,), status int32; return_hessian (get_final2, gaussfit) hess f64 (3,); return_cov
    (gaussfit) cov f64 (3,), info f64 (3,).  No host sync; `heat` and `at` are not modified."""
    decoder, cov_floor = _check_at_outputs(refine, return_hessian, return_fit, return_cov, cov_floor)
    if not isinstance(heat, torch.Tensor) or heat.dim() != 4:
        raise ValueError("expected a 4-D tensor [N, K, H, W]")
    if not heat.is_cuda:
        raise RuntimeError("refine_at runs on the GPU only (no CPU fallback)")
    if heat.dtype != torch.float32:
        raise TypeError(f"expected float32 heatmaps, got {heat.dtype}")
    n, k, h, w = heat.shape
    if not (isinstance(at, torch.Tensor) and at.device == heat.device and at.dtype == torch.int32 and at.dim() in (2, 3) and
            tuple(at.shape[:2]) == (n, k) and at.numel() > 0):
        raise ValueError(f"at must be an int32 tensor [{n}, {k}] or [{n}, {k}, M] on {heat.device}")
    heat, at = heat.contiguous(), at.contiguous()
    m = at.shape[2] if at.dim() == 3 else 1
    dev = heat.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()                     # noqa: E731
    with torch.cuda.device(dev):
        kp = torch.empty((*at.shape, 3), dtype=torch.float32, device=dev)
        o = _at_outputs(at.shape, decoder, return_hessian, return_fit, return_cov, dev)
        ws, ws_ptr, ws_bytes = _at_workspace(n, k, h, w, decoder, dev)
        _lib.check(_lib.lib().esahrnet_keypoints_at(heat.data_ptr(), n, k, h, w, at.data_ptr(), m, decoder, kp.data_ptr(),
                                                    ptr(o["hess"]), ptr(o["fit"]), ptr(o["status"]), ptr(o["cov"]), ptr(o["info"]),
                                                    cov_floor, ws_ptr, ws_bytes, C.c_void_p(stream)))
    rest = _at_returns(o, return_hessian, return_fit, return_cov)
    return (kp, *rest) if rest else kp


def heatmaps_to_candidates(heat: torch.Tensor, candidates: int = 3, nms_radius: int = 6, return_index: bool = False, form=None,
                           refine: str = "get_final", return_hessian: bool = False, return_fit: bool = False,
                           return_cov: bool = False, cov_floor: float = 1e-6):
    """f32 cuda [N,K,H,W] -> f32 cuda [N,K,M,3] = (x, y, peak), the M = `candidates` (1..4) best peaks of every heat-map, best
    first (include/esahrnet.h esahrnet_keypoints_candidates, one kernel, no host sync).  Candidate 0 is the row of
    heatmaps_to_keypoints, bit for bit; candidate m >= 1 is the largest local maximum (>= its 8 neighbours, neither NaN nor
    -inf, no NaN neighbour) at Chebyshev distance > nms_radius from every earlier candidate, ties to the lower index, refined
    by the same get_final step at its own pixel; rows without a qualifying pixel are NaN.  return_index=True: -> (cand, idx int32
    cuda [N,K,M] = row * W + column of each candidate, -1 where there is none).  pnp.candidates_to_pose_batch solves on them.
    form (esahrnet_keypoints_candidates_form): 0 the multi-sweep kernel, 1 the one-sweep kernel (the same bits; refused on a plane
    it does not serve: not 16-byte aligned, W no multiple of 4, more than 4096 cells of 8 x 8), -1 what the fused paths launch;
    None (default): esahrnet_keypoints_candidates, the multi-sweep kernel.
    refine="get_final2" / "gaussfit", or any of return_hessian / return_fit / return_cov (include/esahrnet.h
    esahrnet_keypoints_candidates_refined, form None or -1 only): the same search, then every candidate's (x, y) refined by that decoder
    at the candidate's own pixel, as refine_at does on the index; the peak column is the raw value there either way.  The optional
    outputs follow cand (and idx) in refine_at's order, each [N,K,M] + its own shape; rows without a candidate are NaN, status -1."""
    decoder, cov_floor = _check_at_outputs(refine, return_hessian, return_fit, return_cov, cov_floor)
    refined = decoder != 0 or return_hessian or return_fit or return_cov
    if refined and form not in (None, -1):
        raise ValueError(f"form={form!r} names a kernel of the plain search: a refined call (refine={refine!r}) takes form None or -1")
    if not isinstance(heat, torch.Tensor) or heat.dim() != 4:
        raise ValueError("expected a 4-D tensor [N, K, H, W]")
    if not heat.is_cuda:
        raise RuntimeError("heatmaps_to_candidates runs on the GPU only (no CPU fallback)")
    if heat.dtype != torch.float32:
        raise TypeError(f"expected float32 heatmaps, got {heat.dtype}")
    heat = heat.contiguous()
    n, k, h, w = heat.shape
    m = int(candidates)
    # (the library refuses M outside 1..4 and a negative radius with its own text; nothing is allocated by M before that)
    cand = torch.empty((n, k, min(max(m, 1), _lib.MAX_CANDIDATES), 3), dtype=torch.float32, device=heat.device)
    idx = torch.empty(cand.shape[:3], dtype=torch.int32, device=heat.device) if return_index or refined else None
    stream = torch.cuda.current_stream(heat.device).cuda_stream
    with torch.cuda.device(heat.device):
        if refined:
            ptr = lambda t: None if t is None else t.data_ptr()             # noqa: E731
            o = _at_outputs(cand.shape[:3], decoder, return_hessian, return_fit, return_cov, heat.device)
            ws, ws_ptr, ws_bytes = _at_workspace(n, k, h, w, decoder, heat.device)
            _lib.check(_lib.lib().esahrnet_keypoints_candidates_refined(heat.data_ptr(), n, k, h, w, m, int(nms_radius), decoder,
                                                                        cand.data_ptr(), idx.data_ptr(), ptr(o["hess"]),
                                                                        ptr(o["fit"]), ptr(o["status"]), ptr(o["cov"]),
                                                                        ptr(o["info"]), cov_floor, ws_ptr, ws_bytes,
                                                                        C.c_void_p(stream)))
            out = (cand, *((idx,) if return_index else ()), *_at_returns(o, return_hessian, return_fit, return_cov))
            return out if len(out) > 1 else cand
        if form is None:
            _lib.check(_lib.lib().esahrnet_keypoints_candidates(heat.data_ptr(), n, k, h, w, m, int(nms_radius), cand.data_ptr(),
                                                                idx.data_ptr() if return_index else None, C.c_void_p(stream)))
        else:
            _lib.check(_lib.lib().esahrnet_keypoints_candidates_form(heat.data_ptr(), n, k, h, w, m, int(nms_radius), int(form),
                                                                     cand.data_ptr(), idx.data_ptr() if return_index else None,
                                                                     C.c_void_p(stream)))
    return (cand, idx) if return_index else cand


def check_cov_floor(cov_floor) -> float:
    """cov_floor of the covariance outputs: a number >= 0 (the reference's evaluation.py:479 uses 1e-6)."""
    try:
        f = float(cov_floor)
    except (TypeError, ValueError):
        raise ValueError(f"cov_floor must be a number >= 0, got {cov_floor!r}") from None
    if not f >= 0.0:
        raise ValueError(f"cov_floor must be a number >= 0, got {cov_floor!r}")
    return f


def gaussfit_keypoints(heat: torch.Tensor, return_cov: bool = False, cov_floor: float = 1e-6):
    """The third decoder (include/esahrnet.h esahrnet_keypoints_gaussfit): offset + A exp(-(a dx^2 + 2 b dx dy + c dy^2)) fitted
    on the device to the 13 x 13 window around each plane's arg-max, the fit the reference's test.py makes with curve_fit.
    f32 cuda [N,K,H,W] -> (kp f32 [N,K,3] = (x0, y0, raw peak); fit f64 [N,K,8] = (A, x0, y0, a, b, c, off, cost); status int32
    [N,K], 0 = accepted; hess f64 [N,K,3] = (-2a, -2b, -2c)).  A rejected keypoint (status 1, 2, 3) keeps the get_final row of
    heatmaps_to_keypoints, its fit and hess are NaN.  hess is what keypoints_to_correspondences(weights="hessian") takes.
    return_cov=True (esahrnet_keypoints_gaussfit_cov): -> (kp, fit, status, hess, cov, info), the same bits in the first four; cov
    f64 [N,K,3] = (cxx, cxy, cyy), the (x0, y0) block of curve_fit's pcov = cost / (n - 7) (J^T J)^-1 in crop px^2, NaN for a
    rejected fit or a window of at most 7 pixels; info f64 [N,K,3] = -cov^-1, NaN also where cxx < cov_floor (the reference's
    guard, evaluation.py:479): what keypoints_to_correspondences(weights="covariance") takes in hess' place."""
    if not return_cov:
        return _gaussfit(heat, False)[:4]
    out = _gaussfit(heat, False, True, cov_floor)
    return out[:4] + out[5:]


def _gaussfit(heat: torch.Tensor, want_index: bool, want_cov: bool = False, cov_floor: float = 1e-6):
    """gaussfit_keypoints, plus idx int32 [N,K] (None unless asked for): -> (kp, fit, status, hess, idx), with want_cov (kp, fit,
    status, hess, idx, cov, info)."""
    if not isinstance(heat, torch.Tensor) or heat.dim() != 4:
        raise ValueError("expected a 4-D tensor [N, K, H, W]")
    if want_cov:
        cov_floor = check_cov_floor(cov_floor)
    if not heat.is_cuda:
        raise RuntimeError("gaussfit_keypoints runs on the GPU only (no CPU fallback)")
    if heat.dtype != torch.float32:
        raise TypeError(f"expected float32 heatmaps, got {heat.dtype}")
    heat = heat.contiguous()
    n, k, h, w = heat.shape
    dev = heat.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        kp = torch.empty((n, k, 3), dtype=torch.float32, device=dev)
        fit = torch.empty((n, k, 8), dtype=torch.float64, device=dev)
        status = torch.empty((n, k), dtype=torch.int32, device=dev)
        hess = torch.empty((n, k, 3), dtype=torch.float64, device=dev)
        idx = torch.empty((n, k), dtype=torch.int32, device=dev) if want_index else None
        if want_cov:
            cov = torch.empty((n, k, 3), dtype=torch.float64, device=dev)
            info = torch.empty((n, k, 3), dtype=torch.float64, device=dev)
            _lib.check(_lib.lib().esahrnet_keypoints_gaussfit_cov(heat.data_ptr(), n, k, h, w, kp.data_ptr(),
                                                                  idx.data_ptr() if want_index else None, fit.data_ptr(),
                                                                  status.data_ptr(), hess.data_ptr(), cov.data_ptr(),
                                                                  info.data_ptr(), cov_floor, C.c_void_p(stream)))
            return kp, fit, status, hess, idx, cov, info
        _lib.check(_lib.lib().esahrnet_keypoints_gaussfit(heat.data_ptr(), n, k, h, w, kp.data_ptr(),
                                                          idx.data_ptr() if want_index else None, fit.data_ptr(),
                                                          status.data_ptr(), hess.data_ptr(), C.c_void_p(stream)))
    return kp, fit, status, hess, idx


def gaussfit_sigma_theta(fit):
    """fit [..., 8] (tensor or array) of gaussfit_keypoints -> (sigma_x, sigma_y, theta) as numpy f64 arrays: the parameters of
    the reference's test.py twoD_Gaussian, which reproduce the fitted function when put into it with (A, x0, y0, off):
        a = cos^2 th / (2 sx^2) + sin^2 th / (2 sy^2),  b = -sin 2th / (4 sx^2) + sin 2th / (4 sy^2),  c = sin^2 th / (2 sx^2) + ...
    Of the equivalent triples the one with sigma_x >= sigma_y and theta in (-pi/2, pi/2] is returned.  test.py's sign of b makes
    its theta the NEGATIVE of the counter-clockwise angle (x right, y down the rows) of the sigma_x axis: the long axis points
    along (cos theta, -sin theta).  theta is undetermined when the two sigmas are equal (0 or pi/2 is returned).  NaN for a
    rejected fit."""
    f = fit.detach().cpu().numpy() if isinstance(fit, torch.Tensor) else np.asarray(fit)
    a, b, c = f[..., 3].astype(np.float64), f[..., 4].astype(np.float64), f[..., 5].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        half, rad = 0.5 * (a + c), np.hypot(0.5 * (a - c), b)
        sx, sy = np.sqrt(0.5 / (half - rad)), np.sqrt(0.5 / (half + rad))
        # eigenvector of the SMALLER eigenvalue (the long axis): (b, l - a) or (l - c, b), whichever is better conditioned
        l = half - rad
        th = -np.where(a > c, np.arctan2(l - a, b), np.arctan2(b, l - c))      # test.py's sign
        th = np.where(th > np.pi / 2, th - np.pi, np.where(th <= -np.pi / 2, th + np.pi, th))
    return sx, sy, th


WEIGHTS = ("peak", "hessian", "covariance")


def check_weights(weights, refine="get_final2"):
    """The weight of the pose refinement: "peak" (default; val.py:194-209), "hessian" (the decoder's Hessian as the 2x2
    weight uncertainty_pnp.cpp takes; needs refine="get_final2" or "gaussfit") or "covariance" (refine="gaussfit" only: the
    covariance of the fitted centre, inv(sqrtm(covar)) as evaluation.py:471-487 forms it; its info output goes where the Hessian
    goes).  -> the mode of esahrnet_correspondences."""
    if not isinstance(weights, str) or weights not in WEIGHTS:
        raise ValueError(f"weights must be one of {WEIGHTS}, got {weights!r}")
    if weights == "hessian" and refine not in ("get_final2", "gaussfit"):
        raise ValueError("weights='hessian' needs refine='get_final2' or 'gaussfit': get_final computes no Hessian")
    if weights == "covariance" and refine != "gaussfit":
        raise ValueError("weights='covariance' needs refine='gaussfit': only the Gaussian fit has a parameter covariance")
    return int(weights != "peak")


RECORD_KINDS = ("keypoints", "correspondences", "candidates", "candidate_correspondences", "candidates_refined")
# THE description of the packed records; every layout, view and exchange below and in hrnet / parallel / pipeline derives from it.
# Element type and trailing shape of every field (k = keypoints per crop, M = candidates per keypoint) ...
_RECORD_TYPES = {"rates": (torch.float64, ()), "fit": (torch.float64, ("k", 8)), "hess": (torch.float64, ("k", 3)),
                 "cov": (torch.float64, ("k", 3)), "info": (torch.float64, ("k", 3)), "kp": (torch.float32, ("k", 3)),
                 "boxes": (torch.int32, (4,)), "valid": (torch.int32, ()), "idx": (torch.int32, ("k",)),
                 "status": (torch.int32, ("k",)), "pts": (torch.float64, ("k", 2)), "w": (torch.float64, ("k", 3)),
                 "count": (torch.int32, ()), "order": (torch.int32, ("k",)), "cand": (torch.float32, ("k", "M", 3)),
                 "cidx": (torch.int32, ("k", "M")),
                 # the refined candidates' outputs, one row per candidate: names of their own, since their shapes carry M
                 "cand_fit": (torch.float64, ("k", "M", 8)), "cand_hess": (torch.float64, ("k", "M", 3)),
                 "cand_cov": (torch.float64, ("k", "M", 3)), "cand_info": (torch.float64, ("k", "M", 3)),
                 "cand_status": (torch.int32, ("k", "M")),
                 # the candidates in image pixels, in rank order (esahrnet_correspondences_cand): point, 2x2 weight and peak of each
                 "cpts": (torch.float64, ("k", "M", 2)), "cw": (torch.float64, ("k", "M", 3)), "cpeak": (torch.float32, ("k", "M"))}
# ... and the fields of each record in memory order (the f64 parts first: 8-byte aligned); fit, hess and status are there with
# gaussfit only, cov and info with cov only (cand_fit, cand_status, cand_cov and cand_info likewise; cand_hess is always there)
_RECORD_ORDER = {"keypoints": ("rates", "fit", "hess", "cov", "info", "kp", "boxes", "valid", "idx", "status"),
                 "correspondences": ("pts", "w", "count", "order"),
                 "candidates": ("rates", "cand", "boxes", "valid", "cidx"),
                 "candidate_correspondences": ("cpts", "cw", "cpeak", "count", "order"),
                 "candidates_refined": ("rates", "cand_fit", "cand_hess", "cand_cov", "cand_info", "cand", "boxes", "valid", "cidx",
                                        "cand_status")}
_RECORD_SWITCH = {"fit": "gaussfit", "hess": "gaussfit", "status": "gaussfit", "cov": "cov", "info": "cov",
                  "cand_fit": "gaussfit", "cand_status": "gaussfit", "cand_cov": "cov", "cand_info": "cov"}
_NUMPY_TYPES = {torch.float64: np.dtype(np.float64), torch.float32: np.dtype(np.float32), torch.int32: np.dtype(np.int32)}


def _dims(name, k, mm):
    return tuple(k if d == "k" else mm if d == "M" else d for d in _RECORD_TYPES[name][1])


def _field_bytes(name, k, mm=1):
    """Bytes per crop of a field with k keypoints per crop and mm candidates per keypoint."""
    return _NUMPY_TYPES[_RECORD_TYPES[name][0]].itemsize * math.prod(_dims(name, k, mm))


def record_fields(k: int, kind: str, gaussfit: bool = False, cov: bool = False, candidates=None):
    """The fields of a packed record in memory order, as ((name, bytes per crop), ...): kind="keypoints" the main record of
    net._loader (rates | [fit | hess | [cov | info]] | kp | boxes | valid | idx | [status]), kind="correspondences"
    the buffer of pack_correspondences (pts | w | count | order), kind="candidates" net._loader's main record of a request with
    candidates=(M, r) (rates | cand | boxes | valid | cidx), kind="candidates_refined" that of a request with candidates and a
    refine other than "get_final" (rates | [cand_fit] | cand_hess | [cand_cov | cand_info] | cand | boxes | valid | cidx |
    [cand_status]: the decoder's outputs for every candidate, f64 first; gaussfit=True is refine="gaussfit", False "get_final2"),
    kind="candidate_correspondences" net._loader's second record of a request with candidates and select (cpts | cw | cpeak |
    count | order: what pnp.candidate_correspondences_to_pose_batch consumes; whatever the decoder, no gaussfit / cov switch).
    A record is field-major, so field f of m crops takes m * bytes and
    starts at m * (the bytes of the fields in front of it); every size is a multiple of 4.  This is the description the views
    (record_views), the offsets (packed_layout) and the exchange of a sharded batch (parallel.gather_records,
    esahrnet_gather_records) work from."""
    if kind not in RECORD_KINDS:
        raise ValueError(f"kind must be one of {RECORD_KINDS}, got {kind!r}")
    k = int(k)
    if k < 1:
        raise ValueError(f"k = {k}: a record has at least one keypoint per crop")
    if kind in ("correspondences", "candidate_correspondences") and (gaussfit or cov):
        raise ValueError("gaussfit and cov belong to kind='keypoints'")
    if cov and not gaussfit:
        raise ValueError("cov=True belongs to gaussfit=True")
    mm = 1
    if kind in ("candidates", "candidates_refined", "candidate_correspondences"):
        if gaussfit and kind == "candidates":
            raise ValueError("candidates=M belongs to the get_final decoder (gaussfit=False)")
        if candidates is None or not 1 <= int(candidates) <= _lib.MAX_CANDIDATES:
            raise ValueError(f"candidates must be in 1..{_lib.MAX_CANDIDATES}, got {candidates!r}")
        mm = int(candidates)
    elif candidates is not None:
        raise ValueError("candidates=M belongs to kind='candidates'")     # (and to 'candidates_refined')
    on = {"gaussfit": gaussfit, "cov": cov, None: True}
    return tuple((name, _field_bytes(name, k, mm)) for name in _RECORD_ORDER[kind] if on[_RECORD_SWITCH.get(name)])


def record_views(packed, m: int, k: int, fields):
    """The typed views of a packed record of m crops (uint8 [m * bytes per crop], laid out as `fields` = record_fields(...)
    says): name -> tensor, e.g. kp f32 [m,k,3], rates f64 [m], order int32 [m,k], cand f32 [m,k,M,3] (M from the field's bytes).
    `packed` a numpy uint8 array (the record copied to the host): numpy views of the same shapes and types."""
    host = isinstance(packed, np.ndarray)
    have, need = packed.size if host else packed.numel(), m * sum(b for _, b in fields)
    if have != need:
        raise ValueError(f"a record of {m} crops has {need} bytes, the buffer {have}")
    out, off = {}, 0
    for name, b in fields:
        dtype = _RECORD_TYPES[name][0]
        shape = (m, *_dims(name, k, b // _field_bytes(name, k)))        # (b // the bytes with M = 1: M, where the field has one)
        part = packed[off:off + m * b]
        out[name] = part.view(_NUMPY_TYPES[dtype]).reshape(shape) if host else part.view(dtype).view(shape)
        off += m * b
    return out


@dataclasses.dataclass(frozen=True)
class LoaderRequest:
    """What a caller asks of the device loader (net._loader, parallel._sharded_loader), in its four independent parts.  refine:
    the decoder.  candidates: None, or (M, nms_radius), the M best peaks of every heat-map.  cov_floor: None, or the floor of the
    covariance outputs, which the main record then carries.  select: None, or (thresh, min_k, weights), the solver-ready second
    record.  The constructor refuses what the public entries refuse, with their texts; everything the loader, the exchange and the
    solve need to know of the records is derived here, once."""
    refine: str = "get_final"
    candidates: tuple = None
    cov_floor: float = None
    select: tuple = None

    def __post_init__(self):
        check_refine(self.refine)
        if self.select is not None:
            thresh, min_k, weights = self.select
            check_weights(weights, self.refine)
            object.__setattr__(self, "select", (float(thresh), int(min_k), weights))
        if self.cov_floor is not None:
            if self.candidates is not None:
                _check_at_outputs(self.refine, False, False, True, self.cov_floor)
            elif self.refine != "gaussfit":
                raise ValueError("the covariance of the fitted centre belongs to the Gaussian-fit decoder")
            object.__setattr__(self, "cov_floor", check_cov_floor(self.cov_floor))
        if self.candidates is not None:
            mm, radius = self.candidates
            record_fields(1, "candidates", candidates=mm)                   # its range of M, with its text
            object.__setattr__(self, "candidates", (int(mm), int(radius)))

    @property
    def decoder(self) -> int:
        """The decoder's number in the ABI (include/esahrnet.h)."""
        return REFINES.index(self.refine)

    @property
    def main(self):
        """The main record, as record_fields takes it behind k: (kind, gaussfit, cov, candidates)."""
        gaussfit, cov = self.refine == "gaussfit", self.cov_floor is not None
        if self.candidates is None:
            return "keypoints", gaussfit, cov, None
        return "candidates" if self.refine == "get_final" else "candidates_refined", gaussfit, cov, self.candidates[0]

    @property
    def second(self):
        """The kind of the solver-ready record, None without select."""
        if self.select is None:
            return None
        return "correspondences" if self.candidates is None else "candidate_correspondences"

    @property
    def kinds(self):
        """The records of a result, in the order of their exchange: the second record, if any, first."""
        return tuple(kind for kind in (self.second, self.main[0]) if kind is not None)

    @property
    def mode(self) -> int:
        """The mode of esahrnet_correspondences[_cand]: 1 with a 2x2 weight from the decoder, 0 with the peak (or no select)."""
        return int(self.select is not None and self.select[2] != "peak")

    @property
    def hessian(self):
        """The field of the main record that the correspondence stage takes as the Hessian: hess, or info where the record carries
        the covariance outputs (weights="covariance": -cov^-1 in the Hessian's place); cand_hess or cand_info for the candidates;
        None with mode 0, and for get_final2 without candidates, where esahrnet_frames_correspondences forms the Hessian itself."""
        if not self.mode or (self.candidates is None and self.refine != "gaussfit"):
            return None
        return ("cand_" if self.candidates is not None else "") + ("info" if self.cov_floor is not None else "hess")

    def fields(self, k: int) -> dict:
        """kind -> record_fields(k, kind, ...) of every record of the result, in the order of `kinds`."""
        main = self.main
        return {kind: record_fields(k, *main) if kind == main[0] else record_fields(k, kind, candidates=main[3])
                for kind in self.kinds}


class LoaderResult:
    """What the loader answers: m crops of k keypoints, `records`: kind -> (packed uint8 buffer, fields), and r[name] the typed
    view (record_views) of a field, e.g. r["kp"], r["cand_hess"], r["count"]; the field names of a call's main and second record
    are disjoint, so one namespace (`views`: name -> tensor) holds both."""

    def __init__(self, m: int, k: int, records: dict):
        self.m, self.k, self.records = m, k, records
        self.views = {name: t for packed, fields in records.values() for name, t in record_views(packed, m, k, fields).items()}

    @classmethod
    def empty(cls, request: LoaderRequest, m: int, k: int, device):
        """The records of `request` for m crops, allocated on `device` and not initialised."""
        return cls(m, k, {kind: (torch.empty(m * sum(b for _, b in fields), dtype=torch.uint8, device=device), fields)
                          for kind, fields in request.fields(k).items()})

    def __getitem__(self, name):
        return self.views[name]

    def __contains__(self, name):
        return name in self.views

    def host(self, kind: str) -> dict:
        """A path's only device->host copy: ONE .cpu() of the record of `kind`, -> its numpy views (record_views)."""
        packed, fields = self.records[kind]
        return record_views(packed.cpu().numpy(), self.m, self.k, fields)


def candidate_returns(r: LoaderResult, return_hessian, return_fit, return_cov):
    """What net.frames_to_candidates returns, out of the loader's result: (cand, crop_boxes, rates, valid) and the decoder outputs
    asked for, in net.candidates' order."""
    names = ("cand", "boxes", "rates", "valid", *(("cand_fit", "cand_status") if return_fit else ()),
             *(("cand_hess",) if return_hessian else ()), *(("cand_cov", "cand_info") if return_cov else ()))
    return tuple(r[n] for n in names)


def packed_layout(m: int, k: int, gaussfit: bool = False, cov: bool = False, candidates=None, kind=None):
    """The packed buffer of net.frames_to_keypoints' outputs: name -> (offset, bytes), the fields of record_fields(k, "keypoints",
    gaussfit, cov) for m crops: rates f64 [m] | kp f32 [m,k,3] | crop_boxes int32 [m,4] | valid int32 [m] | idx int32 [m,k]; with
    gaussfit the decoder's f64 outputs come right behind rates (8-byte aligned) and its status last: rates | fit f64 [m,k,8] |
    hess f64 [m,k,3] | kp | crop_boxes | valid | idx | status int32 [m,k]; with cov (gaussfit only) cov f64 [m,k,3] | info f64
    [m,k,3] follow hess.  "total" -> (0, bytes of the buffer).  candidates=M (net.frames_to_candidates; not with gaussfit), the
    fields of record_fields(k, "candidates", candidates=M): rates | cand f32 [m,k,M,3] | crop_boxes | valid | cidx int32 [m,k,M].
    kind (default: "keypoints", or "candidates" with candidates=M) names another record of record_fields, "candidates_refined" among
    them."""
    out, off = {}, 0
    if kind is None:
        kind = "keypoints" if candidates is None else "candidates"
    for name, b in record_fields(k, kind, gaussfit, cov, candidates):
        out[name] = (off, m * b)
        off += m * b
    out["total"] = (0, off)
    return out


def pack_correspondences(m: int, k: int, device):
    """One uint8 buffer and its views count int32 [m] | order int32 [m,k] | pts f64 [m,k,2] | w f64 [m,k,3] (pts first in
    memory: 8-byte aligned), so that a caller fetches the whole record with one copy.  -> (count, order, pts, w, packed)."""
    fields = record_fields(k, "correspondences")
    packed = torch.empty(m * sum(b for _, b in fields), dtype=torch.uint8, device=device)
    v = record_views(packed, m, k, fields)
    return v["count"], v["order"], v["pts"], v["w"], packed


def unpack_correspondences(host: np.ndarray, m: int, k: int):
    """pack_correspondences' buffer, copied to the host -> (count, order, pts, w) as numpy views."""
    v = record_views(host, m, k, record_fields(k, "correspondences"))
    return v["count"], v["order"], v["pts"], v["w"]


def keypoints_to_correspondences(kp: torch.Tensor, crop_boxes: torch.Tensor, rates: torch.Tensor, valid: torch.Tensor,
                                 hess: torch.Tensor = None, thresh: float = 0.8, min_k: int = 24, weights: str = "peak"):
    """val.py:172-180 on the device (include/esahrnet.h esahrnet_correspondences): kp f32 cuda [m,K,3] and the crop boxes
    int32 [m,4], rates f64 [m] and valid int32 [m] of net.frames_to_keypoints / crops.crop_batch_device -> (count int32 [m],
    order int32 [m,K], pts f64 [m,K,2], w f64 [m,K,3]) on the device: what select_keypoints + crop_to_image give, bit for bit,
    and the weight of each point.  weights="hessian" takes hess f64 [m,K,3] (heatmaps_to_keypoints(..., return_hessian=True));
    weights="covariance" takes, as hess, the info f64 [m,K,3] of gaussfit_keypoints(..., return_cov=True): w = rate cov^(-1/2)."""
    mode = check_weights(weights, "gaussfit" if weights == "covariance" else "get_final2")
    if not (isinstance(kp, torch.Tensor) and kp.is_cuda and kp.dtype == torch.float32 and kp.dim() == 3 and kp.shape[2] == 3):
        raise ValueError("kp must be a float32 cuda tensor [m, K, 3]")
    m, k = kp.shape[:2]
    dev = kp.device
    for name, t, dt, shape in (("crop_boxes", crop_boxes, torch.int32, (m, 4)), ("rates", rates, torch.float64, (m,)),
                               ("valid", valid, torch.int32, (m,))) + ((("hess", hess, torch.float64, (m, k, 3)),) if mode else ()):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt and tuple(t.shape) == shape):
            raise ValueError(f"{name} must be a {dt} tensor {list(shape)} on {dev}")
    kp, crop_boxes, rates, valid = kp.contiguous(), crop_boxes.contiguous(), rates.contiguous(), valid.contiguous()
    hess = hess.contiguous() if mode else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        count, order, pts, w, _ = pack_correspondences(m, k, dev)
        _lib.check(_lib.lib().esahrnet_correspondences(kp.data_ptr(), hess.data_ptr() if mode else None, crop_boxes.data_ptr(),
                                                       rates.data_ptr(), valid.data_ptr(), m, k, float(thresh), int(min_k), mode,
                                                       count.data_ptr(), order.data_ptr(), pts.data_ptr(), w.data_ptr(),
                                                       C.c_void_p(stream)))
    return count, order, pts, w


def pack_candidate_correspondences(m: int, k: int, candidates: int, device):
    """One uint8 buffer and its views cpts f64 [m,k,M,2] | cw f64 [m,k,M,3] | cpeak f32 [m,k,M] | count int32 [m] | order int32
    [m,k] (record_fields(k, "candidate_correspondences", candidates=M)).  -> (cpts, cw, cpeak, count, order, packed)."""
    fields = record_fields(k, "candidate_correspondences", candidates=candidates)
    packed = torch.empty(m * sum(b for _, b in fields), dtype=torch.uint8, device=device)
    v = record_views(packed, m, k, fields)
    return v["cpts"], v["cw"], v["cpeak"], v["count"], v["order"], packed


def candidates_to_correspondences(cand: torch.Tensor, crop_boxes: torch.Tensor, rates: torch.Tensor, valid: torch.Tensor,
                                  thresh: float = 0.8, min_k: int = 24, weights: str = "peak", hess: torch.Tensor = None):
    """keypoints_to_correspondences for candidate rows (include/esahrnet.h esahrnet_correspondences_cand): cand f32 cuda [m,K,M,3]
    and the crop boxes int32 [m,4], rates f64 [m] and valid int32 [m] of net.frames_to_candidates -> (cpts f64 [m,K,M,2], cw f64
    [m,K,M,3], cpeak f32 [m,K,M], count int32 [m], order int32 [m,K]) on the device, views of one packed buffer: the selection by
    candidate 0's peak, then in rank order every candidate in image pixels with its 2x2 weight and its peak, the record
    pnp.candidate_correspondences_to_pose_batch solves on.  An absent runner-up (a NaN row) has a NaN point and weight zero; slots
    beyond count are zero.  weights="hessian" / "covariance" take, as hess, the f64 [m,K,M,3] Hessians / infos of
    frames_to_candidates(refine=..., return_hessian / return_cov=True): cw = rate (-hess)^(1/2) per candidate."""
    mode = check_weights(weights, "gaussfit" if weights == "covariance" else "get_final2")
    if not (isinstance(cand, torch.Tensor) and cand.is_cuda and cand.dtype == torch.float32 and cand.dim() == 4 and
            cand.shape[3] == 3):
        raise ValueError("cand must be a float32 cuda tensor [m, K, M, 3]")
    m, k, mm = cand.shape[:3]
    dev = cand.device
    for name, t, dt, shape in (("crop_boxes", crop_boxes, torch.int32, (m, 4)), ("rates", rates, torch.float64, (m,)),
                               ("valid", valid, torch.int32, (m,))) + ((("hess", hess, torch.float64, (m, k, mm, 3)),) if mode else ()):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt and tuple(t.shape) == shape):
            raise ValueError(f"{name} must be a {dt} tensor {list(shape)} on {dev}")
    cand, crop_boxes, rates, valid = cand.contiguous(), crop_boxes.contiguous(), rates.contiguous(), valid.contiguous()
    hess = hess.contiguous() if mode else None
    if not 1 <= mm <= _lib.MAX_CANDIDATES:
        raise ValueError(f"cand holds {mm} candidates per keypoint, supported are 1..{_lib.MAX_CANDIDATES}")
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        cpts, cw, cpeak, count, order, _ = pack_candidate_correspondences(m, k, mm, dev)
        _lib.check(_lib.lib().esahrnet_correspondences_cand(cand.data_ptr(), hess.data_ptr() if mode else None, crop_boxes.data_ptr(),
                                                            rates.data_ptr(), valid.data_ptr(), m, k, mm, float(thresh), int(min_k),
                                                            mode, count.data_ptr(), order.data_ptr(), cpts.data_ptr(),
                                                            cw.data_ptr(), cpeak.data_ptr(), C.c_void_p(stream)))
    return cpts, cw, cpeak, count, order


def _to_device(hm):
    if isinstance(hm, np.ndarray):
        assert hm.ndim == 4, 'batch_images should be 4-ndim'          # inference.py:29
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the keypoint kernel has no CPU fallback")
        return torch.from_numpy(np.ascontiguousarray(hm, dtype=np.float32)).cuda()
    return hm


def get_max_preds(batch_heatmaps):
    """inference.py:22-51 contract: -> (preds [N,K,2] f32 integer coordinates, maxvals [N,K,1]).
    Runs the same HIP kernel as heatmaps_to_keypoints (keypoints.hip), which also hands back the flat index of
    its first-occurrence arg-max: preds = (idx % W, idx // W), maxvals = the raw peak."""
    assert isinstance(batch_heatmaps, (np.ndarray, torch.Tensor)), \
        'batch_heatmaps should be numpy.ndarray'
    t = _to_device(batch_heatmaps)
    kp, idx = _keypoints(t, True)
    w = t.shape[3]
    idx = idx.cpu().numpy()
    preds = np.stack([(idx % w).astype(np.float32), (idx // w).astype(np.float32)], axis=2)
    return preds, kp[..., 2:3].cpu().numpy()


def get_final(hm, coords=None):
    """inference.py:136-152 contract for one sample: hm [1,K,H,W] -> refined preds [K,2].
    `coords` (the caller's integer arg-max list) is accepted and ignored: the fused kernel
    recomputes the identical arg-max.  get_final_at refines at the coords it is given."""
    t = _to_device(hm)
    kp = heatmaps_to_keypoints(t[:1])
    return kp[0, :, :2].cpu().numpy()


def get_final2(hm, coords=None):
    """inference.py:154-169 contract for one sample: hm [1,K,H,W] -> refined preds [K,2] (blur + full-Hessian Newton step).
    `coords` is accepted and ignored: the kernel recomputes the identical arg-max of the raw maps.  Unlike the reference,
    `hm` is NOT modified (the reference blurs the caller's array in place), and a plane whose maxima, rescale factor or
    offset are not finite keeps its integer coordinates.  get_final2_at refines at the coords it is given."""
    t = _to_device(hm)
    kp = heatmaps_to_keypoints(t[:1], refine="get_final2")
    return kp[0, :, :2].cpu().numpy()


def _coords_to_at(hm, coords):
    """coords [K,2] = integer-valued (x, y) inside the planes of hm [1,K,H,W] -> int32 tensor [1,K] = y * W + x (host)."""
    if len(hm.shape) != 4 or hm.shape[0] < 1:
        raise ValueError("expected heat-maps [1, K, H, W]")
    k, h, w = hm.shape[1:]
    c = np.asarray(coords.detach().cpu() if isinstance(coords, torch.Tensor) else coords, np.float64)
    if c.shape != (k, 2):
        raise ValueError(f"coords must be [{k}, 2] = (x, y) per heat-map, got {c.shape}")
    if not (np.isfinite(c).all() and (c == np.floor(c)).all()):
        raise ValueError("coords must be integer-valued pixels (x, y): the reference takes int(coord) of the arg-max it was handed")
    if not ((c >= 0).all() and (c[:, 0] < w).all() and (c[:, 1] < h).all()):
        raise ValueError(f"coords outside the {h} x {w} plane")
    at = c[:, 1].astype(np.int64) * w + c[:, 0].astype(np.int64)
    return torch.from_numpy(at.astype(np.int32)).reshape(1, k)


def get_final_at(hm, coords):
    """inference.py:136-152 with `coords` honoured: hm [1,K,H,W], coords [K,2] the integer-valued (x, y) to refine at (the
    reference's get_final(hm, coords) reads int(coord[0]), int(coord[1])) -> refined preds [K,2].  get_final ignores coords and
    refines at the arg-max; this one refines where it is told (refine_at).  Coordinates that are not integer-valued or lie outside
    the plane raise ValueError.  `hm` is not modified."""
    at = _coords_to_at(hm, coords)                     # (refusals first: they need no device)
    t = _to_device(hm)
    kp = refine_at(t[:1], at.to(t.device))
    return kp[0, :, :2].cpu().numpy()


def get_final2_at(hm, coords):
    """inference.py:154-169 with `coords` honoured, as get_final_at: blur, rescale by the plane's raw maximum over its blurred
    maximum, log, full-Hessian Newton step at the given pixel.  Unlike the reference `hm` is NOT modified, and a plane whose maxima,
    rescale factor or offset are not finite keeps its integer coordinates (as get_final2)."""
    at = _coords_to_at(hm, coords)
    t = _to_device(hm)
    kp = refine_at(t[:1], at.to(t.device), refine="get_final2")
    return kp[0, :, :2].cpu().numpy()


def select_keypoints(maxvals, thresh: float = 0.8, min_k: int = 24):
    """val.py:172-177 (thresh .8, at least 24) / demo.py:195-200 (thresh .6, min_k 0):
    indices of the keypoints handed to PnP, largest peak first."""
    mv = [float(v) for v in maxvals]
    large_k = int(np.sum(np.asarray(mv) > thresh))
    large_k = max(large_k, min_k)
    return heapq.nlargest(large_k, range(len(mv)), mv.__getitem__)


def crop_to_image(preds, rate, x, y):
    """val.py:180: ori_preds = preds * (1 / rate) + [x, y]."""
    return np.asarray(preds) * (1 / rate) + [x, y]
