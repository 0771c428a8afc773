"""Host-side mirror of the reference's model interface for the MI355X path.

Reference interface being mirrored:
  * models/seg_hrnet.py:495-499     get_seg_model(cfg, **kwargs) -> nn.Module
  * models/seg_hrnet.py:258-340     HighResolutionNet(config): parameters/buffers under the
                                    reference's state_dict keys (strict load_state_dict of a
                                    reference checkpoint works, val.py:64-66)
  * models/seg_hrnet.py:425-473     net(x: f32 [N,Cin,H,W]) -> f32 [N,K,H,W], same device
  * models/seg_hrnet.py:475-493     init_weights(pretrained)

The module owns ordinary torch parameters (so .cuda(), .parameters(), .state_dict(),
DataParallel's unwrap idiom `net.module.net` all behave), but forward() never runs a torch
operator: it folds BN into the convolutions once per weight version, hands them to
libesahrnet.so and enqueues the hand-written HIP kernels on torch's current stream.
There is no CPU or eager fallback: without the library or without a GPU, forward raises.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
import threading

import numpy as np
import torch
import torch.nn as nn

from . import _lib, crops
from .fold import fold_conv
from .inference import (LoaderRequest, LoaderResult, _at_returns, _check_at_outputs, candidate_returns, check_cov_floor,
                        check_refine, check_weights)

logger = logging.getLogger(__name__)
BN_MOMENTUM = 0.01           # models/seg_hrnet.py:23 (irrelevant at inference, kept for parity)


# "fp32" is the fp32-grade bf16x6 mode (the reference's arithmetic class, BASELINE configs[1]); "bf16x3" (split-bf16,
# ~16 significand bits) is an explicitly named opt-in and NOT an alias of fp32
# "fp16" is the single-pass mode with fp16 storage: bf16's cost, 11 significand bits, range +-65504 (saturating); seg_hrnet /
# seg_hrnet2 only
PRECISIONS = {"fp32": 2, "bf16x6": 2, "bf16x3": 0, "split-bf16": 0, "bf16": 1, "fp16": 3, 0: 0, 1: 1, 2: 2, 3: 3}


def _cfg_struct(config, cin: int, num_keypoints: int, variant: int = 0, precision=0) -> _lib.Cfg:
    extra = config.MODEL.EXTRA.HIGH_RESOLUTION_NET if hasattr(config, "MODEL") else \
        config["MODEL"]["EXTRA"]["HIGH_RESOLUTION_NET"]
    s = _lib.Cfg()
    s.cin, s.num_keypoints, s.stem_width, s.variant = cin, num_keypoints, 64, variant
    if precision not in PRECISIONS:
        raise ValueError(f"precision={precision!r}: expected one of {sorted(map(str, PRECISIONS))}")
    s.precision = PRECISIONS[precision]
    fk = extra["FINAL_CONV_KERNEL"] if "FINAL_CONV_KERNEL" in extra else 1
    s.final_conv_kernel = int(fk)
    for i in range(4):
        st = extra[f"STAGE{i + 1}"]
        if st["BLOCK"] != "BASIC":
            raise ValueError(f"STAGE{i + 1}.BLOCK={st['BLOCK']!r}: only BASIC blocks are built "
                             "(config/default.py:49-73 uses BASIC everywhere)")
        if st["FUSE_METHOD"] != "SUM":
            raise ValueError("only FUSE_METHOD='SUM' exists in the reference")
        nb = int(st["NUM_BRANCHES"])
        # same consistency checks as HighResolutionModule._check_branches (seg_hrnet.py:123-141)
        if nb != len(st["NUM_BLOCKS"]):
            raise ValueError("NUM_BRANCHES({}) <> NUM_BLOCKS({})".format(nb, len(st["NUM_BLOCKS"])))
        if nb != len(st["NUM_CHANNELS"]):
            raise ValueError("NUM_BRANCHES({}) <> NUM_CHANNELS({})".format(nb, len(st["NUM_CHANNELS"])))
        if nb != i + 1:
            raise ValueError(f"STAGE{i + 1} must have {i + 1} branches (got {nb})")
        s.modules[i] = int(st["NUM_MODULES"])
        for b in range(nb):
            s.blocks[i][b] = int(st["NUM_BLOCKS"][b])
            if i == 3:
                s.widths[b] = int(st["NUM_CHANNELS"][b])
            elif int(st["NUM_CHANNELS"][b]) != int(extra["STAGE4"]["NUM_CHANNELS"][b]):
                raise ValueError("branch widths must agree across stages")
    return s


class _Node(nn.Module):
    """Pure container used to reproduce the reference's dotted state_dict names."""


def _place(root: nn.Module, dotted: str, leaf: nn.Module):
    parts = dotted.split(".")
    cur = root
    for p in parts[:-1]:
        nxt = cur._modules.get(p)
        if nxt is None:
            nxt = _Node()
            cur.add_module(p, nxt)
        cur = nxt
    cur.add_module(parts[-1], leaf)


class HighResolutionNet(nn.Module):
    CIN = 3                  # models/seg_hrnet.py:265
    NUM_KEYPOINTS = 32       # models/seg_hrnet.py:324
    VARIANT = 0              # 1 = seg_hrnet3.py (CBAM)
    DEFAULT_PRECISION = "fp32"   # the reference computes in fp32 (models/seg_hrnet.py:425-473): fp32-grade bf16x6 by default

    def __init__(self, config, **kwargs):
        super().__init__()
        cin = int(kwargs.pop("cin", self.CIN))
        k = int(kwargs.pop("num_keypoints", self.NUM_KEYPOINTS))
        self._cin, self._k = cin, k
        # precision (include/esahrnet.h esahrnet_cfg.precision): "fp32" = "bf16x6" (default: fp32-grade, BASELINE
        # configs[1] / [2]), "bf16x3" (split-bf16, ~16 significand bits: explicit opt-in, ~1.7x faster), "bf16"
        # (single-pass bf16 storage / fp32 accumulate, BASELINE configs[3]), "fp16" (the same with fp16 storage, seg_hrnet /
        # seg_hrnet2 only: seg_hrnet3 raises the library's message)
        self._cfg_struct = _cfg_struct(config, cin, k, int(kwargs.pop("variant", self.VARIANT)),
                                       kwargs.pop("precision", self.DEFAULT_PRECISION))
        self.__dict__["_config"] = config      # calibrate_fp16 builds a bf16 twin from it
        object.__setattr__(self, "_rt", _Runtime(self._cfg_struct))
        self._descs = self._rt.conv_descs()
        for d in self._descs:
            conv = nn.Conv2d(d["cin"], d["cout"], d["k"], d["stride"], (d["k"] - 1) // 2, bias=d["has_bias"])
            _place(self, d["name"], conv)
            if d["bn"]:
                _place(self, d["bn"], nn.BatchNorm2d(d["cout"], momentum=BN_MOMENTUM))
        # parameters that are not convolutions of the main graph (seg_hrnet3: ChannelAttention.fc,
        # SpatialAttention.conv1); some names alias a conv that already exists (conv1.weight)
        self._aux = self._rt.aux_descs()
        have = set(dict(self.named_parameters()).keys())
        for a in self._aux:
            if a["name"] in have:
                continue
            co, ci, kh, kw = a["shape"]
            _place(self, a["name"][: -len(".weight")], nn.Conv2d(ci, co, (kh, kw), padding=(kh // 2, kw // 2), bias=False))
        self.eval()

    # ---- reference API -------------------------------------------------------------------------
    def init_weights(self, pretrained=""):
        logger.info("=> init weights from normal distribution")
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.001)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if os.path.isfile(pretrained):
            # weights_only: a checkpoint is data, nothing in it is executed
            pretrained_dict = torch.load(pretrained, map_location="cpu", weights_only=True)
            logger.info("=> loading pretrained model {}".format(pretrained))
            model_dict = self.state_dict()
            model_dict.update({k: v for k, v in pretrained_dict.items() if k in model_dict})
            self.load_state_dict(model_dict)

    def _inference_only(self):
        if self.training:
            raise RuntimeError("HighResolutionNet (MI355X path) is inference-only: call .eval() "
                               "(the reference callers do, val.py:95 / demo.py:80)")

    OUTPUTS = ("heatmaps", "keypoints", "keypoints+index")

    def forward(self, x0: torch.Tensor, output: str = "heatmaps", refine: str = "get_final"):
        """output="heatmaps" (default): f32 [N,K,H,W], the reference's forward.  "keypoints": f32 cuda [N,K,3] = (x, y, peak)
        without writing heat-maps (include/esahrnet.h esahrnet_forward_keypoints), bit-identical to
        inference.heatmaps_to_keypoints(net(x)); "keypoints+index": (kp, idx int32 [N,K] = row * W + column).
        refine="get_final2" (keypoint outputs only): the second decoder, bit-identical to
        inference.heatmaps_to_keypoints(net(x), refine="get_final2"), without writing heat-maps either
        (include/esahrnet.h esahrnet_forward_keypoints_final2).  refine="gaussfit": the Gaussian-fit decoder fused into the
        forward (esahrnet_forward_keypoints_gaussfit), the kp of keypoints_gaussfit."""
        self._inference_only()
        check_refine(refine)
        if output == "heatmaps":
            if refine != "get_final":
                raise ValueError(f"refine={refine!r} applies to output='keypoints' / 'keypoints+index' only")
            return self._rt.forward(self, x0)
        if output not in self.OUTPUTS:
            raise ValueError(f"output must be one of {self.OUTPUTS}, got {output!r}")
        if refine == "gaussfit":
            kp, _, _, _, idx = self._rt.forward_gaussfit(self, x0, False, output == "keypoints+index", want_hessian=False)
        elif refine == "get_final2":
            kp, idx = self._rt.forward_final2(self, x0, output == "keypoints+index")
        else:
            kp, idx = self._rt.forward_keypoints(self, x0, output == "keypoints+index")
        return (kp, idx) if output == "keypoints+index" else kp

    def keypoints(self, x0: torch.Tensor) -> torch.Tensor:
        """net(x, output="keypoints"): f32 cuda [N,K,3] keypoints straight from the crops."""
        return self(x0, output="keypoints")

    def frames_to_keypoints(self, frames: torch.Tensor, det_boxes, frame_idx=None, scale: int = 256, rule: str = "val",
                            refine: str = "get_final", mean=None, std: float = crops.STD, pixel_format=None):
        """Camera frames and raw detector boxes to keypoints in one library call (include/esahrnet.h
        esahrnet_frames_keypoints): box rule, crops, forward and decoder on the device, nothing allocated or synchronised in
        between, capturable into a graph.  Arguments as crops.crop_batch_device; mean defaults to the rule's loader
        (crops.MEAN_VAL / crops.MEAN_TRAIN).  -> (kp f32 [m,K,3], crop_boxes int32 [m,4], rates f64 [m], valid int32 [m]),
        all on the device; kp equals crops.crop_batch -> net(x, output="keypoints", refine=refine) bit for bit, except that
        the rows of an invalid crop (empty box, frame index out of range: valid == 0) are NaN."""
        self._inference_only()
        r = self._loader(LoaderRequest(refine), frames, det_boxes, frame_idx, scale, rule, mean, std, pixel_format)
        return r["kp"], r["boxes"], r["rates"], r["valid"]

    def frames_to_correspondences(self, frames: torch.Tensor, det_boxes, frame_idx=None, scale: int = 256, rule: str = "val",
                                  refine: str = "get_final", thresh: float = 0.8, min_k: int = 24, weights: str = "peak",
                                  mean=None, std: float = crops.STD, pixel_format=None, cov_floor: float = 1e-6):
        """frames_to_keypoints and val.py:172-180 behind it in one library call (include/esahrnet.h
        esahrnet_frames_correspondences): -> (count int32 [m], order int32 [m,K], pts f64 [m,K,2], w f64 [m,K,3], kp, crop_boxes,
        rates, valid), all on the device.  The first four are the record the host pose solver consumes
        (pnp.correspondences_to_pose_batch): the keypoints handed to PnP, largest peak first, in image pixels, each with its
        2x2 weight (wxx, wxy, wyy) — weights="peak": (peak, 0, peak); "hessian" (refine="get_final2" or "gaussfit"): the
        decoder's Hessian as an information matrix, rate * (-H)^(1/2).  Equal, bit for bit, to frames_to_keypoints followed by
        inference.keypoints_to_correspondences; capturable into a graph.  refine="gaussfit": two library calls on one stream
        (esahrnet_frames_keypoints_gaussfit, then esahrnet_correspondences on its outputs).  weights="covariance"
        (refine="gaussfit" only): esahrnet_frames_keypoints_gaussfit_cov, then esahrnet_correspondences(mode 1) with its info
        output: w = rate cov^(-1/2), the covariance of the fitted centre (inference.gaussfit_keypoints return_cov=True), zero
        where cov[0] < cov_floor."""
        self._inference_only()
        request = LoaderRequest(refine, None, cov_floor if weights == "covariance" else None, (thresh, min_k, weights))
        r = self._loader(request, frames, det_boxes, frame_idx, scale, rule, mean, std, pixel_format)
        return r["count"], r["order"], r["pts"], r["w"], r["kp"], r["boxes"], r["rates"], r["valid"]

    def keypoints_hessian(self, x0: torch.Tensor):
        """net(x, output="keypoints+index", refine="get_final2") with the Hessian of each step: -> (kp f32 [N,K,3], idx int32
        [N,K], hess f64 [N,K,3] = (dxx, dxy, dyy), NaN where no step was taken), bit-identical to
        inference.heatmaps_to_keypoints(net(x), refine="get_final2", return_hessian=True), without heat-maps in caller memory
        (include/esahrnet.h esahrnet_forward_keypoints_final2_hess)."""
        self._inference_only()
        return self._rt.forward_final2(self, x0, True, want_hessian=True)

    def keypoints_gaussfit(self, x0: torch.Tensor, return_fit: bool = False, return_cov: bool = False, cov_floor: float = 1e-6):
        """The forward with the Gaussian-fit decoder in place of its last launch (include/esahrnet.h
        esahrnet_forward_keypoints_gaussfit): -> (kp f32 [N,K,3], status int32 [N,K], hess f64 [N,K,3] = (-2a, -2b, -2c)), or
        with return_fit=True (kp, fit f64 [N,K,8], status, hess); bit-identical to inference.gaussfit_keypoints(net(x)), without
        heat-maps in caller memory.  return_cov=True (esahrnet_forward_keypoints_gaussfit_cov) appends (cov, info) f64 [N,K,3]
        each, the covariance of the fitted centre and -cov^-1 as inference.gaussfit_keypoints(net(x), return_cov=True,
        cov_floor=cov_floor) gives them, bit for bit; the other outputs keep their bits."""
        self._inference_only()
        if return_cov:
            kp, fit, status, hess, _, cov, info = self._rt.forward_gaussfit(self, x0, bool(return_fit), False,
                                                                            cov=check_cov_floor(cov_floor))
            return (kp, fit, status, hess, cov, info) if return_fit else (kp, status, hess, cov, info)
        kp, fit, status, hess, _ = self._rt.forward_gaussfit(self, x0, bool(return_fit), False)
        return (kp, fit, status, hess) if return_fit else (kp, status, hess)

    def candidates(self, x0: torch.Tensor, candidates: int = 3, nms_radius: int = 6, return_index: bool = False,
                   refine: str = "get_final", return_hessian: bool = False, return_fit: bool = False, return_cov: bool = False,
                   cov_floor: float = 1e-6):
        """The forward with the candidate decoder in place of its last launch (include/esahrnet.h
        esahrnet_forward_keypoints_candidates): -> cand f32 cuda [N,K,M,3] = (x, y, peak), the M = `candidates` (1..4) best peaks of
        every heat-map, `nms_radius` pixels apart, best first; with return_index=True (cand, cidx int32 [N,K,M]).  Bit-identical to
        inference.heatmaps_to_candidates(net(x), candidates, nms_radius, return_index), without heat-maps in caller memory (they
        live in the workspace: the runner-up rule needs whole planes).
        refine="get_final2" / "gaussfit" and return_hessian / return_fit / return_cov (esahrnet_forward_keypoints_candidates_refined):
        every candidate refined by that decoder at its own pixel, still in the one call; -> the tuple
        inference.heatmaps_to_candidates(net(x), ...) returns for the same keywords, in the same order and bit for bit."""
        self._inference_only()
        decoder, cov_floor = _check_at_outputs(refine, return_hessian, return_fit, return_cov, cov_floor)
        if decoder == 0:                    # (get_final takes none of the optional outputs: _check_at_outputs has refused them)
            cand, cidx = self._rt.forward_candidates(self, x0, int(candidates), int(nms_radius), bool(return_index))
            return (cand, cidx) if return_index else cand
        cand, cidx, o = self._rt.forward_candidates_refined(self, x0, int(candidates), int(nms_radius), bool(return_index), decoder,
                                                            bool(return_hessian), bool(return_fit), bool(return_cov), cov_floor)
        out = (cand, *((cidx,) if return_index else ()), *_at_returns(o, return_hessian, return_fit, return_cov))
        return out if len(out) > 1 else cand

    def frames_to_candidates(self, frames: torch.Tensor, det_boxes, frame_idx=None, scale: int = 256, rule: str = "val",
                             candidates: int = 3, nms_radius: int = 6, mean=None, std: float = crops.STD, pixel_format=None,
                             refine: str = "get_final", return_hessian: bool = False, return_fit: bool = False,
                             return_cov: bool = False, cov_floor: float = 1e-6):
        """frames_to_keypoints with the candidate decoder (include/esahrnet.h esahrnet_frames_keypoints_candidates): box rule,
        crops, forward and the M best peaks of every heat-map in one library call.  -> (cand f32 [m,K,M,3], crop_boxes int32 [m,4],
        rates f64 [m], valid int32 [m]), all on the device; cand equals crops.crop_batch -> net.candidates(x, candidates,
        nms_radius) bit for bit, except that the rows of an invalid crop (valid == 0) are NaN.
        refine="get_final2" / "gaussfit" (esahrnet_frames_keypoints_candidates_refined): every candidate refined at its own pixel;
        the outputs asked for follow in net.candidates' order, [fit f64 [m,K,M,8], status int32 [m,K,M]], [hess f64 [m,K,M,3]],
        [cov, info f64 [m,K,M,3]], equal to crops.crop_batch -> net.candidates(x, ..., refine=...) bit for bit; in the rows of an
        invalid crop the f64 outputs are NaN and status is -1."""
        self._inference_only()
        _check_at_outputs(refine, return_hessian, return_fit, return_cov, cov_floor)
        request = LoaderRequest(refine, (candidates, nms_radius), cov_floor if return_cov else None)
        r = self._loader(request, frames, det_boxes, frame_idx, scale, rule, mean, std, pixel_format)
        return candidate_returns(r, return_hessian, return_fit, return_cov)

    def frames_to_candidate_correspondences(self, frames: torch.Tensor, det_boxes, frame_idx=None, scale: int = 256,
                                            rule: str = "val", refine: str = "get_final", candidates: int = 3, nms_radius: int = 6,
                                            thresh: float = 0.8, min_k: int = 24, weights: str = "peak", mean=None,
                                            std: float = crops.STD, pixel_format=None, cov_floor: float = 1e-6):
        """frames_to_candidates and the selection, back-projection and weights of val.py:172-180 behind it, for every candidate:
        -> (cpts f64 [m,K,M,2], cw f64 [m,K,M,3], cpeak f32 [m,K,M], count int32 [m], order int32 [m,K], cand, crop_boxes, rates,
        valid), all on the device.  The first five are the record pnp.candidate_correspondences_to_pose_batch solves on
        (inference.record_fields(K, "candidate_correspondences", candidates=M)): the keypoints handed to PnP by their primary's
        peak, largest first, and in that order every candidate in image pixels with its 2x2 weight -- weights="peak": (peak, 0,
        peak); "hessian" (refine="get_final2" or "gaussfit"): rate * (-H)^(1/2) of the candidate's own Hessian; "covariance"
        (refine="gaussfit"): rate * cov^(-1/2) of its fitted centre, zero where cov[0] < cov_floor -- and its peak.  Two library
        calls on one stream (esahrnet_frames_keypoints_candidates[_refined], then esahrnet_correspondences_cand on its outputs);
        equal, bit for bit, to frames_to_candidates(refine=...) followed by inference.candidates_to_correspondences; capturable
        into a graph.  An invalid crop has count 0."""
        self._inference_only()
        check_weights(weights, refine)
        _check_at_outputs(refine, weights == "hessian", False, weights == "covariance", cov_floor)
        request = LoaderRequest(refine, (candidates, nms_radius), cov_floor if weights == "covariance" else None,
                                (thresh, min_k, weights))
        r = self._loader(request, frames, det_boxes, frame_idx, scale, rule, mean, std, pixel_format)
        return r["cpts"], r["cw"], r["cpeak"], r["count"], r["order"], r["cand"], r["boxes"], r["rates"], r["valid"]

    def _loader(self, request: LoaderRequest, frames, det_boxes, frame_idx, scale, rule, mean, std, pixel_format) -> LoaderResult:
        """The one loader call behind the four public ones (and parallel._sharded_loader, pipeline): the records `request` asks
        for, every field a view of its record's one uint8 buffer (r["kp"], r["cidx"], r["count"], ...), so a caller that needs a
        record on the host fetches it with one copy (LoaderResult.host).  The main record holds everything its decoder writes
        (idx / cidx, a fit's parameters and status, the candidates' Hessians) whether or not a public call returns it; the rows
        of an invalid crop are NaN, its cidx and status -1, its count 0."""
        self._inference_only()
        rule_n, fmt, m = crops.check_device_loader_args(frames, det_boxes, frame_idx, rule, pixel_format)
        if mean is None:                    # the rule's loader
            mean = crops.MEAN_TRAIN if rule == "train" else crops.MEAN_VAL
        return self._rt.frames_keypoints(self, request, frames, det_boxes, frame_idx, m, int(scale), rule_n, fmt, float(mean),
                                         float(std))

    # ---- extras of the MI355X path ---------------------------------------------------------------
    @property
    def num_keypoints(self):
        return self._k

    def flops_per_crop(self, h: int, w: int) -> float:
        return self._rt.flops_per_crop(h, w)

    def launch_count(self) -> int:
        return self._rt.launch_count()

    def forward_timed(self, x0: torch.Tensor):
        """Measurement: one forward with every launch bracketed by HIP events on the current
        stream -> (heatmaps, [dict(kernel, label, ms, flops, bytes)] per launch)."""
        return self._rt.forward_timed(self, x0)

    def taps(self, x0: torch.Tensor) -> dict:
        """Debug: run a forward keeping every intermediate; returns {name: f32 NCHW tensor}."""
        return self._rt.taps(self, x0)

    def activation_stats(self, x0: torch.Tensor) -> "ActivationStats":
        """The activation range report of one forward (include/esahrnet.h: esahrnet_forward_stats): every tensor of the plan
        scanned on the device where the forward left it, one 64-byte record per (tensor, crop), one device -> host copy.
        Which precision can these weights afford: see ActivationStats.headroom_fp16, saturated, first_nonfinite."""
        return self._rt.forward_stats(self, x0)

    def precision_report(self, x0: torch.Tensor, reference=None) -> "PrecisionReport":
        """What this net's precision costs on its own weights and these crops, tensor by tensor (include/esahrnet.h:
        esahrnet_forward_diff): the crops go through this net and through `reference`, every tensor of both
        plans is kept, and a two-operand scan leaves one 64-byte error record per (tensor, crop); one device -> host copy.
        reference=None: an fp32-grade twin of the same class and configuration, built from this net's state dict and closed
        again.  A caller's own net (same configuration; any precision, but only tensors the reference stores in f32 and the
        heat-maps are compared) is left as it is."""
        self._inference_only()
        if reference is not None:
            return self._rt.forward_diff(self, reference, x0)
        twin = type(self)(self._config, cin=self._cin, num_keypoints=self._k, variant=self._cfg_struct.variant, precision="fp32")
        try:
            twin.load_state_dict(self.state_dict())
            twin.to(x0.device).eval()
            return self._rt.forward_diff(self, twin, x0)
        finally:
            twin._rt.close()            # its handles, packed weights and scratch, now

    # ---- fp16 scale exponents (include/esahrnet.h: fp16 scale groups) ---------------------------------
    @property
    def fp16_scale_groups(self):
        """Names of the handle's scale groups, in the library's order ("stream0", "stem1", "head0", a conv1's name, ...); ()
        for a network without them (seg_hrnet3, the 32-bit formats)."""
        return self._rt.scale_group_names()

    @property
    def fp16_exponents(self):
        """One exponent per scale group: the tensors of group g are stored as T * 2^-e[g] and the weights absorb the
        difference, so the heat-maps keep their scale.  All zero unless set (or calibrated: calibrate_fp16)."""
        e = self.__dict__.get("_fp16_exp")
        return tuple(e) if e is not None else (0,) * len(self.fp16_scale_groups)

    @fp16_exponents.setter
    def fp16_exponents(self, exponents):
        e = [int(v) for v in exponents]
        self._rt.check_scale_exponents(e)           # the library's refusals (count, range, precision), raised here
        self.__dict__["_fp16_exp"] = e
        self.invalidate_weights()                   # every device's handle re-commits on its next call

    def calibrate_fp16(self, x_or_batches, headroom_bits: int = 3) -> "Fp16Calibration":
        """Choose and set the scale exponents of an fp16 net from calibration crops (one cuda tensor [N,Cin,H,W] or several).
        A temporary bf16 twin — the same plan row for row, with f32's exponent range, so nothing saturates or underflows in
        it — runs one range-scanning forward per batch (esahrnet_forward_stats_h0: every stored tensor, and the h0 the fused
        head rounds in registers); the library turns the records into one exponent per group, the largest magnitude of a
        group landing in (2^(14 - headroom_bits), 2^(15 - headroom_bits)]; the exponents are set on this net, which then
        runs one verifying scan per batch: no stored value and no h0 may reach 65504 (RuntimeError naming the rows).  A
        weight the shift pushes out of fp16's range is the library's commit error, passed through."""
        self._inference_only()
        if self._cfg_struct.precision != PRECISIONS["fp16"]:
            raise ValueError("calibrate_fp16 belongs to precision='fp16' (the other formats have f32's exponent range)")
        batches = [x_or_batches] if isinstance(x_or_batches, torch.Tensor) else list(x_or_batches)
        if not batches:
            raise ValueError("calibrate_fp16 needs at least one batch of crops")
        twin = type(self)(self._config, cin=self._cin, num_keypoints=self._k, variant=self._cfg_struct.variant, precision="bf16")
        try:
            twin.load_state_dict(self.state_dict())
            twin.to(batches[0].device)
            scans = [twin._rt.forward_stats(twin, x, with_h0=True) for x in batches]
            n, _, hh, ww = batches[0].shape
            mine = self._rt.stats_rows(self._rt._probe, n, hh, ww)
            if [d.name for d in mine] != [d.name for d in scans[0].descs]:
                raise RuntimeError("calibrate_fp16: the bf16 twin's report rows are not the fp16 net's")
            exps = twin._rt.exponents_from_stats(np.concatenate([st.per_image for st in scans], axis=1),
                                                 np.concatenate([st.h0 for st in scans]), int(headroom_bits))
        finally:
            twin._rt.close()            # its handles, packed weights and scratch, now
        self.fp16_exponents = exps
        names = self.fp16_scale_groups
        stored = [0.0] * len(names)
        bad = []
        for x in batches:
            st = self._rt.forward_stats(self, x, with_h0=True)
            bad += [r["name"] for r in st.saturated() if r["group"] >= 0]       # (the f32 heat-maps are no fp16 store)
            if int(st.h0["n_ge_f16max"].astype(np.int64).sum()):
                bad.append("h0")
            for r in st.scanned():
                if r["group"] >= 0:
                    stored[r["group"]] = max(stored[r["group"]], r["max_abs"])
            if "head0" in names:        # h0 is formed at the scale of its group: the record is a stored magnitude as it stands
                stored[names.index("head0")] = max(stored[names.index("head0")], float(st.h0["max_abs"].max()))
        if bad:
            raise RuntimeError(f"calibrate_fp16: values still reach 65504 under exponents {tuple(exps)} in {sorted(set(bad))}; "
                               "raise headroom_bits or calibrate on crops that cover the deployment's range")
        return Fp16Calibration(tuple(exps), tuple(names), tuple(stored), int(headroom_bits))

    # ---- weight-version tracking (an eager forward must not walk the module tree: val.py:112 calls the
    # net once per image) ---------------------------------------------------------------------------
    def _weight_tensors(self):
        """Flat list of every parameter and buffer, rebuilt only after the module was converted
        (`_apply`: .cuda()/.to()/.float()) or re-loaded."""
        ts = self.__dict__.get("_wt_cache")
        if ts is None:
            ts = [t for t in self.state_dict(keep_vars=True).values()]
            self.__dict__["_wt_cache"] = ts
        return ts

    def _weights_key(self):
        """What the folded/packed weights on a device are valid for: "the weights are what the Parameters
        say" (the reference's semantics).  load_state_dict, init_weights and every conversion
        (.cuda()/.to()/.float()) bump the epoch through the hooks below; an in-place edit of ANY parameter or
        buffer (under no_grad, by an optimizer step, ...) is seen through that tensor's autograd version
        counter: the key holds all of them (~40 us per forward for 539 tensors, 1.5 % of a batch-32 step).
        Only writes through `.data` / `.detach()` aliases are invisible to version counters: call
        invalidate_weights() after those.  A caller that runs the net once per image (val.py:112) and never
        touches the weights can drop the walk with freeze_weights()."""
        ts = self._weight_tensors()
        if self.__dict__.get("_wt_frozen", False):
            return (self.__dict__.get("_wt_epoch", 0),)
        return (self.__dict__.get("_wt_epoch", 0), *[t._version for t in ts])

    def freeze_weights(self, frozen: bool = True):
        """Opt-in fast path for per-image loops: promise that no parameter or buffer is edited in place until
        freeze_weights(False) / invalidate_weights() / load_state_dict() / a conversion; the forward then checks
        the epoch only (1 us instead of 40 us of host time)."""
        self.invalidate_weights()               # whatever was edited before the promise is folded in once
        self.__dict__["_wt_frozen"] = bool(frozen)
        return self

    def invalidate_weights(self):
        """Force a re-fold on the next forward (see _weights_key)."""
        self.__dict__["_wt_cache"] = None
        self.__dict__["_wt_epoch"] = self.__dict__.get("_wt_epoch", 0) + 1

    def _apply(self, fn, *a, **kw):
        r = super()._apply(fn, *a, **kw)
        self.invalidate_weights()
        return r

    def load_state_dict(self, *a, **kw):
        r = super().load_state_dict(*a, **kw)
        self.invalidate_weights()
        return r

    def release_workspaces(self):
        """Drop the cached scratch tensors of eager forwards (HIP graphs own theirs, see _Runtime)."""
        self._rt.release_workspaces()

    def _replicate_for_data_parallel(self):
        # nn.DataParallel (val.py:382, main.py:254): a replica has no Parameters of its own (torch re-attaches
        # broadcast copies as plain attributes), so it keeps a reference to the module it was made from and
        # the shared runtime folds THAT module's weights once per device.
        r = super()._replicate_for_data_parallel()
        object.__setattr__(r, "_rt", self._rt)
        r.__dict__["_master"] = self.__dict__.get("_master", self)
        return r


class _Runtime:
    """One libesahrnet handle per device + caller-owned workspace tensors.

    Shared by a module and its DataParallel replicas (one Python thread per device): everything that
    mutates the tables below happens under `self.lock`; the launches themselves run outside it, one
    handle per device, so replicas do not serialise each other."""

    WS_SHAPES_PER_DEVICE = 4     # eager scratch tensors kept per device (LRU)
    # workspace kind -> (the cache its tensors live in, its size query, that query's arguments between the handle and the result).
    # The loader's kinds take n crops of hh x hh, share one cache and are told apart by the key's `keep`: the decoder,
    # "gaussfit", or (decoder, mode) with the correspondences
    _crops = lambda n, hh, ww, keep: (n, hh, ww)      # noqa: E731  (used by the table below only)
    WS_KINDS = {
        "forward": ("forward", "esahrnet_workspace_bytes", _crops),
        "keypoints": ("keypoints", "esahrnet_keypoints_workspace_bytes", _crops),
        "final2": ("final2", "esahrnet_keypoints_final2_forward_workspace_bytes", _crops),
        "gaussfit": ("gaussfit", "esahrnet_keypoints_gaussfit_forward_workspace_bytes", _crops),
        "candidates": ("candidates", "esahrnet_keypoints_candidates_forward_workspace_bytes", _crops),
        # (the refined candidates: the key's `keep` is ("refined", decoder), the decoder the query's last argument)
        "candidates_refined": ("candidates", "esahrnet_keypoints_candidates_refined_forward_workspace_bytes",
                               lambda n, hh, ww, keep: (n, hh, ww, keep[1])),
        "frames_candidates_refined": ("frames", "esahrnet_frames_keypoints_candidates_refined_workspace_bytes",
                                      lambda n, hh, ww, keep: (n, hh, keep[1])),
        "frames": ("frames", "esahrnet_frames_keypoints_workspace_bytes", lambda n, hh, ww, keep: (n, hh, 0)),
        "frames_candidates": ("frames", "esahrnet_frames_keypoints_candidates_workspace_bytes", lambda n, hh, ww, keep: (n, hh)),
        "frames_final2": ("frames", "esahrnet_frames_keypoints_workspace_bytes", lambda n, hh, ww, keep: (n, hh, 1)),
        "frames_gaussfit": ("frames", "esahrnet_frames_keypoints_gaussfit_workspace_bytes", lambda n, hh, ww, keep: (n, hh)),
        "corr": ("frames", "esahrnet_frames_correspondences_workspace_bytes", lambda n, hh, ww, keep: (n, hh, *keep)),
        "stats": ("stats", "esahrnet_forward_stats_workspace_bytes", _crops),
        "stats_h0": ("stats", "esahrnet_forward_stats_h0_workspace_bytes", _crops),
        # (the key's `keep` is the reference handle's address: both forwards and the partials live in this one workspace)
        "diff": ("diff", "esahrnet_forward_diff_workspace_bytes", lambda n, hh, ww, keep: (C.c_void_p(keep), n, hh, ww)),
    }

    def __init__(self, cfg_struct):
        self.cfg = cfg_struct
        self.lib = _lib.lib()
        self.lock = threading.RLock()
        self.handles = {}        # device index -> (handle, weight-version key)
        self.dev_locks = {}      # device index -> lock serialising the enqueues of that device's handle
        self.ws = {}             # cache name (WS_KINDS) -> {(device, stream, n, h, w, keep): uint8 tensor}, insertion order = LRU order
        self.part_tiles = {}     # (handle, h, w) -> tiles per heat-map with partial maxima (0: none)
        self._probe = self._create(-1)

    def use_library(self, other):
        """Run this runtime through another build of the library (_lib.load_other), for A/B timing of the entries both have.
        Only before the first forward: no handle of the first library may exist yet."""
        if self.handles:
            raise RuntimeError("use_library: this runtime already holds handles of its library")
        self.lib.esahrnet_destroy(self._probe)
        self.lib = other
        self._probe = self._create(-1)

    def _create(self, device):
        h = C.c_void_p()
        _lib.check(self.lib.esahrnet_create(C.byref(self.cfg), max(device, 0), C.byref(h)))
        return h

    def close(self):
        """Destroy every handle (their packed weights on the devices) and drop the scratch; the runtime is unusable afterwards."""
        with self.lock:
            for h, _ in self.handles.values():
                self.lib.esahrnet_destroy(h)
            self.handles.clear()
            self.ws.clear()
            if self._probe is not None:
                self.lib.esahrnet_destroy(self._probe)
                self._probe = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def aux_descs(self):
        out = []
        for i in range(self.lib.esahrnet_aux_count(self._probe)):
            d = _lib.AuxDesc()
            _lib.check(self.lib.esahrnet_aux_desc_get(self._probe, i, C.byref(d)))
            out.append(dict(name=d.name.decode(), shape=tuple(d.shape)))
        return out

    def conv_descs(self):
        out = []
        for i in range(self.lib.esahrnet_conv_count(self._probe)):
            d = _lib.ConvDesc()
            _lib.check(self.lib.esahrnet_conv_desc_get(self._probe, i, C.byref(d)))
            out.append(dict(name=d.name.decode(), bn=d.bn.decode(), cin=d.cin, cout=d.cout, k=d.k,
                            stride=d.stride, has_bias=bool(d.has_bias), relu=bool(d.relu)))
        return out

    def scale_group_names(self):
        g = C.c_int(0)
        _lib.check(self.lib.esahrnet_scale_groups(self._probe, C.byref(g)))
        buf = C.create_string_buffer(96)
        names = []
        for i in range(g.value):
            _lib.check(self.lib.esahrnet_scale_group_name(self._probe, i, buf, 96))
            names.append(buf.value.decode())
        return tuple(names)

    def check_scale_exponents(self, exps):
        """esahrnet_set_scale_exponents on the probe handle (host only): its refusals, before anything is kept."""
        arr = (C.c_int32 * len(exps))(*exps)
        _lib.check(self.lib.esahrnet_set_scale_exponents(self._probe, arr, len(exps)))

    def exponents_from_stats(self, records, h0, headroom_bits):
        """esahrnet_scale_exponents_from_stats: records [rows, n_total] and h0 [n_total] (structured, _lib.stats_dtype)."""
        def laid_out(a):            # numpy drops a structured type's padding when it concatenates: back to the 64-byte record
            out = np.zeros(a.shape, dtype=_lib.stats_dtype())
            for name, _ in _lib.STATS_FIELDS:
                out[name] = a[name]
            return out

        records = laid_out(records)
        h0 = None if h0 is None else laid_out(h0)
        g = len(self.scale_group_names())
        out = (C.c_int32 * g)()
        _lib.check(self.lib.esahrnet_scale_exponents_from_stats(
            self._probe, records.ctypes.data_as(C.c_void_p), records.shape[0], records.shape[1],
            None if h0 is None else h0.ctypes.data_as(C.c_void_p), headroom_bits, out, g))
        return [int(v) for v in out]

    def flops_per_crop(self, h, w):
        f = C.c_double()
        _lib.check(self.lib.esahrnet_flops_per_crop(self._probe, h, w, C.byref(f)))
        return f.value

    def launch_count(self):
        return self.lib.esahrnet_launch_count(self._probe)

    def _handle_for(self, module, device):
        master = module.__dict__.get("_master", module)     # a DataParallel replica folds its master's weights
        key = master._weights_key()
        ent = self.handles.get(device.index)
        if ent is not None and ent[1] == key:
            return ent[0]
        with self.lock:
            ent = self.handles.get(device.index)
            if ent is not None and ent[1] == key:
                return ent[0]
            h = ent[0] if ent is not None else self._create(device.index)
            sd = master.state_dict()
            for i, d in enumerate(master._descs):
                w, b = fold_conv(sd, d["name"], d["bn"], d["has_bias"])
                _lib.check(self.lib.esahrnet_set_conv(h, i, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
            for i, a in enumerate(master._aux):
                w = np.ascontiguousarray(sd[a["name"]].detach().cpu().float().numpy())
                _lib.check(self.lib.esahrnet_set_aux(h, i, w.ctypes.data_as(C.c_void_p)))
            exps = master.__dict__.get("_fp16_exp")
            if exps is not None:        # fp16 scale exponents: folded into the weights by the commit below
                _lib.check(self.lib.esahrnet_set_scale_exponents(h, (C.c_int32 * len(exps))(*exps), len(exps)))
            with torch.cuda.device(device):
                _lib.check(self.lib.esahrnet_commit(h))
            self.handles[device.index] = (h, key)
            return h

    def _check_input(self, module, x0):
        if not isinstance(x0, torch.Tensor) or x0.dim() != 4:
            raise ValueError("expected a 4-D tensor [N, Cin, H, W]")
        if not x0.is_cuda:
            raise RuntimeError("the MI355X HRNet path runs only on a GPU tensor; there is no CPU "
                               "fallback (move the model and the crops to 'cuda')")
        if x0.dtype != torch.float32:
            raise TypeError(f"expected float32 crops, got {x0.dtype}")
        if x0.shape[1] != module._cin:
            raise ValueError(f"expected {module._cin} input channels, got {x0.shape[1]}")
        if "_master" not in module.__dict__:     # (a replica runs wherever DataParallel scattered its input)
            p = module._weight_tensors()[0]
            if p.device != x0.device:
                raise RuntimeError(f"input on {x0.device} but parameters on {p.device}")
        return x0.contiguous()

    def release_workspaces(self):
        with self.lock:
            self.ws.clear()

    def ws_cache(self, kind):
        """The cached scratch tensors of one workspace kind (WS_KINDS): {(device, stream, n, h, w, keep): uint8 tensor}."""
        return self.ws.setdefault(self.WS_KINDS[kind][0], {})

    def _workspace(self, h, device, stream, n, hh, ww, keep, kind="forward"):
        """Scratch for one forward.  Contract: while the stream is being CAPTURED into a HIP
        graph the scratch is a fresh tensor allocated inside the capture (the graph's private pool owns it, like
        any temporary of a captured torch op) and is never cached, so no graph ever holds a pointer into the
        eager cache; eager forwards share a small per-device LRU of scratch tensors, keyed by stream and shape
        (two streams never share scratch) and protected by record_stream."""
        nbytes = C.c_size_t()
        _, query, args = self.WS_KINDS[kind]
        _lib.check(getattr(self.lib, query)(h, *args(n, hh, ww, keep), C.byref(nbytes)))
        cache = self.ws_cache(kind)
        if torch.cuda.is_current_stream_capturing():
            ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=device)
        else:
            key = (device.index, stream.cuda_stream, n, hh, ww, keep)
            with self.lock:
                ws = cache.pop(key, None)
                if ws is None or ws.numel() < nbytes.value + 256:
                    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=device)
                cache[key] = ws                                      # most recently used last
                mine = [k for k in cache if k[0] == device.index]
                for k in mine[: max(0, len(mine) - self.WS_SHAPES_PER_DEVICE)]:
                    del cache[k]
        off = (-ws.data_ptr()) % 256
        return ws, ws.data_ptr() + off, nbytes.value

    def _device_lock(self, index):
        lk = self.dev_locks.get(index)
        if lk is None:
            with self.lock:
                lk = self.dev_locks.setdefault(index, threading.RLock())
        return lk

    def _enqueue(self, module, x0, kind, entry, outputs, keep=False, ws_key=None):
        """One forward entry `h, x, n, h, w, <outputs>, ws, ws_bytes, stream` on the current stream of x's device, with the
        workspace of `kind`.  outputs(h, n, hh, ww, new) allocates what the entry writes (new(dtype, *shape): an empty tensor
        on that device) and returns the entry's output arguments in order: tensors, None, plain numbers.  -> those outputs.
        ws_key: what the workspace kind's size query and cache key take in the place of `keep`."""
        x = self._check_input(module, x0)
        n, _, hh, ww = x.shape
        dev = x.device
        ts = torch.cuda.current_stream(dev)
        # calls on one handle are not re-entrant (include/esahrnet.h): threads that share a device enqueue one
        # after the other; threads on different devices (DataParallel's replicas) do not wait for each other
        with self._device_lock(dev.index):
            h = self._handle_for(module, dev)
            _lib.check(self.lib.esahrnet_set_debug_keep(h, 1 if keep else 0))
            ws, ws_ptr, ws_bytes = self._workspace(h, dev, ts, n, hh, ww, keep if ws_key is None else ws_key, kind=kind)
            outs = outputs(h, n, hh, ww, lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev))
            args = (h, x.data_ptr(), n, hh, ww, *[o.data_ptr() if isinstance(o, torch.Tensor) else o for o in outs], ws_ptr, ws_bytes,
                    C.c_void_p(ts.cuda_stream))
            fn = getattr(self.lib, entry)
            if torch.cuda.current_device() == dev.index:
                rc = fn(*args)
            else:
                with torch.cuda.device(dev):
                    rc = fn(*args)
            _lib.check(rc)
        ws.record_stream(ts)
        x.record_stream(ts)
        return outs

    def forward(self, module, x0, keep=False):
        k = module._k

        def outputs(h, n, hh, ww, new):
            # per-tile maxima beside the heat-maps (include/esahrnet.h: esahrnet_forward_partials): 8 bytes per plane
            # and 16x16 tile, so that inference.heatmaps_to_keypoints need not sweep the maps again
            nt = self._partial_tiles(h, hh, ww)
            return new(torch.float32, n, k, hh, ww), new(torch.float32, n * k, nt, 2) if nt else None

        heat, part = self._enqueue(module, x0, "forward", "esahrnet_forward_partials", outputs, keep)
        if part is not None:
            try:
                heat._esa_partials = (part, part.shape[1], heat._version)
            except RuntimeError:            # torch.inference_mode(): no version counter, so no way to tell a later edit
                pass
        return heat

    def forward_keypoints(self, module, x0, want_index):
        """esahrnet_forward_keypoints: (kp f32 [N,K,3], idx int32 [N,K] or None), no heat-map in caller memory.  Same device
        lock, workspace contract (graph capture included) and record_stream handling as forward()."""
        k = module._k
        return self._enqueue(module, x0, "keypoints", "esahrnet_forward_keypoints", lambda h, n, hh, ww, new: (
            new(torch.float32, n, k, 3), new(torch.int32, n, k) if want_index else None))

    def forward_final2(self, module, x0, want_index, want_hessian=False):
        """net(x, output="keypoints", refine="get_final2"): esahrnet_forward_keypoints_final2, the forward with get_final2 in
        place of its last launch; nothing but (kp, idx) — and the Hessians, if asked for — reaches caller memory."""
        k = module._k
        return self._enqueue(module, x0, "final2", "esahrnet_forward_keypoints_final2" + ("_hess" if want_hessian else ""),
                             lambda h, n, hh, ww, new: (new(torch.float32, n, k, 3), new(torch.int32, n, k) if want_index else None)
                             + ((new(torch.float64, n, k, 3),) if want_hessian else ()))

    def forward_gaussfit(self, module, x0, want_fit, want_index, want_hessian=True, cov=None):
        """esahrnet_forward_keypoints_gaussfit: -> (kp f32 [N,K,3], fit f64 [N,K,8] or None, status int32 [N,K], hess f64 [N,K,3]
        or None, idx int32 [N,K] or None); nothing else reaches caller memory.  cov = cov_floor (not None):
        esahrnet_forward_keypoints_gaussfit_cov, -> (..., cov f64 [N,K,3], info f64 [N,K,3]) appended."""
        k = module._k
        kp, idx, fit, status, hess, *more = self._enqueue(
            module, x0, "gaussfit", "esahrnet_forward_keypoints_gaussfit" + ("" if cov is None else "_cov"),
            lambda h, n, hh, ww, new: (new(torch.float32, n, k, 3), new(torch.int32, n, k) if want_index else None,
                                       new(torch.float64, n, k, 8) if want_fit else None, new(torch.int32, n, k),
                                       new(torch.float64, n, k, 3) if want_hessian else None)
            + (() if cov is None else (new(torch.float64, n, k, 3), new(torch.float64, n, k, 3), float(cov))))
        return (kp, fit, status, hess, idx, *more[:2])

    def forward_candidates(self, module, x0, candidates, nms_radius, want_index):
        """esahrnet_forward_keypoints_candidates: (cand f32 [N,K,M,3], cidx int32 [N,K,M] or None); the library refuses M outside
        1..4 and a negative radius with its own text (nothing is allocated by M before that)."""
        k = module._k
        mm = min(max(candidates, 1), _lib.MAX_CANDIDATES)
        _, _, cand, cidx = self._enqueue(module, x0, "candidates", "esahrnet_forward_keypoints_candidates",
                                         lambda h, n, hh, ww, new: (candidates, nms_radius, new(torch.float32, n, k, mm, 3),
                                                                    new(torch.int32, n, k, mm) if want_index else None))
        return cand, cidx

    def forward_candidates_refined(self, module, x0, candidates, nms_radius, want_index, decoder, want_hessian, want_fit, want_cov,
                                   cov_floor):
        """esahrnet_forward_keypoints_candidates_refined: (cand f32 [N,K,M,3], cidx int32 [N,K,M] or None, the optional outputs as
        inference._at_outputs names them: fit, status, hess, cov, info, each [N,K,M] + its own shape or None).  Without want_index
        the candidates' pixels stay in the workspace."""
        k = module._k
        mm = min(max(candidates, 1), _lib.MAX_CANDIDATES)

        def outputs(h, n, hh, ww, new):
            slot = lambda on, dt, *tail: new(dt, n, k, mm, *tail) if on else None          # noqa: E731
            return (candidates, nms_radius, decoder, new(torch.float32, n, k, mm, 3), slot(want_index, torch.int32),
                    slot(want_hessian, torch.float64, 3), slot(want_fit, torch.float64, 8), slot(decoder == 2, torch.int32),
                    slot(want_cov, torch.float64, 3), slot(want_cov, torch.float64, 3), float(cov_floor))

        _, _, _, cand, cidx, hess, fit, status, cov, info, _ = self._enqueue(
            module, x0, "candidates_refined", "esahrnet_forward_keypoints_candidates_refined", outputs, ws_key=("refined", decoder))
        return cand, cidx, {"fit": fit, "status": status, "hess": hess, "cov": cov, "info": info}

    # The loader's library entries.  form -> (entry, workspace kind, that workspace's cache key, the entry's arguments between the
    # loader's own and the workspace): a name is the pointer of that field of the result (None where no record has it), a callable
    # takes the request.  ("candidates" / "gaussfit" as a cache key only keep that workspace apart from the other loader kinds.)
    _PLACED = ("boxes", "rates", "valid")
    _SELECTED = ("count", "order", "pts", "w")
    _FITTED = ("kp", "idx", "fit", "status", "hess")
    _SELECT = (lambda q: q.select[0], lambda q: q.select[1], lambda q: q.mode)
    LOADER_ENTRIES = {
        "keypoints": ("esahrnet_frames_keypoints", lambda q: "frames_final2" if q.decoder else "frames", lambda q: bool(q.decoder),
                      (lambda q: q.decoder, "kp", "idx", *_PLACED)),
        "correspondences": ("esahrnet_frames_correspondences", lambda q: "corr", lambda q: (q.decoder, q.mode),
                            (lambda q: q.decoder, *_SELECT, "kp", "idx", *_PLACED, *_SELECTED)),
        "gaussfit": ("esahrnet_frames_keypoints_gaussfit", lambda q: "frames_gaussfit", lambda q: "gaussfit", (*_FITTED, *_PLACED)),
        "gaussfit_cov": ("esahrnet_frames_keypoints_gaussfit_cov", lambda q: "frames_gaussfit", lambda q: "gaussfit",
                         (*_FITTED, *_PLACED, "cov", "info", lambda q: q.cov_floor)),
        "candidates": ("esahrnet_frames_keypoints_candidates", lambda q: "frames_candidates", lambda q: "candidates",
                       (lambda q: q.candidates[0], lambda q: q.candidates[1], "cand", "cidx", *_PLACED)),
        "candidates_refined": ("esahrnet_frames_keypoints_candidates_refined", lambda q: "frames_candidates_refined",
                               lambda q: ("refined", q.decoder),
                               (lambda q: q.candidates[0], lambda q: q.candidates[1], lambda q: q.decoder, "cand", "cidx", "cand_hess",
                                "cand_fit", "cand_status", "cand_cov", "cand_info", lambda q: float(q.cov_floor or 0.0), *_PLACED)),
    }
    # the correspondence stage of the two-call forms, behind the main entry on the same stream, on its outputs: second record ->
    # (entry, its arguments behind the Hessian's pointer: m, k and M are the result's)
    SECOND_ENTRIES = {
        "correspondences": ("esahrnet_correspondences", "kp", (*_PLACED, "m", "k", *_SELECT, *_SELECTED)),
        "candidate_correspondences": ("esahrnet_correspondences_cand", "cand",
                                      (*_PLACED, "m", "k", "M", *_SELECT, "count", "order", "cpts", "cw", "cpeak")),
    }

    @staticmethod
    def _loader_form(q):
        if q.candidates is not None:
            return q.main[0]                                        # "candidates" / "candidates_refined"
        if q.refine == "gaussfit":                                  # its own entry points; the correspondences behind them
            return "gaussfit" if q.cov_floor is None else "gaussfit_cov"
        return "keypoints" if q.select is None else "correspondences"      # (one call does both for get_final / get_final2)

    def frames_keypoints(self, module, request, frames, det_boxes, frame_idx, m, scale, rule, fmt, mean, std):
        """The loader's library call for `request` (LOADER_ENTRIES; arguments already checked by crops.check_device_loader_args)
        and, for the Gaussian fit and the candidates with a select, the correspondence stage behind it (SECOND_ENTRIES), which
        takes the request's Hessian field, if any, where the entry takes a Hessian -> LoaderResult: the records of
        inference.record_fields, the library's outputs written straight into them.  Same device lock, weight-staleness key,
        workspace contract (graph capture included) and record_stream handling as forward()."""
        if module._cin != 1:
            raise ValueError(f"the loader makes 1-channel crops; this network takes {module._cin} channels")
        if "_master" not in module.__dict__:
            p = module._weight_tensors()[0]
            if p.device != frames.device:
                raise RuntimeError(f"frames on {frames.device} but parameters on {p.device}")
        frames = frames.contiguous()
        dev = frames.device
        nframes, fh, fw = frames.shape[:3]
        ts = torch.cuda.current_stream(dev)
        stream = C.c_void_p(ts.cuda_stream)
        form = self._loader_form(request)
        entry, ws_kind, ws_key, spec = self.LOADER_ENTRIES[form]
        with torch.cuda.device(dev):
            det = crops.to_device_int32(det_boxes, dev)
            fidx = None if frame_idx is None else crops.to_device_int32(frame_idx, dev)
            out = LoaderResult.empty(request, m, module._k, dev)
            p = {name: t.data_ptr() for name, t in out.views.items()}
            p.update(m=m, k=module._k, M=request.main[3])
            args = lambda names: [a(request) if callable(a) else p.get(a) for a in names]        # noqa: E731
            with self._device_lock(dev.index):
                h = self._handle_for(module, dev)
                _lib.check(self.lib.esahrnet_set_debug_keep(h, 0))
                ws, ws_ptr, ws_bytes = self._workspace(h, dev, ts, m, scale, scale, ws_key(request), kind=ws_kind(request))
                _lib.check(getattr(self.lib, entry)(
                    h, frames.data_ptr(), nframes, fh, fw, fmt, det.data_ptr(), None if fidx is None else fidx.data_ptr(), m, scale,
                    rule, mean, std, *args(spec), ws_ptr, ws_bytes, stream))
                if request.second is not None and form != "correspondences":
                    second, rows, spec2 = self.SECOND_ENTRIES[request.second]
                    _lib.check(getattr(self.lib, second)(p[rows], p.get(request.hessian), *args(spec2), stream))
        for t in (ws, frames, det, fidx):
            if t is not None:
                t.record_stream(ts)
        return out

    def _partial_tiles(self, h, hh, ww):
        if os.environ.get("ESAHRNET_NO_PARTIALS"):
            return 0
        key = (getattr(h, "value", h), hh, ww)
        nt = self.part_tiles.get(key)
        if nt is None:
            v = C.c_int(0)
            _lib.check(self.lib.esahrnet_partial_tiles(h, hh, ww, C.byref(v)))
            nt = self.part_tiles[key] = v.value
        return nt

    def forward_timed(self, module, x0):
        x = self._check_input(module, x0)
        n, _, hh, ww = x.shape
        dev = x.device
        h = self._handle_for(module, dev)
        _lib.check(self.lib.esahrnet_set_debug_keep(h, 0))
        ws, ws_ptr, ws_bytes = self._workspace(h, dev, torch.cuda.current_stream(dev), n, hh, ww, False)
        heat = torch.empty((n, module._k, hh, ww), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        nops = self.lib.esahrnet_launch_count(h)
        ms = (C.c_float * nops)()
        with torch.cuda.device(dev):
            _lib.check(self.lib.esahrnet_forward_timed(h, x.data_ptr(), n, hh, ww, heat.data_ptr(), ws_ptr,
                                                       ws_bytes, C.c_void_p(stream), ms))
        ops = []
        for i in range(nops):
            d = _lib.OpDesc()
            _lib.check(self.lib.esahrnet_op_desc_get(h, i, n, hh, ww, C.byref(d)))
            if not d.kernel:        # a plan alternative that this shape does not run (esahrnet.h: op_desc_get)
                continue
            ops.append(dict(kernel=d.kernel.decode(), label=d.label.decode(), ms=float(ms[i]),
                            flops=d.flops, bytes=d.bytes))
        return heat, ops

    def stats_rows(self, h, n, hh, ww):
        """The row descriptions of a handle's report at a shape (esahrnet_stats_row_get): no GPU needed."""
        rows = C.c_int(0)
        _lib.check(self.lib.esahrnet_stats_rows(h, C.byref(rows)))
        descs = []
        for i in range(rows.value):
            d = _lib.StatsRowDesc()
            _lib.check(self.lib.esahrnet_stats_row_get(h, i, n, hh, ww, C.byref(d)))
            descs.append(d)
        return descs

    def forward_stats(self, module, x0, with_h0=False):
        """esahrnet_forward_stats on the current stream of x's device: -> ActivationStats.  Same device lock, workspace contract
        and record_stream handling as forward(); the records come back in one copy.  with_h0: esahrnet_forward_stats_h0, the
        same rows plus ActivationStats.h0, one record per crop for the h0 of the fused head."""
        x = self._check_input(module, x0)
        n, _, hh, ww = x.shape
        dev = x.device
        ts = torch.cuda.current_stream(dev)
        with self._device_lock(dev.index):
            h = self._handle_for(module, dev)
            _lib.check(self.lib.esahrnet_set_debug_keep(h, 0))
            descs = self.stats_rows(h, n, hh, ww)
            ws, ws_ptr, ws_bytes = self._workspace(h, dev, ts, n, hh, ww, bool(with_h0), kind="stats_h0" if with_h0 else "stats")
            heat = torch.empty((n, module._k, hh, ww), dtype=torch.float32, device=dev)
            # (one buffer: the rows, then, with_h0, the h0 records behind them)
            stats = torch.empty((len(descs) + bool(with_h0), n, _lib.STATS_RECORD_BYTES), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                if with_h0:
                    _lib.check(self.lib.esahrnet_forward_stats_h0(h, x.data_ptr(), n, hh, ww, heat.data_ptr(), ws_ptr, ws_bytes,
                                                                  stats.data_ptr(), stats[len(descs)].data_ptr(),
                                                                  C.c_void_p(ts.cuda_stream)))
                else:
                    _lib.check(self.lib.esahrnet_forward_stats(h, x.data_ptr(), n, hh, ww, heat.data_ptr(), ws_ptr, ws_bytes,
                                                               stats.data_ptr(), C.c_void_p(ts.cuda_stream)))
            groups = []
            g = C.c_int(0)
            for i in range(len(descs)):
                _lib.check(self.lib.esahrnet_scale_row_group(h, i, C.byref(g)))
                groups.append(g.value)
        ws.record_stream(ts)
        x.record_stream(ts)
        rec = stats.cpu().numpy().reshape(-1).view(_lib.stats_dtype()).reshape(len(descs) + bool(with_h0), n)
        master = module.__dict__.get("_master", module)
        return ActivationStats(descs, rec[:len(descs)], heat, groups=groups, exponents=master.fp16_exponents,
                               h0=rec[len(descs)] if with_h0 else None)

    def diff_rows(self, h, href, n, hh, ww):
        """The rows of h's report paired with href's at a shape (esahrnet_diff_row_get): no GPU needed."""
        rows = C.c_int(0)
        _lib.check(self.lib.esahrnet_stats_rows(h, C.byref(rows)))
        descs = []
        for i in range(rows.value):
            d = _lib.DiffRowDesc()
            _lib.check(self.lib.esahrnet_diff_row_get(h, href, i, n, hh, ww, C.byref(d)))
            descs.append(d)
        return descs

    def forward_diff(self, module, ref_module, x0):
        """esahrnet_forward_diff on the current stream of x's device: -> PrecisionReport.  Same device lock (this runtime's, then
        the reference's), workspace contract and record_stream handling as forward_stats(); the records come back in one copy."""
        x = self._check_input(module, x0)
        ref_rt = ref_module._rt
        ref_rt._check_input(ref_module, x)
        n, _, hh, ww = x.shape
        dev = x.device
        ts = torch.cuda.current_stream(dev)
        with self._device_lock(dev.index), ref_rt._device_lock(dev.index):
            h = self._handle_for(module, dev)
            href = h if ref_module is module else ref_rt._handle_for(ref_module, dev)
            descs = self.diff_rows(h, href, n, hh, ww)
            ws, ws_ptr, ws_bytes = self._workspace(h, dev, ts, n, hh, ww, href.value, kind="diff")
            heat = torch.empty((n, module._k, hh, ww), dtype=torch.float32, device=dev)
            heat_ref = torch.empty_like(heat)
            rec_dev = torch.empty((len(descs), n, _lib.DIFF_RECORD_BYTES), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(self.lib.esahrnet_forward_diff(h, href, x.data_ptr(), n, hh, ww, heat.data_ptr(), heat_ref.data_ptr(),
                                                          ws_ptr, ws_bytes, rec_dev.data_ptr(), C.c_void_p(ts.cuda_stream)))
        ws.record_stream(ts)
        x.record_stream(ts)
        rec = rec_dev.cpu().numpy().reshape(-1).view(_lib.diff_dtype()).reshape(len(descs), n)
        return PrecisionReport(descs, rec, heat, heat_ref)

    def taps(self, module, x0):
        x = self._check_input(module, x0)
        n, _, hh, ww = x.shape
        dev = x.device
        heat = self.forward(module, x, keep=True)
        h = self.handles[dev.index][0]
        _, ws_ptr, _ = self._workspace(h, dev, torch.cuda.current_stream(dev), n, hh, ww, True)
        out = {"heatmaps": heat}
        stream = torch.cuda.current_stream(dev).cuda_stream
        buf = C.create_string_buffer(96)
        for i in range(self.lib.esahrnet_tap_count(h)):
            _lib.check(self.lib.esahrnet_tap_name(h, i, buf, 96))
            name = buf.value
            c, th, tw = C.c_int(), C.c_int(), C.c_int()
            _lib.check(self.lib.esahrnet_tap_shape(h, name, hh, ww, C.byref(c), C.byref(th), C.byref(tw)))
            t = torch.empty((n, c.value, th.value, tw.value), dtype=torch.float32, device=dev)
            if self.lib.esahrnet_tap_read(h, name, n, hh, ww, ws_ptr, t.data_ptr(), C.c_void_p(stream)) != 0:
                if b"head alternative" in self.lib.esahrnet_last_error():
                    continue                # tensor of the head variant this shape does not run
                _lib.check(1)
            out[name.decode()] = t
        _lib.check(self.lib.esahrnet_set_debug_keep(h, 0))
        return out


class ActivationStats:
    """net.activation_stats(x): per-tensor ranges of one forward.

    per_image   the raw records, a structured numpy array [rows, n] (_lib.STATS_FIELDS); rows not scanned are all zero
    rows        one dict per row in plan order, the last one "heatmaps": name, def_op, shape (c, h, w), format, scanned and
                the batch-combined figures (maxima and counts exactly, sum_abs added in crop order, mean_abs = sum_abs / n_finite)
                each row also carries `group`, its fp16 scale group (-1: none) and `exponent`, that group's exponent: the
                figures are those of the STORED values T * 2^-exponent, so the saturation counts keep their meaning
    heatmaps    the forward's heat-maps (f32 [n, K, H, W] on the device), the bits net(x) returns
    h0          with esahrnet_forward_stats_h0 only: the records [n] of the fused head's h0 (max_abs and n_ge_f16max before its
                rounding where the fused head ran, the stored row "head0" otherwise), else None"""

    F16_MAX = 65504.0
    COUNTS = tuple(name for name, t in _lib.STATS_FIELDS if t == "u4")

    def __init__(self, descs, per_image, heatmaps, groups=None, exponents=(), h0=None):
        self.descs = descs
        self.per_image = per_image
        self.heatmaps = heatmaps
        self.h0 = h0
        self.rows = []
        for i, (d, rec) in enumerate(zip(descs, per_image)):
            row = dict(name=d.name.decode(), def_op=d.def_op, shape=(d.c, d.h, d.w), format=_lib.STATS_FORMATS[d.fmt],
                       scanned=bool(d.scanned))
            row["group"] = groups[i] if groups is not None else -1
            row["exponent"] = int(exponents[row["group"]]) if row["group"] >= 0 and len(exponents) else 0
            row["max_abs"] = float(rec["max_abs"].max())
            row["min"] = float(rec["min"].min())
            row["max"] = float(rec["max"].max())
            sum_abs = 0.0
            for v in rec["sum_abs"]:
                sum_abs += float(v)
            row["sum_abs"] = sum_abs
            for name in self.COUNTS:
                row[name] = int(rec[name].astype(np.int64).sum())
            row["mean_abs"] = sum_abs / row["n_finite"] if row["n_finite"] else 0.0
            self.rows.append(row)

    def scanned(self):
        return [r for r in self.rows if r["scanned"]]

    def first_nonfinite(self):
        """Name of the first scanned row in plan order that holds a NaN or an infinity, or None."""
        for r in self.scanned():
            if r["n_nan"] + r["n_inf"] > 0:
                return r["name"]
        return None

    def headroom_fp16(self) -> float:
        """65504 / the largest finite |value| any stored tensor holds (the heat-maps row is caller memory, not a stored
        tensor): 1.0 in an fp16 net that saturates, below 1.0 in another format where fp16 would clamp."""
        top = max((r["max_abs"] for r in self.scanned()[:-1]), default=0.0)
        return self.F16_MAX / top if top > 0 else float("inf")

    def saturated(self):
        """The scanned rows with a finite |value| >= 65504: in an fp16 net the saturated stores (a genuine 65504 cannot be told
        apart from one), in the other formats the values fp16 would clamp."""
        return [r for r in self.scanned() if r["n_ge_f16max"] > 0]

    def table(self) -> str:
        head = f"{'row':>4} {'op':>4} {'name':<44} {'shape':<14} {'format':<8} {'max_abs':>11} {'mean_abs':>11} {'min':>11} " \
               f"{'max':>11} {'nan':>6} {'inf':>6} {'>=65504':>8} {'f16 tiny':>9} {'zero':>9}"
        lines = [head]
        for i, r in enumerate(self.rows):
            shape = "x".join(str(v) for v in r["shape"])
            if not r["scanned"]:
                lines.append(f"{i:>4} {r['def_op']:>4} {r['name'][:44]:<44} {shape:<14} {r['format']:<8} (not scanned)")
                continue
            lines.append(f"{i:>4} {r['def_op']:>4} {r['name'][:44]:<44} {shape:<14} {r['format']:<8} {r['max_abs']:>11.4e} "
                         f"{r['mean_abs']:>11.4e} {r['min']:>11.4e} {r['max']:>11.4e} {r['n_nan']:>6} {r['n_inf']:>6} "
                         f"{r['n_ge_f16max']:>8} {r['n_f16_tiny']:>9} {r['n_zero']:>9}")
        return "\n".join(lines)


class PrecisionReport:
    """net.precision_report(x): the error of one forward against the reference net's, tensor by tensor.

    per_image     the raw records, a structured numpy array [rows, n] (_lib.DIFF_FIELDS); rows not compared are all zero
    keys          one key per row of the tested net's report in plan order, the last one "heatmaps": what the tensor is (its
                  tap name, else the convolution whose output it is), the same in every plan of the configuration
    compared      bool [rows]: the key names one row in both plans, the shapes agree and both tensors were scanned
    descs         the row descriptions (_lib.DiffRowDesc): shape, formats, ref_row, exponent
    heatmaps, heatmaps_ref    the two forwards' heat-maps (f32 [n, K, H, W] on the device), the bits net(x) returns"""

    def __init__(self, descs, per_image, heatmaps, heatmaps_ref):
        self.descs = descs
        self.per_image = per_image
        self.heatmaps = heatmaps
        self.heatmaps_ref = heatmaps_ref
        self.keys = [d.key.decode() for d in descs]
        self.compared = np.array([bool(d.compared) for d in descs])

    def max_abs_err(self):
        """f32 [rows]: the largest |a - b| of each row over the crops (0 for a row not compared)."""
        return self.per_image["max_abs_err"].max(axis=1)

    def rel_max(self):
        """f64 [rows]: max_abs_err over the largest |b| of the row (0 where that is 0)."""
        ref = self.per_image["max_abs_ref"].max(axis=1).astype(np.float64)
        return np.divide(self.max_abs_err().astype(np.float64), ref, out=np.zeros_like(ref), where=ref > 0)

    def rel_rms(self):
        """f64 [rows]: sqrt(sum of err^2 / sum of b^2) over the compared elements of all crops (0 where the reference is 0)."""
        num = self.per_image["sum_sq_err"].sum(axis=1)
        den = self.per_image["sum_sq_ref"].sum(axis=1)
        return np.sqrt(np.divide(num, den, out=np.zeros_like(den), where=den > 0))

    def where(self, row: int, i: int):
        """(c, y, x) of the element record.at names in crop i of `row`; None when nothing was compared."""
        at = int(self.per_image["at"][row, i])
        if at == _lib.DIFF_AT_NONE:
            return None
        d = self.descs[row]
        if d.fmt == _lib.STATS_NCHW:
            return at // (d.h * d.w), at % (d.h * d.w) // d.w, at % d.w
        return at % d.c, at // d.c // d.w, at // d.c % d.w

    def worst(self, k: int = 5):
        """The k compared rows with the largest rel_max, largest first: dicts of row, key, shape, rel_max, rel_rms,
        max_abs_err, and the crop and (c, y, x) of that error."""
        rel, rms, err = self.rel_max(), self.rel_rms(), self.max_abs_err()
        order = sorted((r for r in range(len(self.keys)) if self.compared[r]), key=lambda r: -rel[r])[:k]
        out = []
        for r in order:
            i = int(self.per_image["max_abs_err"][r].argmax())
            d = self.descs[r]
            out.append(dict(row=r, key=self.keys[r], shape=(d.c, d.h, d.w), rel_max=float(rel[r]), rel_rms=float(rms[r]),
                            max_abs_err=float(err[r]), crop=i, where=self.where(r, i)))
        return out

    def keypoints(self, refine: str = "get_final"):
        """Both heat-map tensors through the device decoder (inference.heatmaps_to_keypoints): -> dict of max_shift and
        mean_shift (f64 [n]: the largest and the mean distance in pixels between a crop's keypoints and the reference's),
        argmax_differs (planes whose arg-max pixel differs), kp and kp_ref (f32 [n, K, 3] on the device)."""
        from .inference import _keypoints
        kp, idx = _keypoints(self.heatmaps, True, refine)[:2]
        kp_ref, idx_ref = _keypoints(self.heatmaps_ref, True, refine)[:2]
        shift = (kp[..., :2].double() - kp_ref[..., :2].double()).norm(dim=-1).cpu().numpy()
        return dict(max_shift=shift.max(axis=1), mean_shift=shift.mean(axis=1),
                    argmax_differs=int((idx != idx_ref).sum().item()), kp=kp, kp_ref=kp_ref)

    def table(self) -> str:
        rel, rms, err = self.rel_max(), self.rel_rms(), self.max_abs_err()
        head = f"{'row':>4} {'ref':>4} {'key':<44} {'shape':<14} {'format':<8} {'exp':>4} {'max_abs_err':>12} {'rel_max':>10} " \
               f"{'rel_rms':>10} {'max_abs_ref':>12} {'nonfin a':>9} {'nonfin b':>9} {'class !=':>9}"
        lines = [head]
        for r, d in enumerate(self.descs):
            shape = "x".join(str(v) for v in (d.c, d.h, d.w))
            fmt = _lib.STATS_FORMATS[d.fmt]
            if not self.compared[r]:
                lines.append(f"{r:>4} {d.ref_row:>4} {self.keys[r][:44]:<44} {shape:<14} {fmt:<8} (not compared)")
                continue
            rec = self.per_image[r]
            lines.append(f"{r:>4} {d.ref_row:>4} {self.keys[r][:44]:<44} {shape:<14} {fmt:<8} {d.exponent:>4} {err[r]:>12.4e} "
                         f"{rel[r]:>10.3e} {rms[r]:>10.3e} {rec['max_abs_ref'].max():>12.4e} "
                         f"{int(rec['n_nonfinite_test'].astype(np.int64).sum()):>9} "
                         f"{int(rec['n_nonfinite_ref'].astype(np.int64).sum()):>9} "
                         f"{int(rec['n_class_differs'].astype(np.int64).sum()):>9}")
        return "\n".join(lines)


class Fp16Calibration:
    """What net.calibrate_fp16 chose: exponents[g] for group names[g], and stored_max[g], the largest magnitude the verifying
    forward found stored in that group (true magnitude = stored_max[g] * 2^exponents[g])."""

    def __init__(self, exponents, names, stored_max, headroom_bits):
        self.exponents, self.names, self.stored_max, self.headroom_bits = exponents, names, stored_max, headroom_bits

    def as_dict(self):
        return {n: e for n, e in zip(self.names, self.exponents)}

    def table(self) -> str:
        lines = [f"{'group':<40} {'exponent':>8} {'stored max':>12} {'true max':>12}"]
        for n, e, m in zip(self.names, self.exponents, self.stored_max):
            lines.append(f"{n[:40]:<40} {e:>8d} {m:>12.4e} {m * 2.0 ** e:>12.4e}")
        return "\n".join(lines)


def get_seg_model(cfg, **kwargs):
    """models/seg_hrnet.py:495-499."""
    model = HighResolutionNet(cfg, **kwargs)
    pre = cfg.MODEL.PRETRAINED if hasattr(cfg, "MODEL") else cfg["MODEL"]["PRETRAINED"]
    model.init_weights(pre)
    return model
