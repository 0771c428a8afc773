"""Loader contract in front of the path (SURVEY.md §8f NEXT-2): bbox -> clamped crop box -> GPU crop.

Reference being mirrored: ESAValDataSet.__getitem__ (data_load_val.py:103-195): the detector box
(x, y, x2, y2) is squared around its centre, scaled by 1.05, shifted back inside the 1920x1200 frame,
the crop is edge-padded, resized to `scale`, divided by 255 and normalised with mean 0.485 / std 0.229;
the caller later needs `bbox` (crop origin) and `rate` (= scale / size) to map keypoints back
(val.py:180).  `val_box` is the integer box arithmetic (host, a few ints per image); the pixel work runs
in crops.hip on the frames already resident on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

IMG_W, IMG_H = 1920, 1200            # data_load_val.py:77-78
MEAN_VAL, STD = 0.485, 0.229         # data_load_val.py:86  (the TRAIN loaders use 0.449: data_load4.py:81)
MEAN_TRAIN = 0.449                   # data_load4.py:81-87 (ESADataSet: training, and demo.py's scored evaluation)
RULES = {"val": 0, "train": 1}       # esahrnet_boxes' rule: val_box / train_box
PIXEL_FORMATS = {"gray": 0, "rgb": 1}


def val_box(bbox, img_w: int = IMG_W, img_h: int = IMG_H, k: float = 1.05):
    """data_load_val.py:127-158 -> ([x_new, y_new, w_new, h_new], size); (w_new, h_new) are the far corner."""
    x, y, w, h = bbox
    c0 = int((x + w) / 2)
    c1 = int((y + h) / 2)
    size = int(max((w - x), (h - y)) / 2)
    x_new, y_new = int(c0 - k * size), int(c1 - k * size)
    w_new, h_new = int(c0 + k * size), int(c1 + k * size)
    if x_new < 0:
        w_new -= x_new
        x_new = 0
    if y_new < 0:
        h_new -= y_new
        y_new = 0
    if w_new > img_w:
        x_new = x_new + img_w - w_new
        if x_new < 0:
            x_new = 0
        w_new = img_w
    if h_new > img_h:
        y_new = y_new + img_h - h_new
        if y_new < 0:
            y_new = 0
        h_new = img_h
    return [x_new, y_new, w_new, h_new], max(w_new - x_new, h_new - y_new)


def train_box(bbox, img_w: int = IMG_W, img_h: int = IMG_H, k: float = 1.05):
    """data_load4.py:112-141 (ESADataSet, which demo.py evaluates through): val_box with the far corner's row moved so
    that the box is square BEFORE it is shifted back inside the frame -> ([x_new, y_new, w_new, h_new], size)."""
    x, y, w, h = bbox
    c0 = int((x + w) / 2)
    c1 = int((y + h) / 2)
    size = int(max((w - x), (h - y)) / 2)
    x_new, y_new = int(c0 - k * size), int(c1 - k * size)
    w_new, h_new = int(c0 + k * size), int(c1 + k * size)
    if (w_new - x_new) != (h_new - y_new):
        h_new = y_new + (w_new - x_new)
    if x_new < 0:
        w_new -= x_new
        x_new = 0
    if y_new < 0:
        h_new -= y_new
        y_new = 0
    if w_new > img_w:
        x_new = max(x_new + img_w - w_new, 0)
        w_new = img_w
    if h_new > img_h:
        y_new = max(y_new + img_h - h_new, 0)
        h_new = img_h
    return [x_new, y_new, w_new, h_new], max(w_new - x_new, h_new - y_new)


def crop_batch(frames: torch.Tensor, bboxes, scale: int = 256, mean: float = MEAN_VAL, std: float = STD):
    """frames: uint8 cuda [N, H, W] (gray camera frames); bboxes: N detector boxes (x, y, x2, y2).
    -> (crops f32 cuda [N,1,scale,scale], boxes [N][4] ints, rates [N]) — image, bbox, rate of
    data_load_val.py:195."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 3):
        raise TypeError("frames must be a uint8 CUDA tensor [N, H, W] (no CPU fallback)")
    frames = frames.contiguous()
    n, fh, fw = frames.shape
    if len(bboxes) != n:
        raise ValueError(f"{len(bboxes)} detector boxes for {n} frames (crop_kernel reads one box per frame)")
    boxes, rates = [], []
    for b in bboxes:
        box, size = val_box(b, fw, fh)
        if box[2] <= box[0] or box[3] <= box[1]:
            raise ValueError(f"empty crop box {box} from detector box {list(b)}")
        boxes.append(box)
        rates.append(1.0 if size == scale else scale / size)
    bt = torch.tensor(boxes, dtype=torch.int32, device=frames.device)
    out = torch.empty((n, 1, scale, scale), dtype=torch.float32, device=frames.device)
    stream = torch.cuda.current_stream(frames.device).cuda_stream
    with torch.cuda.device(frames.device):
        _lib.check(_lib.lib().esahrnet_crops(frames.data_ptr(), n, fh, fw, bt.data_ptr(), scale, mean, std,
                                             out.data_ptr(), C.c_void_p(stream)))
    return out, boxes, rates


def check_device_loader_args(frames, det_boxes, frame_idx, rule, pixel_format):
    """Argument checks of the device loader, all of them before anything touches a GPU.
    -> (rule number, pixel format number, number of boxes)."""
    if rule not in RULES:
        raise ValueError(f"rule={rule!r}: expected one of {sorted(RULES)} (val_box / train_box)")
    if isinstance(det_boxes, torch.Tensor):
        if det_boxes.dtype != torch.int32 or det_boxes.dim() != 2 or det_boxes.shape[1] != 4:
            raise TypeError(f"det_boxes must be int32 [m, 4] (x, y, x2, y2), got {det_boxes.dtype} {tuple(det_boxes.shape)}")
        m = det_boxes.shape[0]
    else:
        a = np.asarray(det_boxes)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError(f"det_boxes must be m boxes (x, y, x2, y2), got shape {a.shape}")
        if a.dtype.kind not in "iuf" or (a.dtype.kind == "f" and not np.all(a == np.trunc(a))) or \
                np.any(np.abs(a.astype(np.float64)) > 2 ** 31 - 1):
            raise ValueError("the device loader takes integer detector boxes (int32); crop_batch takes any Python numbers")
        m = a.shape[0]
    if m == 0:
        raise ValueError("no detector boxes")
    if frame_idx is not None:
        if isinstance(frame_idx, torch.Tensor) and (frame_idx.dtype != torch.int32 or frame_idx.dim() != 1):
            raise TypeError(f"frame_idx must be int32 [m], got {frame_idx.dtype} {tuple(frame_idx.shape)}")
        if len(frame_idx) != m:
            raise ValueError(f"{len(frame_idx)} frame indices for {m} detector boxes")
    if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() in (3, 4)):
        raise TypeError("frames must be a uint8 CUDA tensor [N, H, W] (gray) or [N, H, W, 3] (RGB)")
    if pixel_format is None:
        pixel_format = "rgb" if frames.dim() == 4 else "gray"
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError(f"pixel_format={pixel_format!r}: expected one of {sorted(PIXEL_FORMATS)}")
    if (frames.dim() == 4) != (pixel_format == "rgb") or (frames.dim() == 4 and frames.shape[3] != 3):
        raise ValueError(f"pixel_format={pixel_format!r} does not fit frames of shape {tuple(frames.shape)}")
    if frame_idx is None and m != frames.shape[0]:
        raise ValueError(f"{m} detector boxes for {frames.shape[0]} frames: pass frame_idx (box i lies on frame frame_idx[i])")
    if not frames.is_cuda:
        raise TypeError("frames must be a uint8 CUDA tensor: the device loader has no CPU fallback")
    for name, t in (("det_boxes", det_boxes), ("frame_idx", frame_idx)):
        if isinstance(t, torch.Tensor) and t.device != frames.device:
            raise TypeError(f"{name} is on {t.device}, the frames on {frames.device}")
    return RULES[rule], PIXEL_FORMATS[pixel_format], m


def to_device_int32(seq, device):
    """A host sequence of integers -> int32 tensor on `device`, uploaded once from pinned memory without blocking; a CUDA
    tensor is used as it is."""
    if isinstance(seq, torch.Tensor):
        return seq.contiguous()
    host = torch.from_numpy(np.ascontiguousarray(np.asarray(seq).astype(np.int32)))
    return host.pin_memory().to(device, non_blocking=True)


def crop_batch_device(frames: torch.Tensor, det_boxes, frame_idx=None, scale: int = 256, rule: str = "val",
                      pixel_format=None, mean: float = MEAN_VAL, std: float = STD):
    """crop_batch without the host: frames uint8 cuda [N,H,W] (gray) or [N,H,W,3] (RGB, reduced as PIL's convert('L'));
    det_boxes m detector boxes (x, y, x2, y2), int32 cuda [m,4] or a host sequence of integers; frame_idx (int32 [m], None:
    box i lies on frame i): several boxes may share a frame; rule "val" (val_box) or "train" (train_box).
    -> (crops f32 [m,1,scale,scale], crop_boxes int32 [m,4], rates f64 [m], valid bool-like int32 [m]), all on the device,
    nothing synchronises.  An empty crop box or a frame index out of range cannot raise here: the crop is zeros and
    valid[i] == 0 (include/esahrnet.h: esahrnet_boxes, esahrnet_crops_ex)."""
    rule_n, fmt, m = check_device_loader_args(frames, det_boxes, frame_idx, rule, pixel_format)
    frames = frames.contiguous()
    dev = frames.device
    nframes, fh, fw = frames.shape[:3]
    with torch.cuda.device(dev):
        det = to_device_int32(det_boxes, dev)
        fidx = None if frame_idx is None else to_device_int32(frame_idx, dev)
        boxes = torch.empty((m, 4), dtype=torch.int32, device=dev)
        rates = torch.empty((m,), dtype=torch.float64, device=dev)
        valid = torch.empty((m,), dtype=torch.int32, device=dev)
        out = torch.empty((m, 1, scale, scale), dtype=torch.float32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        lib = _lib.lib()
        _lib.check(lib.esahrnet_boxes(det.data_ptr(), m, fh, fw, scale, rule_n, boxes.data_ptr(), rates.data_ptr(),
                                      valid.data_ptr(), stream))
        if fidx is not None:                # esahrnet_boxes does not see the frames: fold the index check into `valid`
            valid = valid * ((fidx >= 0) & (fidx < nframes)).to(torch.int32)
        _lib.check(lib.esahrnet_crops_ex(frames.data_ptr(), nframes, fh, fw, fmt, None if fidx is None else fidx.data_ptr(),
                                         boxes.data_ptr(), valid.data_ptr(), m, scale, mean, std, out.data_ptr(), stream))
    return out, boxes, rates, valid
