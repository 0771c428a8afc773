"""CPU: the device loader (include/esahrnet.h: esahrnet_boxes, esahrnet_crops_ex, esahrnet_frames_keypoints and its workspace
query) is declared, bound and exported with the ABI number unchanged; crops.train_box is data_load4.py:112-141 (val_box with the
box forced square before the clamps); the argument checks of crop_batch_device / frames_to_keypoints and of the C entry points
answer before anything touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esahrnet_boxes", "esahrnet_crops_ex", "esahrnet_frames_keypoints_workspace_bytes", "esahrnet_frames_keypoints")


def test_header_declares_the_entries_and_keeps_the_abi():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esahrnet.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6


def test_lib_binds_and_exports_the_entries():
    from esa_pose_estimation_amd import _lib as L
    assert L.ABI_VERSION == 6
    assert set(ENTRIES) <= set(L.exported_symbols())
    lib = L.lib()
    assert lib.esahrnet_abi_version() == 6
    for name in ENTRIES:
        assert getattr(lib, name).argtypes is not None, name
    raw = C.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
    assert len(lib.esahrnet_frames_keypoints.argtypes) == 22 and len(lib.esahrnet_crops_ex.argtypes) == 14


def test_frontend_is_built_without_contraction():
    """frontend.hip is a source of the library and the only file compiled with -ffp-contract=off."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "frontend.hip" in b.SOURCES and "crops.hip" in b.SOURCES
    assert "-ffp-contract=off" in b.PER_FILE_FLAGS["frontend.hip"]
    assert [f for f, fl in b.PER_FILE_FLAGS.items() if "-ffp-contract=off" in fl] == ["frontend.hip"]


# ---- the box rules -------------------------------------------------------------------------------------------------------
def _pre_clamp(b, k=1.05):
    """data_load_val.py:127-135 = data_load4.py:112-119: the box around the centre, before any clamp."""
    x, y, w, h = b
    c0, c1 = int((x + w) / 2), int((y + h) / 2)
    size = int(max(w - x, h - y) / 2)
    return int(c0 - k * size), int(c1 - k * size), int(c0 + k * size), int(c1 + k * size)


def _clamps(x_new, y_new, w_new, h_new, img_w=1920, img_h=1200):
    """data_load_val.py:137-158 = data_load4.py:123-140: shift the box back inside the frame."""
    if x_new < 0:
        w_new, x_new = w_new - x_new, 0
    if y_new < 0:
        h_new, y_new = h_new - y_new, 0
    if w_new > img_w:
        x_new, w_new = max(x_new + img_w - w_new, 0), img_w
    if h_new > img_h:
        y_new, h_new = max(y_new + img_h - h_new, 0), img_h
    return [x_new, y_new, w_new, h_new]


def sweep_boxes():
    """Deterministic detector boxes: centres on a grid that reaches past all four borders (so every single clamp and both
    double clamps occur), odd and even sizes, wide and tall."""
    out = []
    for cx in (-40, 3, 10, 57, 400, 960, 1500, 1873, 1917, 1960):
        for cy in (-25, 2, 11, 64, 333, 600, 900, 1151, 1198, 1230):
            for hw, hh in ((30, 30), (101, 77), (77, 101), (202, 150), (333, 334), (611, 480), (950, 1000)):
                out.append((cx - hw, cy - hh, cx + hw + (cx & 1), cy + hh + (cy & 1)))
    return out


def test_train_box_hand_cases():
    from esa_pose_estimation_amd import crops
    # centre (10, 500), half size 101: 1.05 * 101 = 106.05; int() truncates toward zero, so the column span is
    # int(-96.05) .. int(116.05) = -96 .. 116 (212 wide) but the row span int(393.95) .. int(606.05) = 393 .. 606 (213 tall)
    b = (-91, 400, 111, 600)
    assert _pre_clamp(b) == (-96, 393, 116, 606)
    assert crops.val_box(b) == ([0, 393, 212, 606], 213)
    assert crops.train_box(b) == ([0, 393, 212, 605], 212)          # data_load4.py:120-121: h_new = y_new + (w_new - x_new)
    # a box in the interior: both spans truncate the same way, the rules agree
    b = (700, 400, 1100, 760)
    assert crops.val_box(b) == crops.train_box(b) == ([690, 370, 1110, 790], 420)
    # top border, centre (960, 10), half size 101: rows -96 .. 116 (212), columns 853 .. 1066 (213): the rule replaces h_new by
    # y_new + 213 = 117 before the clamp moves the box down by 96
    b = (859, -91, 1061, 111)
    assert _pre_clamp(b) == (853, -96, 1066, 116)
    assert crops.val_box(b) == ([853, 0, 1066, 212], 213)
    assert crops.train_box(b) == ([853, 0, 1066, 213], 213)
    assert crops.MEAN_TRAIN == 0.449 and crops.MEAN_VAL == 0.485


def test_train_box_is_val_box_with_the_forced_square():
    from esa_pose_estimation_amd import crops
    boxes = sweep_boxes()
    square = differ = 0
    hit = dict(left=0, top=0, right=0, bottom=0, left_top=0, right_bottom=0)
    for b in boxes:
        x_new, y_new, w_new, h_new = _pre_clamp(b)
        hit["left"] += x_new < 0
        hit["top"] += y_new < 0
        hit["right"] += w_new > 1920
        hit["bottom"] += h_new > 1200
        hit["left_top"] += x_new < 0 and y_new < 0
        hit["right_bottom"] += w_new > 1920 and h_new > 1200
        vbox, vsize = crops.val_box(b)
        assert vbox == _clamps(x_new, y_new, w_new, h_new) and vsize == max(vbox[2] - vbox[0], vbox[3] - vbox[1])
        if (w_new - x_new) == (h_new - y_new):
            square += 1
            assert crops.train_box(b) == (vbox, vsize), b
        else:
            differ += 1
            exp = _clamps(x_new, y_new, w_new, y_new + (w_new - x_new))
            assert crops.train_box(b) == (exp, max(exp[2] - exp[0], exp[3] - exp[1])), b
    assert square > 100 and differ > 20 and all(v > 0 for v in hit.values()), (square, differ, hit)


# ---- argument errors, before any GPU call --------------------------------------------------------------------------------
def test_python_argument_errors_without_a_gpu():
    from esa_pose_estimation_amd import config, crops, seg_hrnet, seg_hrnet2
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64)))
    gray = torch.zeros((2, 32, 48), dtype=torch.uint8)
    boxes = [(0, 0, 10, 10), (4, 4, 20, 20)]
    calls = [lambda *a, **k: crops.crop_batch_device(*a, **k), lambda *a, **k: net.frames_to_keypoints(*a, **k)]
    for call in calls:
        with pytest.raises(TypeError, match="no CPU"):                       # a CPU tensor
            call(gray, boxes)
        with pytest.raises(TypeError, match="uint8"):                        # wrong dtype
            call(gray.float(), boxes)
        with pytest.raises(TypeError, match="int32"):
            call(gray, torch.zeros((2, 4), dtype=torch.int64))
        with pytest.raises(ValueError, match="frame ind"):                   # frame_idx length mismatch
            call(gray, boxes, frame_idx=[0, 1, 1])
        with pytest.raises(ValueError, match="pass frame_idx"):
            call(gray, boxes + boxes)
        with pytest.raises(ValueError, match="rule"):
            call(gray, boxes, rule="test")
        with pytest.raises(ValueError, match="crop_batch"):                  # non-integral boxes belong to crop_batch
            call(gray, [(0.5, 0, 10, 10), (4, 4, 20, 20)])
        with pytest.raises(ValueError, match="pixel_format"):
            call(torch.zeros((2, 32, 48, 4), dtype=torch.uint8), boxes)
    with pytest.raises(ValueError, match="refine"):
        net.frames_to_keypoints(gray, boxes, refine="get_final3")
    net.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        net.frames_to_keypoints(gray, boxes)
    assert crops.check_device_loader_args.__doc__ and np.asarray(boxes).shape == (2, 4)
    assert hasattr(seg_hrnet.get_seg_model(config.make_config(widths=(8, 16, 32, 64))), "frames_to_keypoints")


def test_c_argument_errors_before_anything_is_enqueued():
    from esa_pose_estimation_amd import _lib as L, config, hrnet
    lib = L.lib()

    def handle(cin, k):
        cfg = hrnet._cfg_struct(config.make_config(widths=(16, 32, 64, 128)), cin, k, 0, "fp32")
        h = C.c_void_p()
        L.check(lib.esahrnet_create(C.byref(cfg), 0, C.byref(h)))
        return h

    h, h3 = handle(1, 11), handle(3, 32)
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    p = C.c_void_p(p.value + (-p.value) % 256)
    nb = C.c_size_t()
    err = lib.esahrnet_last_error
    try:
        # the workspace query: the decoder's own query plus the 256-byte-aligned crop tensor
        for dec, q in ((0, lib.esahrnet_keypoints_workspace_bytes), (1, lib.esahrnet_keypoints_final2_forward_workspace_bytes)):
            for m, s in ((1, 256), (32, 256), (3, 90)):
                base = C.c_size_t()
                L.check(q(h, m, s, s, C.byref(base)))
                L.check(lib.esahrnet_frames_keypoints_workspace_bytes(h, m, s, dec, C.byref(nb)))
                assert nb.value == base.value + ((m * s * s * 4 + 255) & ~255)
        assert lib.esahrnet_frames_keypoints_workspace_bytes(h, 1, 256, 2, C.byref(nb)) != 0 and b"decoder" in err()
        assert lib.esahrnet_frames_keypoints_workspace_bytes(h, 0, 256, 0, C.byref(nb)) != 0
        assert lib.esahrnet_frames_keypoints_workspace_bytes(h, 1, 256, 0, None) != 0 and b"null" in err()
        assert lib.esahrnet_frames_keypoints_workspace_bytes(h3, 1, 256, 0, C.byref(nb)) != 0 and b"1-channel" in err()

        def boxes(m=1, fh=1200, fw=1920, scale=256, rule=0, det=p, out=p):
            return lib.esahrnet_boxes(det, m, fh, fw, scale, rule, out, p, p, None)
        assert boxes(m=0) != 0 and b"boxes" in err()
        assert boxes(rule=2) != 0 and b"rule" in err()
        assert boxes(scale=0) != 0 and boxes(fh=0) != 0
        assert boxes(det=None) != 0 and b"null" in err()
        assert boxes(out=None) != 0 and b"null" in err()

        def crops_ex(nframes=1, fmt=0, fidx=None, m=1, scale=256, std=0.229, frames=p):
            return lib.esahrnet_crops_ex(frames, nframes, 1200, 1920, fmt, fidx, p, None, m, scale, 0.485, std, p, None)
        assert crops_ex(fmt=2) != 0 and b"pixel_format" in err()
        assert crops_ex(std=0.0) != 0 and b"stdv" in err()
        assert crops_ex(m=0) != 0 and crops_ex(nframes=0) != 0
        assert crops_ex(frames=None) != 0 and b"null" in err()
        assert crops_ex(nframes=1, m=2) != 0 and b"frame index" in err()

        def fk(hh=h, m=1, nframes=1, fmt=0, rule=0, dec=0, std=0.229, kp=p, ws=p, wsb=4096, fidx=None):
            return lib.esahrnet_frames_keypoints(hh, p, nframes, 1200, 1920, fmt, p, fidx, m, 256, rule, 0.485, std, dec, kp, None,
                                                 p, p, p, ws, wsb, None)
        assert fk(m=0) != 0 and fk(m=-1) != 0
        assert fk(rule=3) != 0 and b"rule" in err()
        assert fk(fmt=5) != 0 and b"pixel_format" in err()
        assert fk(std=-1.0) != 0 and b"stdv" in err()
        assert fk(kp=None) != 0 and b"null" in err()
        assert fk(ws=None) != 0 and b"null" in err()
        assert fk(hh=None) != 0 and b"null" in err()
        assert fk(m=2) != 0 and b"frame index" in err()
        assert fk() != 0 and b"commit" in err()                 # a handle without weights: refused before any launch
        assert fk(dec=2) != 0
    finally:
        lib.esahrnet_destroy(h)
        lib.esahrnet_destroy(h3)
