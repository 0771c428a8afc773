"""References and the case table of the crop stage (crop_kernel of csrc/crops.hip, crop_ex_kernel<0|1> of csrc/frontend.hip),
for tests/test_crops_ref_host.py (what holds them) and tests/test_gpu_crops.py (the kernels).  No GPU, no package import.

exact()      the loader's rule written from the loader, not from the kernel: slice the box, np.pad(image, ((0, size - xs),
             (0, size - ys)), 'edge') (the reference's swapped amounts), then float64 bilinear interpolation with half-pixel
             centres and no antialiasing (torch.nn.functional.interpolate, align_corners=False, on a float64 CPU tensor: low end
             clamped to source index 0, upper neighbour clamped to src - 1).  Real values in [0, 255].
bilinear()   the same interpolation in numpy with a coordinate `shift`; shift 0 equals exact()'s (test_crops_ref_host.py), a
             shift of 0.5 is the geometry without half-pixel centres.
luma()       PIL's convert('L') as include/esahrnet.h states it;  normalise() / recover_u8()  the f32 normalisation and back.
B            the bound on |8-bit fixed-point resize - exact| in gray levels, derived in test_crops_ref_host.py's docstring.
CASES        single-crop rows (class, name, frame, box, S, mean, std); BATCHES launches of several crops; NOT_SERVED crops that
             esahrnet_crops_ex must write as zeros.  Frames are uniform random u8 (the worst case for interpolation error), made
             once and read-only.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
MEAN, STD = 0.485, 0.229
NORMALISATIONS = ((0.485, 0.229), (0.449, 0.229), (0.0, 1.0))

# final rounding + two `>> 16` truncations of a quarter level each + the `>> 4` truncation (1/128 level, weights summing to 1)
# + per pass 255 x (coefficient quantisation 2^-12 + float32 rounding of the source coordinate 2^-13): 1.19458
B = 0.5 + 2 * 0.25 + 2.0 ** -7 + 2 * 255 * (2.0 ** -12 + 2.0 ** -13)


# ---- references -------------------------------------------------------------------------------------------------------------
def padded(frame_u8, box, swapped=True):
    """The loader's source image of a crop box (x0, y0, x1, y1): the slice, edge-padded by the reference's amounts (rows by
    the width deficit, columns by the height deficit); swapped=False: rows by the height deficit, the square the call meant."""
    x0, y0, x1, y1 = box
    image = frame_u8[y0:y1, x0:x1]
    xs, ys = x1 - x0, y1 - y0
    size = max(xs, ys)
    if xs != size or ys != size:
        image = np.pad(image, ((0, size - xs), (0, size - ys)) if swapped else ((0, size - ys), (0, size - xs)), 'edge')
    return image


def exact(frame_u8, box, S, swapped=True):
    image = np.ascontiguousarray(padded(frame_u8, box, swapped)).astype(np.float64)
    assert image.ndim == 2 and image.size > 0
    out = F.interpolate(torch.from_numpy(image)[None, None], size=(S, S), mode="bilinear", align_corners=False)
    return out[0, 0].numpy()


def _axis(dst, src, shift):
    c = (np.arange(dst, dtype=np.float64) + 0.5) * (src / dst) - 0.5 + shift
    c = np.clip(c, 0.0, src - 1.0)
    i0 = np.minimum(np.floor(c).astype(np.int64), src - 1)
    return i0, np.minimum(i0 + 1, src - 1), c - i0


def bilinear(image, dst_h, dst_w, shift=0.0):
    """float64 bilinear interpolation, source coordinate (d + 0.5) * src / dst - 0.5 + shift, clamped to [0, src - 1]."""
    im = image.astype(np.float64)
    y0, y1, v = _axis(dst_h, im.shape[0], shift)
    x0, x1, u = _axis(dst_w, im.shape[1], shift)
    rows = im[:, x0] * (1.0 - u) + im[:, x1] * u
    return rows[y0] * (1.0 - v)[:, None] + rows[y1] * v[:, None]


def luma(rgb):
    """PIL's convert('L'): L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 (include/esahrnet.h: esahrnet_crops_ex)."""
    c = rgb.astype(np.int64)
    return ((c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def normalise(u8, mean=MEAN, std=STD):
    return ((u8.astype(np.float32) / np.float32(255)) - np.float32(mean)) / np.float32(std)


def _recover(out, mean, std):
    return np.rint((out.astype(np.float64) * float(np.float32(std)) + float(np.float32(mean))) * 255.0)


@functools.lru_cache(maxsize=None)
def _round_trip_checked(mean, std):
    all256 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(_recover(normalise(all256, mean, std), mean, std), all256), (mean, std)
    return True


def recover_u8(out, mean=MEAN, std=STD):
    """The gray level (float64, integral) a normalised f32 value stands for; exact for every level under (mean, std)."""
    assert _round_trip_checked(float(mean), float(std))
    return _recover(out, mean, std)


# ---- frames -----------------------------------------------------------------------------------------------------------------
# name -> (shape, seed).  A, B: odd FH != FW, both ways round; W: the wide frame of the deep-downscale rows; X: the workload's
# frame; R: every one of the 256 levels once; A3: three frames of distinct content; C3: three RGB frames, independent channels.
FRAMES = {"A": ((151, 197), 101), "B": ((173, 131), 102), "W": ((41, 1100), 103), "X": ((1200, 1920), 104), "R": ((16, 16), 105),
          "A3": ((3, 151, 197), 106), "C3": ((3, 131, 173, 3), 107)}


@functools.lru_cache(maxsize=None)
def frame(name):
    shape, seed = FRAMES[name]
    rng = np.random.default_rng(seed)
    a = rng.permutation(256).astype(np.uint8).reshape(shape) if name == "R" else rng.integers(0, 256, size=shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


def frame_hw(name):
    shape = FRAMES[name][0]
    return shape[-3:-1] if name == "C3" else shape[-2:]


# ---- single-crop rows -------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "cls name frame box S mean std")
CLASSES = ("ratio", "blocks", "nonsquare", "position", "workload", "normalisation")


def _case(cls, name, frm, box, S, mean=MEAN, std=STD):
    return Case(cls, f"{cls}-{name}", frm, tuple(box), S, mean, std)


def _sq(x, y, k):
    return (x, y, x + k, y + k)


def _cases():
    rows = []
    # ratio: source side 1, 2, 3, S-1, S (identity), S+1, 2S (the four-pixel mean) and a non-integer downscale >= 4x, square
    # boxes (both axes at once); the wide frame's rows reach a 270x downscale and source coordinates past 2048
    for k in (1, 2, 3, 31, 32, 33, 64, 137):
        rows.append(_case("ratio", f"A-side{k}-S32", "A", _sq(10, 7, k), 32))
    for k in (1, 2, 3, 7, 8, 9, 16, 35):
        rows.append(_case("ratio", f"B-side{k}-S8", "B", _sq(61, 90, k), 8))
    rows.append(_case("ratio", "W-deep-S8", "W", (0, 0, 1100, 41), 8))
    rows.append(_case("ratio", "W-deep-S64", "W", (3, 1, 1098, 40), 64))
    # column blocks of crop_ex_kernel (256 columns a block): one block, one block full, one lane in the second, the workload's
    # 384, three blocks with one lane in the last; sources about 40 wide
    for S in (8, 64, 255, 256, 257, 384, 513):
        rows.append(_case("blocks", f"B-40-S{S}", "B", (30, 50, 70, 90), S))
    rows.append(_case("blocks", "A-41x40-S257", "A", (100, 60, 141, 100), 257))
    # non-square, both ways, and 1-pixel boxes
    for S in (32, 257):
        rows.append(_case("nonsquare", f"A-40x25-S{S}", "A", (25, 30, 65, 55), S))
        rows.append(_case("nonsquare", f"A-25x40-S{S}", "A", (25, 30, 50, 70), S))
    rows.append(_case("nonsquare", "A-1x30-S32", "A", (60, 20, 61, 50), 32))
    rows.append(_case("nonsquare", "A-30x1-S32", "A", (20, 60, 50, 61), 32))
    rows.append(_case("nonsquare", "B-40x25-S16", "B", (13, 101, 53, 126), 16))
    rows.append(_case("nonsquare", "B-25x40-S16", "B", (90, 17, 115, 57), 16))
    # position: each edge, each corner, the whole frame, the interior
    for frm in ("A", "B"):
        fh, fw = frame_hw(frm)
        k, mx, my = 37, (fw - 37) // 2, (fh - 37) // 2
        for name, (x, y) in (("left", (0, my)), ("right", (fw - k, my)), ("top", (mx, 0)), ("bottom", (mx, fh - k)),
                             ("topleft", (0, 0)), ("topright", (fw - k, 0)), ("bottomleft", (0, fh - k)),
                             ("bottomright", (fw - k, fh - k)), ("interior", (mx - 9, my + 5))):
            rows.append(_case("position", f"{frm}-{name}-S16", frm, _sq(x, y, k), 16))
        rows.append(_case("position", f"{frm}-whole-S16", frm, (0, 0, fw, fh), 16))
    # the workload: the full 1920x1200 frame at scale 256 (test_crops_pipeline.BOXES[3] after val_box)
    rows.append(_case("workload", "X-whole-S256", "X", (0, 0, 1920, 1200), 256))
    # normalisation: every level, identity resize
    for mean, std in NORMALISATIONS:
        rows.append(_case("normalisation", f"R-mean{mean}-std{std}", "R", (0, 0, 16, 16), 16, mean, std))
    return tuple(rows)


CASES = _cases()


def source_shape(box):
    """(rows, cols) of the padded source."""
    xs, ys = box[2] - box[0], box[3] - box[1]
    size = max(xs, ys)
    return ys + (size - xs), xs + (size - ys)


def replicated_edge(frame_u8, box):
    """The line of a non-square box that the pad replicates, its neighbour inside the box and the frame's line just past it
    (None where there is none): (edge, inner, outer).  xs > ys replicates the last COLUMN, xs < ys the last ROW (the swap)."""
    x0, y0, x1, y1 = box
    xs, ys = x1 - x0, y1 - y0
    assert xs != ys
    fh, fw = frame_u8.shape
    if xs > ys:
        line = lambda x: frame_u8[y0:y1, x] if x0 - 1 <= x < fw else None      # noqa: E731
        return line(x1 - 1), (line(x1 - 2) if xs > 1 else None), line(x1)
    line = lambda y: frame_u8[y, x0:x1] if y0 - 1 <= y < fh else None          # noqa: E731
    return line(y1 - 1), (line(y1 - 2) if ys > 1 else None), line(y1)


# ---- launches of several crops ----------------------------------------------------------------------------------------------
Batch = collections.namedtuple("Batch", "name frame boxes fidx S rgb")
TARGET = (33, 21, 90, 78)                                  # the box whose bits must not depend on its batch (frame 1 of A3)
FILL = ((0, 0, 40, 40), (120, 90, 197, 151), (10, 100, 60, 130), (150, 5, 170, 60), (70, 70, 71, 71), (5, 5, 105, 105))
BATCHES = (
    Batch("alone", "A3", (TARGET,), (1,), 24, False),
    Batch("first", "A3", (TARGET,) + FILL, (1, 0, 2, 1, 0, 2, 1), 24, False),
    Batch("middle", "A3", FILL[:3] + (TARGET,) + FILL[3:], (0, 2, 1, 1, 0, 2, 1), 24, False),
    Batch("last", "A3", FILL + (TARGET,), (0, 2, 1, 0, 2, 1, 1), 24, False),
    Batch("permuted", "A3", FILL + (TARGET,), (2, 0, 0, 1, 2, 0, 2), 24, False),
    Batch("identity", "A3", FILL[:2] + (TARGET,), (0, 1, 2), 24, False),
    Batch("rgb-S64", "C3", ((20, 10, 100, 90), (0, 0, 173, 131), (100, 50, 140, 75)), (2, 0, 1), 64, True),
    Batch("rgb-S257", "C3", ((60, 40, 101, 81), (130, 20, 155, 60)), (1, 1), 257, True),
    Batch("rgb-identity", "C3", ((5, 7, 45, 32), (9, 9, 41, 41), (0, 91, 173, 131)), (0, 1, 2), 32, True),
)
TARGET_AT = {"alone": 0, "first": 0, "middle": 3, "last": 6}


def gray(name):
    """The gray plane(s) the resize sees."""
    return luma(frame(name)) if name == "C3" else frame(name)


# ---- crops esahrnet_crops_ex must not serve ----------------------------------------------------------------------------------
# Five served crops on the three frames of A3; each row replaces the crop at `pos`: (name, pos, box or None, fidx or None, valid)
NS_BOXES = ((0, 0, 40, 40), TARGET, (120, 90, 197, 151), (10, 100, 60, 130), (150, 5, 170, 60))
NS_FIDX = (0, 1, 2, 1, 0)
NS_S = 24
NOT_SERVED = (
    ("valid0-first", 0, None, None, 0), ("valid0-middle", 2, None, None, 0), ("valid0-last", 4, None, None, 0),
    ("fidx-minus1", 1, None, -1, 1), ("fidx-nframes", 3, None, 3, 1),
    ("empty-x", 2, (50, 20, 50, 60), None, 1), ("empty-y", 0, (50, 20, 90, 20), None, 1),
    ("reversed-x", 4, (90, 20, 50, 60), None, 1), ("reversed-y", 1, (50, 60, 90, 20), None, 1),
    ("x0-negative", 2, (-3, 20, 37, 60), None, 1), ("y0-negative", 3, (20, -1, 60, 39), None, 1),
    ("x1-past-FW", 0, (160, 20, 198, 58), None, 1), ("y1-past-FH", 4, (20, 120, 52, 152), None, 1),
    ("x0-INT32_MIN", 1, (INT32_MIN, 20, 40, 60), None, 1), ("x1-INT32_MAX", 2, (10, 20, INT32_MAX, 60), None, 1),
    ("x-both-extremes", 3, (INT32_MIN, 20, INT32_MAX, 60), None, 1), ("y-both-extremes", 0, (20, INT32_MIN, 60, INT32_MAX), None, 1),
)


def rows():
    """Every served crop of the tables as (class, name, gray frame [FH, FW], box, S): CASES, then each crop of BATCHES."""
    for c in CASES:
        yield c.cls, c.name, frame(c.frame), c.box, c.S
    for b in BATCHES:
        g = gray(b.frame)
        for i, (box, fi) in enumerate(zip(b.boxes, b.fidx)):
            yield "batching", f"batching-{b.name}-{i}", g[fi], box, b.S
