"""References and case tables for the resampling kernels (fuse.hip: fuse_kernel / fuse2x2_kernel; cbam.hip:
resample_slice_*_kernel, zero_slice_*_kernel) — test helper, never shipped.

  * fuse / resample: the operation in float64 through F.interpolate(mode="bilinear"); fuse32 / resample32: the same in
    torch float32, the yardstick of the fp32-grade bound (tests/test_gpu_fp32.py::test_op_conv_fp32_grade's rule).
  * taps: the kernels' tap rule (lerp_scaled in fuse.hip, lerp_any in cbam.hip) restated in numpy float32, checked against
    ATen over every level pair a crop side of 16..512 produces (tests/test_resample_host.py): the all-sizes check, on the CPU.
  * claim_2x2: what fuse2x2_kernel assumes about the taps of a 2-pixel block.
  * the case tables of tests/test_gpu_resample.py, shared with the host self-check of the reference.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------- references
def _up(t, H, W, align):
    if tuple(t.shape[-2:]) == (H, W):
        return t
    return F.interpolate(t, size=(H, W), mode="bilinear", align_corners=bool(align))


def _fuse(xs, H, W, relu, dtype):
    y = None
    for t in xs:
        u = _up(t.to(dtype), H, W, 0)
        y = u.clone() if y is None else y + u
    return F.relu(y) if relu else y


def fuse(xs, H, W, relu):
    """y = [relu](sum_i up(x_i)), align_corners=False, float64."""
    return _fuse(xs, H, W, relu, torch.float64)


def fuse32(xs, H, W, relu):
    return _fuse(xs, H, W, relu, torch.float32)


def resample(x, H, W, align):
    return _up(x.double(), H, W, align).clone()


def resample32(x, H, W, align):
    return _up(x.float(), H, W, align).clone()


# ---------------------------------------------------------------------------------------------- format roundings
def q_sb(t):
    """split-bf16 storage: hi = bf16(v), lo = bf16(v - hi), value hi + lo (oracle/emulate_split_bf16.rq)."""
    hi = t.to(torch.bfloat16).to(torch.float32)
    return hi + (t - hi).to(torch.bfloat16).to(torch.float32)


def q_bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ---------------------------------------------------------------------------------------------- the tap rule
def taps(inn: int, out: int, align: int = 0, fused: bool = True):
    """(i0, i1, l0, l1) for every destination index 0..out-1, in the float32 arithmetic of lerp_scaled / lerp_any:
    scale as the f32 quotient; src = scale * (dst + 0.5) - 0.5 clamped at 0, or scale = (in - 1) / (out - 1), src = scale * dst;
    i0 = min(int(src), in - 1); i1 = i0 + (i0 < in - 1); l1 = src - i0; l0 = 1 - l1.
    fused: scale * (dst + 0.5) - 0.5 with ONE rounding (a fused multiply-add: what hipcc's default contraction makes of the
    expression on the device, and what ATen's AVX2 / AVX-512 builds do); otherwise the product is rounded first.  The two differ
    by an ulp of src here and there, and where src lands on an integer in one and just below it in the other the pair (i0, l1)
    reads (k, 0) in one and (k - 1, 1 - 2^-24) in the other: as weights on the source row the same to 2 ulp of the source
    size (tests/test_resample_host.py asserts that figure)."""
    f = np.float32
    dst = np.arange(out, dtype=np.float32)
    if align:
        scale = f(inn - 1) / f(out - 1) if out > 1 else f(0)
        src = scale * dst
    else:
        scale = f(inn) / f(out)
        if fused:       # exact in f64: a 24-bit scale times a 10-bit (dst + 0.5), minus 0.5; then the one rounding
            src = (np.float64(scale) * (dst.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
        else:
            src = scale * (dst + f(0.5)) - f(0.5)
        src = np.where(src < 0, f(0), src)
    src = src.astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), inn - 1)
    i1 = i0 + (i0 < inn - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (f(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def tap_matrix(inn: int, out: int, align: int = 0, fused: bool = True):
    """[out][in] float32: what the tap rule makes of one-hot rows (l0 at i0 plus l1 at i1, added in f32 where they meet)."""
    i0, i1, l0, l1 = taps(inn, out, align, fused)
    m = np.zeros((out, inn), np.float32)
    d = np.arange(out)
    m[d, i0] = l0
    m[d, i1] = (m[d, i1] + l1).astype(np.float32)       # i1 == i0 at the last source index: l0 * 1 + l1 * 1
    return m


def aten_matrix(inn: int, out: int, align: int = 0):
    """The same through torch's float32 F.interpolate of the one-hot rows (interpolated along the width; the height stays)."""
    if inn == out:
        return np.eye(inn, dtype=np.float32)
    x = torch.eye(inn, dtype=torch.float32).reshape(1, inn, 1, inn)
    y = F.interpolate(x, size=(1, out), mode="bilinear", align_corners=bool(align))
    return y[0, :, 0, :].T.contiguous().numpy()


def level_chain(s: int, depth: int = 3):
    """Sides of the levels under a side of s: every level is (h + 1) / 2 of the one above (stride-2 3x3, padding 1)."""
    out = [s]
    for _ in range(depth):
        out.append((out[-1] + 1) // 2)
    return out


def chain2(h: int, w: int, depth: int = 3):
    return list(zip(level_chain(h, depth), level_chain(w, depth)))


def claim_2x2(inn: int, out: int, fused: bool = True):
    """fuse2x2_kernel's claim for a pair of neighbouring destination indices (Y, Y + 1), Y even, out even:
    (first) i0(Y+1) is i0(Y) or i1(Y) — the kernel's select between rows a and b; (cell) the two pixels share both taps.
    The claim's middle part, "the taps of both lie in {i0(Y), i1(Y), i1(Y+1)}", says nothing beyond (first): i1(Y+1) is a
    loaded row by definition, so only i0(Y+1) can fall outside the set.  Returns (first, cell) over all pairs."""
    i0, i1, _, _ = taps(inn, out, 0, fused)
    a, b, a1, c = i0[0::2], i1[0::2], i0[1::2], i1[1::2]
    first = (a1 == a) | (a1 == b)
    cell = (a1 == a) & (c == b)
    return bool(first.all()), bool(cell.all())


# ---------------------------------------------------------------------------------------------- GPU cases
C18 = chain2(18, 34)            # [(18, 34), (9, 17), (5, 9), (3, 5)]: the non-exact ratios a 2x-strided network really has
C36 = chain2(36, 132)           # [(36, 132), (18, 66), (9, 33), (5, 17)]

# (id, n, c, (H, W), term sizes) — fp32-grade (precision 2), each with relu 0 and 1
FUSE_TABLE = [
    ("chain18x34", 2, 40, (18, 34), C18),                                # 2x2 kernel, selection path; ratios 2, 3.6/3.78, 6/6.8
    ("cell16x32", 2, 40, (16, 32), [(16, 32), (4, 4), (2, 8)]),          # cell path with ry != rx (4/8, 8/4)
    ("nocell16x32", 2, 40, (16, 32), [(4, 5)]),                          # exact in y only: no cell
    ("ratio16_32", 2, 40, (32, 32), [(2, 2), (1, 1)]),                   # ratio 16 / 32, in - 1 = 0
    ("fallback_h", 2, 40, (18, 34), [(10, 18)]),                         # 2h > H: fuse_kernel
    ("fallback_w", 2, 40, (18, 34), [(9, 18)]),                          # 2w > W: fuse_kernel
    ("odd9x17", 2, 40, (9, 17), C18[1:]),                                # odd grid: fuse_kernel
    ("chain36x132", 3, 8, (36, 132), C36),                               # > 1 block per row (2x2: 66 * 4 threads), batch indexing
]

# the 14 (NS, NU) of launch_fuse's switch
NSNU = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (4, 0)]
UP18 = C18[1:] + [(2, 3)]       # up-sampled terms for output 18x34; the fourth is the chain's next level


def nsnu_sizes(ns: int, nu: int):
    """Term sizes of an (NS, NU) case at output 18x34, in a shuffled order [up, same, up, same, ...]: launch_fuse must put
    the same-resolution terms first itself."""
    ups, sames = list(UP18[:nu]), [C18[0]] * ns
    order = []
    while ups or sames:
        if ups:
            order.append(ups.pop(0))
        if sames:
            order.append(sames.pop(0))
    return order


# precisions 0, 1, 3: the chain and the odd grid at (1, 3), and three more instantiations the plan emits
FUSE_LOWP = [
    ("chain18x34", 2, 40, (18, 34), C18),
    ("odd9x17", 2, 40, (9, 17), C18[1:]),
    ("ns2nu1", 2, 8, (18, 34), nsnu_sizes(2, 1)),
    ("ns3nu1", 2, 8, (18, 34), nsnu_sizes(3, 1)),
    ("ns4nu0", 2, 8, (18, 34), nsnu_sizes(4, 0)),
]
# fuse_kernel with more than one block per row and n = 3 (split-bf16 and bf16 instantiations)
FUSE_LOWP_WIDE = ("chain36x132", 3, 8, (36, 132), C36)

# (id, (h, w), (H, W)) — each with align 0 and 1, precisions 0, 1, 2
RESAMPLE_SIZES = [
    ("x2", (9, 17), (18, 34)),
    ("x3.6", (5, 9), (18, 34)),
    ("x6", (3, 5), (18, 34)),
    ("x2odd", (35, 25), (70, 50)),          # seg_hrnet3's heat-map up-sampling: align 1, x2, odd source
    ("one", (1, 1), (4, 4)),
    ("copy", (18, 34), (18, 34)),
]


@functools.lru_cache(maxsize=None)
def fuse_inputs(tag: str, n: int, c: int, sizes: tuple):
    from esa_pose_estimation_amd import synth
    return tuple(torch.from_numpy(synth.normal(f"rs_{tag}_{i}", 7, (n, c, a, b))) for i, (a, b) in enumerate(sizes))


@functools.lru_cache(maxsize=None)
def fuse_refs(tag: str, n: int, c: int, hw: tuple, sizes: tuple, relu: int):
    """(f64 reference, torch f32 result) of a fuse case; computed once, shared, never modified."""
    xs = fuse_inputs(tag, n, c, sizes)
    return fuse(xs, hw[0], hw[1], relu), fuse32(xs, hw[0], hw[1], relu)


@functools.lru_cache(maxsize=None)
def resample_input(tag: str, n: int, c: int, hw: tuple):
    from esa_pose_estimation_amd import synth
    return torch.from_numpy(synth.normal(f"rr_{tag}", 8, (n, c, hw[0], hw[1])))


# fp16 saturation (test_op_fuse_fp16_saturates at the 18x34 chain): the same-resolution term N(0, 3e4), the others N(0, 3e3)
SAT_CASE = (1, 64, (18, 34), tuple(C18))


def sat_inputs():
    n, c, _, sizes = SAT_CASE
    return tuple(t * (3.0e4 if i == 0 else 3.0e3) for i, t in enumerate(fuse_inputs("sat", n, c, sizes)))


# resample_slice beyond RESAMPLE_SIZES: (tag, n, c, (h, w), (H, W)) of the placement and the partial-group case
RESAMPLE_EXTRA = [("place", 2, 40, (5, 9), (9, 17)), ("partial", 2, 12, (5, 9), (9, 17))]


def fuse_is_copy(hw, sizes):
    """One same-resolution term: the result is the input, in every arithmetic."""
    return len(sizes) == 1 and tuple(sizes[0]) == tuple(hw)
