"""Every convolution launcher (conv_mfma.hip, conv_s2c32.hip, conv1x1.hip, conv_x6.hip, bblock32.hip, stem_fused.hip) restated
in plain torch — test helper, never shipped.

  * ref_conv / ref_block32 / ref_stem2: F.conv2d in float64 of the FORMAT-HELD inputs (x and res stored in the format; the
    weights rounded too in the 16-bit formats, which pack them rounded), plus bias, residual, ReLU.  The two-convolution
    kernels: the chain in float64 with nothing rounded in between.
  * conv / emu_block32 / emu_stem2: the arithmetic each kernel's header states, in torch float32, stored in the format —
    split-bf16: head_ref._sb3 (hi.hi + hi.lo + lo.hi, f32 accumulation); fp32-grade: a plain f32 convolution; bf16 / fp16:
    an f32 convolution of rounded operands.  The two-convolution kernels round the mid tensor where the kernel does: bblock32
    and stem_fused split it to hi + lo (sb.h: split4 / split8), stem_x6_kernel splits it exactly into three terms (no rounding).
    conv() is head_ref._conv generalised to stride and residual; head_ref imports it back.
  * inputs of three regimes.  "signed": synth.normal, weights N(0, 1 / fan_in).  "positive": x, w, b, res >= 0 — what ReLU
    feeds the network, and the case without cancellation that conv_x6.hip's header measures on its own.  "edge" (bblock32 and the
    fused stems): x >= 0, every weight of the FIRST convolution >= 0 and its bias +1, so that the first convolution evaluated on
    the zero-padded input is >= 1 everywhere outside the image — a mid pixel there that is not forced to zero (it is the second
    convolution's padding) shows on every tile that touches the border.  Everything is rounded to the format at the end, so
    that the device holds exactly the numbers the reference reads.
  * geometry: the launchers' arithmetic restated — items, cout slices, grids, which stream variant, the 1x1 kernels' kern2 /
    nsplit / slice choices — given a CU count (tests/test_conv_host.py holds them to hand-counted values).
  * dispatch: choose_conv / conv_kernel_name / conv_x6_kernel_name restated, so that every (row, precision) has an expected
    kernel name; the table files each row under the literal name of its home precision.
  * the case tables of tests/test_gpu_conv.py, shared with the host self-check.
"""
from __future__ import annotations

import functools
import os
import sys
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import head_ref as HR  # noqa: E402
from esa_pose_estimation_amd import synth  # noqa: E402

Q = HR.QSTORE                   # precision -> rounding of a tensor to the format (0 split-bf16, 1 bf16, 2 f32, 3 fp16)
QUANTUM = HR.QUANTUM            # one storage quantum of the format relative to the scale
PNAME = HR.PRECISION_NAME
CUS = 256                       # MI355X


def pad(c: int, p: int) -> int:
    m = 64 if p in (1, 3) else 32
    return (c + m - 1) // m * m


def out_hw(h, w, stride):
    return ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)


# ---------------------------------------------------------------------------------------------- one convolution
def conv(precision, x, w, b, stride=1, res=None, relu=False):
    """One convolution of the format on f32 tensors that are data of the format: w, b f32 (rounded here in the 16-bit formats,
    split in the split format); the result stored in the format.  Emu.conv's order: + bias, + residual, ReLU, store."""
    bb = 0.0 if b is None else b[None, :, None, None]
    pd = (w.shape[-1] - 1) // 2
    if precision == 0:
        y = HR._sb3(x, w, stride) + bb
    elif precision == 2:
        y = F.conv2d(x, w, None, stride, pd) + bb
    else:
        y = F.conv2d(x, Q[precision](w), None, stride, pd) + bb
    if res is not None:
        y = y + res
    return Q[precision](F.relu(y) if relu else y)


def held_w(precision, w):
    """The weights the reference reads: rounded in the 16-bit formats, f32 otherwise (the split and the three-term split of
    the other two are part of the kernel's arithmetic, not of its input)."""
    return Q[precision](w) if precision in (1, 3) else w


def ref_conv(precision, x, w, b, stride=1, res=None, relu=False):
    y = F.conv2d(x.double(), held_w(precision, w).double(), b.double(), stride, (w.shape[-1] - 1) // 2)
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


# ---------------------------------------------------------------------------------------------- the two-convolution kernels
def ref_block32(x, w1, b1, w2, b2, masked=True):
    """relu(conv2(relu(conv1(x) + b1)) + b2 + x), float64.  masked=False: conv1 evaluated on the zero-padded input also where
    the mid pixel lies outside the image (what bblock32.hip would compute without its `inside` test)."""
    xd = x.double()
    if masked:
        mid = F.relu(F.conv2d(xd, w1.double(), b1.double(), 1, 1))
        y = F.conv2d(mid, w2.double(), b2.double(), 1, 1)
    else:
        mid = F.relu(F.conv2d(xd, w1.double(), b1.double(), 1, 2))            # the 1-pixel ring outside the image included
        y = F.conv2d(mid, w2.double(), b2.double(), 1, 0)
    return F.relu(y + xd)


def emu_block32(x, w1, b1, w2, b2):
    mid = Q[0](F.relu(HR._sb3(x, w1) + b1[None, :, None, None]))
    return Q[0](F.relu(HR._sb3(mid, w2) + b2[None, :, None, None] + x))


def ref_stem2(x, w1, b1, w2, b2, masked=True):
    """relu(conv2_s2(relu(conv1(x) + b1)) + b2), float64; masked=False as in ref_block32."""
    xd = x.double()
    if masked:
        mid = F.relu(F.conv2d(xd, w1.double(), b1.double(), 1, 1))
        return F.relu(F.conv2d(mid, w2.double(), b2.double(), 2, 1))
    mid = F.relu(F.conv2d(xd, w1.double(), b1.double(), 1, 2))
    return F.relu(F.conv2d(mid, w2.double(), b2.double(), 2, 0))


def emu_stem2(precision, x, w1, b1, w2, b2):
    """conv1 on the f32 VALU from the raw f32 crop in both modes; the mid tile is split to hi + lo (stem_fused) or into three
    exact terms (stem_x6_kernel: nothing lost); conv2 as any convolution of the format."""
    mid = F.relu(F.conv2d(x, w1, b1, 1, 1))
    return conv(precision, Q[precision](mid), w2, b2, 2, None, True)


def unmasked_ring_min(x, w1, b1):
    """Smallest pre-ReLU value of conv1 on the ring of mid pixels just outside the image (zero-padded input)."""
    m = F.conv2d(x.double(), w1.double(), b1.double(), 1, 2)
    ring = torch.ones_like(m, dtype=torch.bool)
    ring[:, :, 1:-1, 1:-1] = False
    return m[ring].min().item()


# ---------------------------------------------------------------------------------------------- inputs
REGIMES = ("signed", "positive")
REGIMES2 = ("signed", "edge")


def _n(tag, seed, shape, std=1.0, positive=False):
    t = torch.from_numpy(synth.normal(tag, seed, tuple(shape), float(std)))
    return t.abs() if positive else t


Row = namedtuple("Row", "n cin cout h w k stride res relu")


def row_id(r: Row) -> str:
    return f"n{r.n}-c{r.cin}-{r.cout}-{r.h}x{r.w}-k{r.k}s{r.stride}" + ("-res" if r.res else "") + ("-relu" if r.relu else "")


@functools.lru_cache(maxsize=16)
def _raw(r: Row, regime: str):
    pos = regime == "positive"
    tag = row_id(r)
    oh, ow = out_hw(r.h, r.w, r.stride)
    x = _n("cx" + tag, 31, (r.n, r.cin, r.h, r.w), 1.0, pos)
    w = _n("cw" + tag, 32, (r.cout, r.cin, r.k, r.k), np.sqrt(1.0 / (r.cin * r.k * r.k)), pos)
    b = _n("cb" + tag, 33, (r.cout,), 0.1, pos)
    res = _n("cr" + tag, 34, (r.n, r.cout, oh, ow), 1.0, pos) if r.res else None
    return x, w, b, res


@functools.lru_cache(maxsize=8)
def conv_data(r: Row, regime: str, p: int, a: int = 0, bexp: int = 0):
    """dict(x, w, b, res, ref, emu) of a row in a precision: inputs held by the format, the float64 reference and the emulation —
    made once, shared, never written to.  (a, bexp): x scaled by 2^a, w by 2^bexp, b and res by 2^(a + bexp) (exact)."""
    x, w, b, res = _raw(r, regime)
    sx, sw = 2.0 ** a, 2.0 ** bexp
    x, w, b = Q[p](x) * sx, w * sw, b * (sx * sw)
    res = None if res is None else Q[p](res) * (sx * sw)
    with torch.no_grad():
        ref = ref_conv(p, x, w, b, r.stride, res, r.relu)
        emu = conv(p, x, w, b, r.stride, res, r.relu)
    return dict(x=x, w=w, b=b, res=res, ref=ref, emu=emu)


@functools.lru_cache(maxsize=8)
def block_data(n, h, w, regime, a=0, bexp=0):
    edge = regime == "edge"
    tag = f"bb{n}x{h}x{w}"
    s = np.sqrt(1.0 / 288)
    x = Q[0](_n("x" + tag, 41, (n, 32, h, w), 1.0, edge)) * 2.0 ** a
    w1 = _n("w1" + tag, 42, (32, 32, 3, 3), s, edge) * 2.0 ** bexp
    b1 = (torch.ones(32) if edge else _n("b1" + tag, 43, (32,), 0.1)) * 2.0 ** (a + bexp)
    w2 = _n("w2" + tag, 44, (32, 32, 3, 3), s) * 2.0 ** -bexp           # (so that conv2's result is on the scale of the residual x)
    b2 = _n("b2" + tag, 45, (32,), 0.1) * 2.0 ** a
    with torch.no_grad():
        return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, ref=ref_block32(x, w1, b1, w2, b2), emu=emu_block32(x, w1, b1, w2, b2))


@functools.lru_cache(maxsize=8)
def stem2_data(n, cin, h, w, cmid, cout, regime, p, a=0, bexp=0):
    edge = regime == "edge"
    tag = f"st{n}x{cin}x{h}x{w}x{cmid}x{cout}"
    x = _n("x" + tag, 51, (n, cin, h, w), 1.0, edge) * 2.0 ** a                # the raw crop: f32 in every mode
    w1 = _n("w1" + tag, 52, (cmid, cin, 3, 3), np.sqrt(1.0 / (cin * 9)), edge)
    b1 = (torch.ones(cmid) if edge else _n("b1" + tag, 53, (cmid,), 0.1)) * 2.0 ** a
    w2 = _n("w2" + tag, 54, (cout, cmid, 3, 3), np.sqrt(1.0 / (cmid * 9))) * 2.0 ** bexp
    b2 = _n("b2" + tag, 55, (cout,), 0.1) * 2.0 ** (a + bexp)
    with torch.no_grad():
        return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, ref=ref_stem2(x, w1, b1, w2, b2), emu=emu_stem2(p, x, w1, b1, w2, b2))


# ---------------------------------------------------------------------------------------------- dispatch restated
SB_S1_64, SB_S1_32 = "conv_s2c32_kernel<1, 8, 4, false>", "conv_s2c32_kernel<1, 8, 2, false>"
SB_S2_64, SB_S2_32 = "conv_s2c32_kernel<2, 4, 4, false>", "conv_s2c32_kernel<2, 4, 2, false>"
SB_RING8, SB_RING16 = "conv_mfma_ring_kernel<1, 8, 2>", "conv_mfma_ring_kernel<1, 16, 2>"
SB_TILE_P = "conv_mfma_kernel<3, 1, 16, 2, true>"
SB_1X1, SB_TILE_1X1 = "conv1x1_kernel", "conv_mfma_kernel<1, 1, 16, 2, false>"
BF_S1, BF_S2, BF_1X1 = "conv_s2c32_kernel<1, 8, 4, false, true>", "conv_s2c32_kernel<2, 4, 4, false, true>", "conv1x1_kernel<bf16>"
HF_S1, HF_S2, HF_1X1 = "conv_s2c32_kernel<1, 8, 4, false, fp16>", "conv_s2c32_kernel<2, 4, 4, false, fp16>", "conv1x1_kernel<fp16>"
X6_C1 = "conv1x1_x6_kernel"
X6_S2_64, X6_S2_32 = "conv_x6_kernel<3, 2, 4, 4, 4, 2, 1>", "conv_x6_kernel<3, 2, 2, 2, 4, 2, 1>"
X6_S1_64, X6_S1_32 = "conv_x6_kernel<3, 1, 4, 8, 4, 2, 2>", "conv_x6_kernel<3, 1, 2, 4, 4, 2, 2>"
X6_1X1_64, X6_1X1_32 = "conv_x6_kernel<1, 1, 4, 8, 4, 2, 2>", "conv_x6_kernel<1, 1, 2, 4, 4, 2, 2>"

# every name conv_kernel_name / conv_x6_kernel_name can return for esahrnet_op_conv_ex's parameters in the shipped build
REACHABLE = (SB_S1_64, SB_S1_32, SB_S2_64, SB_S2_32, SB_RING8, SB_RING16, SB_TILE_P, SB_1X1, SB_TILE_1X1, BF_S1, BF_S2, BF_1X1,
             HF_S1, HF_S2, HF_1X1, X6_C1, X6_S2_64, X6_S2_32, X6_S1_64, X6_S1_32, X6_1X1_64, X6_1X1_32)
PRECISION_OF = {**{k: 0 for k in REACHABLE[:9]}, **{k: 1 for k in REACHABLE[9:12]}, **{k: 3 for k in REACHABLE[12:15]},
                **{k: 2 for k in REACHABLE[15:]}}
# names in the sources that no operator call can reach, and why
EXCLUDED = {
    "conv_s2c32_kernel<1, 16, 4, false>": "use_th16 is false: S2_TH16 = 0 in the shipped build (an experiment kept for the record)",
    "conv_mfma_ring_kernel<2, 4, 2>": "C_TILE_S2: only where conv_s2c32_supported rejects, i.e. an image of 2 GiB or more",
    "conv_mfma_kernel<3, 2, 4, 2, true>": "C_TILE_S2, as above",
    "conv_mfma_kernel<3, 2, 4, 2, false>": "C_TILE_S2, as above (and ESA_CONV_RING = 1 takes every Cinp > 32)",
    "conv_mfma_kernel<3, 1, 8, 2, true>": "C_TILE_S1_8 needs Cinp > 32, the persistent form Cinp == 32",
    "conv_mfma_kernel<3, 1, 8, 2, false>": "ESA_CONV_RING = 1: every Cinp > 32 takes the ring kernel",
    "conv_mfma_kernel<3, 1, 16, 2, false>": "ESA_CONV_RING = 1: every Cinp > 32 takes the ring kernel",
    "conv_s2c32_f32out_kernel<1, 8, 4, true>": "out_f32 is no operator parameter: seg_hrnet3's bf16 output layer, held by tests/test_gpu_head.py",
}
C1_SB_CHUNKS, C1_16_BLOCKS, C1_X6_CHUNKS = (2, 3, 4, 6, 8, 12), (1, 2, 3, 4, 6, 8, 12), (1, 2, 3, 4, 6, 8)
X6_C1_MINCOUT, S1W_MAXC = 256, 256


def dispatch(r: Row, p: int) -> str:
    """choose_conv + conv_kernel_name for esahrnet_op_conv_ex's parameters (no out_f32, one head; images far below 2 GiB)."""
    cinp, coutp = pad(r.cin, p), pad(r.cout, p)
    oh, ow = out_hw(r.h, r.w, r.stride)
    if p == 2:
        if r.k == 1 and not r.res and cinp // 32 in C1_X6_CHUNKS and coutp >= X6_C1_MINCOUT:
            return X6_C1
        wide = coutp % 64 == 0
        if r.k == 1:
            return X6_1X1_64 if wide else X6_1X1_32
        if r.stride == 2:
            return X6_S2_64 if wide else X6_S2_32
        return X6_S1_64 if wide else X6_S1_32
    if p in (1, 3):
        names = (BF_S1, BF_S2, BF_1X1) if p == 1 else (HF_S1, HF_S2, HF_1X1)
        if r.k == 3:
            return names[0] if r.stride == 1 else names[1]
        return names[2] if not r.res and cinp // 64 in C1_16_BLOCKS else "none"
    if r.k == 1:
        return SB_1X1 if not r.res and cinp // 32 in C1_SB_CHUNKS else SB_TILE_1X1
    if r.stride == 2:
        return SB_S2_64 if coutp % 64 == 0 else SB_S2_32
    items = ((oh + 15) // 16) * ((ow + 15) // 16) * (coutp // 32)
    if items >= 8 and cinp <= S1W_MAXC:
        return SB_S1_64 if coutp % 64 == 0 else SB_S1_32
    if cinp > 32 and items < 12 and oh > 8:
        return SB_RING8
    return SB_RING16 if cinp > 32 else SB_TILE_P


# ---------------------------------------------------------------------------------------------- launch geometry restated
def stream_geometry(r: Row, p: int, cus: int = CUS):
    """launch_s2c32_t: dict(items, ctiles, grid, double_buffered) of a stream-kernel launch (16-column tiles of 8 rows, 4 at
    stride 2; a workgroup covers 64 couts, or 32 in the split format where the padded couts are no multiple of 64)."""
    coutp = pad(r.cout, p)
    oh, ow = out_hw(r.h, r.w, r.stride)
    th = 8 if r.stride == 1 else 4
    per = 64 if (p != 0 or coutp % 64 == 0) else 32
    ctiles = coutp // per
    items = r.n * ((oh + th - 1) // th) * ((ow + 15) // 16) * ctiles
    grid = min(items, 2 * cus)
    if grid > ctiles:
        grid -= grid % ctiles
    return dict(items=items, ctiles=ctiles, grid=grid, double_buffered=r.stride == 1 and items <= cus)


def tile_geometry(r: Row, cus: int = CUS):
    """launch_tp<3, 1, 16, 2, true> (the persistent tile kernel of a 32-channel input): 16x16 tiles, 32-cout slices, two
    workgroups per CU."""
    coutp = pad(r.cout, 0)
    items = r.n * ((r.h + 15) // 16) * ((r.w + 15) // 16) * (coutp // 32)
    return dict(items=items, ctiles=coutp // 32, grid=min(items, 2 * cus))


def x6_geometry(r: Row, cus: int = CUS, limit: int = 1 << 30):
    """launch_x6_t (test_gpu_x6_resident.py::_geometry with the grid): rows per tile 8 at stride 1, 4 at stride 2."""
    coutp = pad(r.cout, 2)
    per = 64 if coutp % 64 == 0 else 32
    oh, ow = out_hw(r.h, r.w, r.stride)
    th = 4 if r.stride == 2 else 8
    ctiles = coutp // per
    items = r.n * ((oh + th - 1) // th) * ((ow + 15) // 16) * ctiles
    grid = min(items, min(2 * cus, limit))
    if grid > ctiles:
        grid -= grid % ctiles
    return dict(items=items, ctiles=ctiles, grid=grid)


def conv1x1_geometry(r: Row, p: int, cus: int = CUS):
    """launch_conv1x1_n: a tile is 16 pixels of a row; kern2 (two tiles per wave, 16-bit formats with <= 4 blocks) from 32 * cus
    tiles on; otherwise four tiles a workgroup and, from 1024 padded couts on, the couts cut into nsplit <= 8 parts."""
    cinp, coutp = pad(r.cin, p), pad(r.cout, p)
    ntiles = r.n * r.h * ((r.w + 15) // 16)
    if p in (1, 3) and cinp // 64 <= 4 and ntiles >= 32 * cus:
        return dict(ntiles=ntiles, kern2=True, nblk=(ntiles + 7) // 8, nsplit=1)
    nblk = (ntiles + 3) // 4
    nsplit = min(8, max(1, (4 * cus + nblk - 1) // nblk)) if coutp // 32 >= 32 else 1
    return dict(ntiles=ntiles, kern2=False, nblk=nblk, nsplit=nsplit)


def conv1x1_x6_geometry(r: Row, cus: int = CUS):
    """launch_c1_x6_t: PG pixel groups a wave (2 up to 4 chunks, else 1); cout slices of >= 4 tiles of 16 until there are four
    workgroups per CU."""
    cinp, coutp = pad(r.cin, 2), pad(r.cout, 2)
    pg = 2 if cinp // 32 <= 4 else 1
    ntiles = r.n * r.h * ((r.w + 15) // 16)
    nblk = (ntiles + 4 * pg - 1) // (4 * pg)
    ntile16 = coutp // 16
    want = min((4 * cus + nblk - 1) // nblk, ntile16 // 4)
    slices = max(1, want)
    per = (ntile16 + slices - 1) // slices
    return dict(ntiles=ntiles, nblk=nblk, per=per, slices=(ntile16 + per - 1) // per)


def block_geometry(n, h, w, cus: int = CUS):
    items = n * ((h + 15) // 16) * ((w + 15) // 16)
    return dict(items=items, grid=min(items, cus))


# ---------------------------------------------------------------------------------------------- the case table
def R(n, cin, cout, h, w, k=3, stride=1, res=False, relu=False):
    return Row(n, cin, cout, h, w, k, stride, res, relu)


def S2(*a, **kw):
    return R(*a, stride=2, **kw)


def K1(*a, **kw):
    return R(*a, k=1, **kw)


# Spatial classes against 16-column tiles of 8 / 16 rows (4 output rows at stride 2): smaller than a tile (7x5), exactly one tile
# (8x16, 16x16; stride 2: 8x32), one pixel past (17x33), partial both ways (20x24), odd stride-2 sizes (17x31, 34x30).  n 1..3.
# Chunks of 32 input channels: 1, 2, 3, 4, 8, 15 (cin 480) where the kernel has them; 12 blocks of 64 for the 16-bit 1x1.  Cout
# slices of 32, 64, 96 (three 32-slices), 128.  Channel padding on both sides: cin 8 and 48, cout 11 and 16.
# kernel name -> rows filed under it (its home precision: PRECISION_OF).  Every row also runs in every other precision whose
# dispatch serves it, under the name `dispatch` gives.
TABLE = {
    # -- split-bf16: the stream kernel needs >= 8 items of 16x16x32 couts an image and <= 256 input channels
    SB_S1_64: [R(2, 64, 128, 17, 33), R(1, 32, 256, 7, 5), R(3, 256, 64, 20, 24, res=True, relu=True), R(1, 48, 64, 34, 30, relu=True),
               R(2, 8, 64, 20, 24), R(1, 96, 128, 17, 33, res=True), R(1, 128, 64, 33, 33, relu=True)],
    SB_S1_32: [R(2, 32, 11, 33, 33), R(3, 64, 96, 20, 24, res=True, relu=True), R(1, 96, 16, 33, 33), R(1, 256, 32, 34, 49, relu=True)],
    SB_RING8: [R(2, 64, 64, 16, 16), R(3, 128, 32, 20, 24, res=True, relu=True), R(1, 480, 48, 9, 17), R(2, 96, 11, 17, 33)],
    SB_RING16: [R(2, 64, 64, 7, 5), R(2, 64, 32, 8, 16, res=True, relu=True), R(1, 288, 128, 17, 33), R(1, 480, 64, 8, 17, relu=True),
                R(2, 128, 96, 5, 20)],
    SB_TILE_P: [R(3, 32, 32, 20, 24, res=True, relu=True), R(2, 8, 11, 7, 5), R(2, 32, 96, 16, 16), R(1, 32, 32, 17, 33, relu=True)],
    SB_S2_64: [S2(2, 32, 64, 17, 31), S2(3, 64, 128, 34, 30, relu=True), S2(1, 256, 64, 8, 32), S2(2, 48, 64, 7, 5), S2(1, 480, 64, 9, 9),
               S2(1, 96, 128, 20, 24, res=True, relu=True)],
    SB_S2_32: [S2(2, 32, 32, 17, 31, relu=True), S2(3, 64, 96, 20, 24), S2(1, 32, 11, 34, 30), S2(1, 128, 16, 8, 32, res=True)],
    SB_1X1: [K1(2, 64, 64, 17, 33), K1(1, 96, 32, 7, 5, relu=True), K1(3, 128, 96, 20, 24), K1(1, 192, 64, 16, 16), K1(2, 256, 11, 5, 17),
             K1(1, 384, 128, 9, 9, relu=True), K1(2, 64, 1024, 8, 8)],
    SB_TILE_1X1: [K1(2, 32, 64, 17, 33), K1(2, 64, 64, 20, 24, res=True, relu=True), K1(1, 480, 32, 7, 5), K1(1, 8, 16, 16, 16)],
    # -- bf16 / fp16: blocks of 64 channels; every 3x3 is the stream kernel
    BF_S1: [R(2, 64, 64, 17, 33), R(3, 128, 128, 20, 24, res=True, relu=True), R(1, 48, 11, 7, 5), R(1, 192, 64, 8, 16),
            R(1, 512, 64, 16, 16, relu=True)],
    BF_S2: [S2(2, 64, 64, 17, 31), S2(3, 128, 128, 34, 30, relu=True), S2(1, 8, 16, 7, 5), S2(1, 64, 64, 8, 32), S2(1, 960, 64, 9, 9)],
    BF_1X1: [K1(2, 64, 64, 17, 33), K1(1, 128, 48, 7, 5, relu=True), K1(3, 192, 128, 20, 24), K1(1, 256, 64, 16, 16), K1(1, 384, 11, 5, 17),
             K1(1, 512, 64, 9, 9), K1(1, 768, 128, 9, 9, relu=True), K1(2, 64, 1024, 8, 8)],
    # -- fp32-grade
    X6_C1: [K1(2, 32, 256, 17, 33), K1(1, 64, 256, 7, 5, relu=True), K1(3, 96, 288, 20, 24), K1(1, 128, 480, 16, 16), K1(1, 192, 256, 9, 9),
            K1(2, 256, 272, 5, 17, relu=True)],
    X6_S2_64: [S2(2, 32, 64, 17, 31), S2(3, 64, 128, 34, 30, relu=True), S2(1, 480, 64, 9, 9), S2(1, 64, 64, 8, 32, res=True)],
    X6_S2_32: [S2(2, 32, 32, 17, 31, relu=True), S2(3, 64, 96, 20, 24), S2(1, 32, 11, 34, 30)],
    X6_S1_64: [R(2, 64, 64, 7, 5), R(2, 64, 128, 17, 33), R(3, 256, 64, 20, 24, res=True, relu=True), R(1, 480, 64, 8, 16)],
    X6_S1_32: [R(3, 32, 32, 20, 24, res=True, relu=True), R(2, 64, 96, 17, 33), R(1, 8, 11, 7, 5)],
    X6_1X1_64: [K1(2, 64, 64, 17, 33), K1(2, 64, 256, 20, 24, res=True, relu=True), K1(1, 480, 128, 7, 5)],
    X6_1X1_32: [K1(2, 32, 32, 17, 33), K1(3, 128, 96, 20, 24, res=True, relu=True), K1(1, 8, 16, 16, 16)],
}
TABLE[HF_S1], TABLE[HF_S2], TABLE[HF_1X1] = TABLE[BF_S1], TABLE[BF_S2], TABLE[BF_1X1]


def table_rows():
    """Every distinct row of the table, in table order."""
    seen = {}
    for rows in TABLE.values():
        for r in rows:
            seen.setdefault(r, None)
    return list(seen)


def single_cases():
    """[(row, precision, expected kernel name)]: every row in every precision that serves it."""
    return [(r, p, dispatch(r, p)) for r in table_rows() for p in (0, 1, 2, 3) if dispatch(r, p) != "none"]


def case_id(c):
    return f"{row_id(c[0])}-{PNAME[c[1]]}"


# ---------------------------------------------------------------------------------------------- CU-limit sweeps
CU_LIMITS = (1, 2, 3)
# (row, precision, what the limit changes).  Three images; under a limit of 1 every workgroup walks >= 4 items.
SWEEP_CASES = [
    (R(3, 64, 128, 20, 24, res=True, relu=True), 0, "stream"), (R(3, 64, 96, 20, 24, res=True, relu=True), 0, "stream"),
    (R(3, 32, 128, 17, 31, relu=True), 0, "stream"), (R(3, 64, 96, 17, 31), 0, "stream"),
    (R(3, 32, 96, 16, 24, res=True, relu=True), 0, "tile"),
    (R(3, 64, 128, 20, 24, res=True, relu=True), 1, "stream"), (R(3, 64, 128, 17, 31, relu=True), 1, "stream"),
    (R(3, 64, 128, 20, 24, res=True, relu=True), 3, "stream"), (R(3, 64, 128, 17, 31, relu=True), 3, "stream"),
    (R(3, 64, 128, 20, 24, res=True, relu=True), 2, "x6"), (R(3, 32, 128, 17, 31, relu=True), 2, "x6"),
    (R(3, 32, 32, 20, 24, res=True, relu=True), 2, "x6"), (R(3, 64, 96, 20, 24), 2, "x6"),
    # the 1x1 kernels across kern2 (16-bit, from 32 tiles a CU) and nsplit / the x6 slices (wide outputs on small grids)
    (R(2, 64, 64, 17, 33, k=1, relu=True), 1, "kern2"), (R(2, 128, 64, 17, 33, k=1), 3, "kern2"), (R(3, 256, 128, 20, 24, k=1), 1, "kern2"),
    (R(2, 64, 1024, 8, 8, k=1), 0, "nsplit"), (R(2, 64, 1024, 8, 8, k=1), 1, "nsplit"), (R(2, 64, 1024, 8, 8, k=1), 3, "nsplit"),
    (R(2, 64, 256, 8, 8, k=1, relu=True), 2, "slices"), (R(2, 256, 480, 5, 17, k=1), 2, "slices"),
]
SWEEP_BLOCKS = [(3, 20, 24), (2, 17, 33)]


def sweep_id(c):
    return f"{row_id(c[0])}-{PNAME[c[1]]}-{c[2]}"


# ---------------------------------------------------------------------------------------------- merged launches
# Member pools per (k, stride): (cin, cout, h, w, n, res, relu), unequal sizes in an order that is NOT longest-first, so that
# the launcher's sort by steps reorders them.  Channel counts serve every format (multiples of 64 after padding where a
# predicate wants them); a stride-1 3x3 member is a stream-kernel launch on its own in the split format (>= 8 items an image).
POOL = {
    (3, 1): [(64, 64, 34, 30, 2, True, True), (256, 256, 7, 5, 2, True, True), (128, 128, 17, 33, 2, False, True), (64, 128, 20, 24, 3, False, False)],
    (3, 2): [(64, 64, 17, 31, 2, False, True), (128, 256, 9, 9, 2, False, False), (64, 128, 34, 30, 3, False, True), (128, 64, 20, 24, 1, False, False)],
    (1, 1): [(64, 64, 17, 33, 2, False, True), (256, 64, 5, 9, 2, False, False), (128, 128, 9, 17, 3, False, False), (256, 64, 7, 5, 1, False, True),
             (128, 64, 20, 24, 2, False, False), (64, 128, 8, 16, 2, False, True)],
}
# the split format and the fp32-grade mode also merge 32-multiples (a 32-cout member beside 64-cout ones: both bodies in one grid)
POOL32 = {
    (3, 1): [(32, 96, 20, 24, 2, True, True), (64, 64, 34, 30, 2, True, True), (128, 32, 33, 49, 1, False, True)],
    (3, 2): [(32, 32, 17, 31, 2, False, True), (64, 96, 34, 30, 2, False, False), (32, 64, 20, 24, 3, False, True)],
}
MAXJOBS = {(0, 3): 4, (1, 3): 4, (3, 3): 4, (2, 3): 6, (0, 1): 6, (2, 1): 6}     # (precision, k) -> members a merged launch takes


def group_cases():
    """[(precision, k, stride, members)] with 2 .. the launcher's maximum members."""
    out = []
    for p in (0, 1, 2, 3):
        for (k, s), pool in POOL.items():
            if (p, k) not in MAXJOBS:
                continue                      # the 16-bit formats have no merged 1x1 launch: refused (test_refusals)
            top = min(MAXJOBS[(p, k)], len(pool))
            for cnt in sorted({2, 3, top}):
                out.append((p, k, s, tuple(pool[:cnt])))
        if p in (0, 2):
            for (k, s), pool in POOL32.items():
                out.append((p, k, s, tuple(pool)))
    return out


def group_id(c):
    p, k, s, members = c
    return f"{PNAME[p]}-k{k}s{s}-" + "+".join(f"{m[0]}>{m[1]}" for m in members)


def member_row(m, k, s):
    cin, cout, h, w, n, res, relu = m
    return Row(n, cin, cout, h, w, k, s, res, relu)


def group_steps(rows, p, cus: int = CUS):
    """launch_jobs_t / launch_x6_jobs_t: per member ceil(items / grid) * chunks — the key the launcher sorts by, longest first."""
    out = []
    for r in rows:
        g = x6_geometry(r, cus) if p == 2 else stream_geometry(r, p, cus)
        out.append(-(-g["items"] // g["grid"]) * (pad(r.cin, p) // (64 if p in (1, 3) else 32)))
    return out


# ---------------------------------------------------------------------------------------------- multi-head, bblock32, stems
# (n, cin, h, w, couts per head, relu flags): totals a multiple of 64 (64-cout workgroups) and not (32-cout ones)
MULTI_CASES = [
    (2, 32, 17, 31, (32, 32), (1, 0)), (3, 64, 34, 30, (32, 64), (0, 1)), (2, 32, 20, 24, (64, 32, 32), (1, 0, 1)),
    (1, 96, 7, 5, (32, 32, 32), (0, 1, 0)), (2, 64, 8, 32, (64, 64), (1, 1)),
]
BLOCK_SHAPES = [(2, 7, 5), (1, 16, 16), (2, 17, 33), (3, 20, 24), (1, 32, 17)]
# (n, cin, h, w, cmid, cout, precision): stem_fused per path — Coutp 64 (launch_sf64), 128 (two cout tiles a workgroup), 96 (an
# odd tile count, one a workgroup) — cin 1..4; stem_x6_kernel where it serves
STEM2_CASES = [
    (2, 1, 17, 31, 64, 64, 0), (1, 2, 7, 5, 64, 64, 0), (2, 3, 34, 30, 64, 48, 0), (1, 4, 8, 32, 32, 64, 0), (3, 1, 20, 24, 64, 64, 0),
    (2, 1, 17, 33, 64, 128, 0), (1, 3, 20, 24, 96, 128, 0), (2, 2, 17, 31, 64, 96, 0), (1, 4, 7, 5, 32, 80, 0),
    (2, 1, 17, 31, 64, 64, 2), (1, 1, 7, 5, 64, 128, 2), (3, 1, 20, 24, 64, 64, 2), (1, 1, 34, 30, 64, 48, 2), (1, 1, 8, 32, 64, 128, 2),
]

# ---------------------------------------------------------------------------------------------- power-of-two scaling
SCALES = ((12, -7), (-12, 7))
# one row per kernel family and precision 0, 1, 2 (fp16 has no room for 2^12)
SCALE_ROWS = [
    (R(2, 64, 128, 17, 33, res=True, relu=True), (0, 1, 2)), (R(2, 64, 96, 17, 31, relu=True), (0, 2)), (R(2, 64, 64, 17, 31, relu=True), (1,)),
    (R(2, 64, 64, 17, 33, k=1, relu=True), (0, 1, 2)), (R(2, 64, 64, 16, 16, res=True), (0,)), (R(2, 64, 64, 7, 5), (0,)),
    (R(2, 32, 32, 20, 24, res=True, relu=True), (0, 2)), (R(2, 32, 64, 17, 33, k=1, res=True), (0,)), (R(1, 64, 256, 7, 5, k=1), (2,)),
]
