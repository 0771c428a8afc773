"""The CBAM kernels (cbam.hip: pool_partial, ca_mlp, cbam_maps, cbam_apply, cbam_spatial) and the pooling stem (stem.hip:
launch_stem_pool) restated step by step in plain torch — test helper, never shipped.

  * ref_partial / ref_ca / ref_maps / ref_y: each step in float64.  Composed they are oracle.hrnet_ref._cbam run in float64
    (tests/test_cbam_host.py holds them to it at 1e-12): the section references are the project's oracle cut at the buffers the
    kernels hand to each other, not a second opinion.
  * emu_ca / emu_maps / emu_y: the same steps in torch float32 in the kernels' step order, the result rounded by q_sb / q_bf
    where the format stores it (only y is stored in the format; partial, ca and maps are f32 in every mode).
  * slab geometry restated: S = ceil(HW / P); slab s holds the pixels [s * S, min(HW, s * S + S)) in row-major order; an empty
    slab holds (0, -inf).  The stem's slabs: slab `row * pieces + piece`, a piece being 256 pixels of a row.
  * planted: the inputs.  Seeded synth.normal clipped to +-4, then
      (a) per image and channel one planted value is the channel's maximum: 5 + (k + 1) / 32 with k = (7 ch + 3 img) mod 96 — numbers
          every format holds exactly, distinct among any 96 neighbouring channels (bf16 has 96 values in (5, 8]).  Its pixel
          cycles with ch + img through POSITION_CLASSES: the first and last pixel, both sides of the border between slab 0 and
          slab 1, the first and last pixel of the last non-empty slab, the last pixel of a row;
      (b) about every fifth pixel (pixel % 5 == 3, away from the pixels of (a)) holds -(M_NEG + |z|) in all real channels: the
          only input on which a padding channel's zero can win the channel maximum;
      (c) the channels 1 and c - 2 (+ img) are negative everywhere: -(1 + |z|), their planted maximum -(1/4 + k / 256) — a pool
          that starts from 0 instead of -inf shows there;
    and everything rounded to the format at the end, so that the device holds exactly the numbers the reference reads.
    A 1x1 image has one pixel: image 0 carries (a), image 1 is the all-negative pixel of (b).
  * the case tables of tests/test_gpu_cbam.py, shared with the host self-check (tests/test_cbam_host.py).
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from resample_ref import q_bf, q_sb  # noqa: E402
from esa_pose_estimation_amd import synth  # noqa: E402

Q = {0: q_sb, 1: q_bf, 2: lambda t: t}
QUANTUM = {0: 2.0 ** -17, 1: 2.0 ** -9, 2: 2.4e-7}      # head_ref.QUANTUM's figures for the three modes op_cbam serves
Q_F32 = 2.4e-7
PNAME = {0: "bf16x3", 1: "bf16", 2: "fp32"}
M_NEG = 6.0           # (b): how far below zero the all-negative pixels lie (test_cbam_host.py: why this much)
EPS24 = 2.0 ** -24


def pad(c: int, precision: int) -> int:
    m = 64 if precision == 1 else 32
    return (c + m - 1) // m * m


# ---------------------------------------------------------------------------------------------- slab geometry
def slab_rule(hw: int, slabs: int, pool_slabs: int = 64) -> int:
    """P of a case: the plan's rule min(POOL_SLABS, HW), or the count asked for."""
    return slabs if slabs else min(pool_slabs, hw)


def slab_bounds(hw: int, P: int):
    """[(p0, p1)] per slab; p1 <= p0: empty."""
    S = (hw + P - 1) // P
    return [(s * S, min(hw, s * S + S)) for s in range(P)]


def last_slab(hw: int, P: int) -> int:
    S = (hw + P - 1) // P
    return (hw + S - 1) // S - 1


POSITION_CLASSES = ("pixel 0", "pixel HW-1", "last of slab 0", "first of slab 1", "first of the last non-empty slab",
                    "last of the last non-empty slab", "a row's last pixel")


def positions(h: int, w: int, P: int):
    """{class name: pixel} at this geometry; a class that does not exist here (slab 1 with P = 1) is left out."""
    hw = h * w
    b = slab_bounds(hw, P)
    L = last_slab(hw, P)
    out = {"pixel 0": 0, "pixel HW-1": hw - 1, "last of slab 0": b[0][1] - 1}
    if P > 1 and b[1][1] > b[1][0]:
        out["first of slab 1"] = b[1][0]
    out["first of the last non-empty slab"] = b[L][0]
    out["last of the last non-empty slab"] = b[L][1] - 1
    out["a row's last pixel"] = ((h - 1) // 2) * w + w - 1
    return out


def stem_slabs(h: int, w: int, stem_px: int = 8) -> int:
    """stem_pool_slabs restated: a block is 256 threads = 32 groups of stem_px pixels x 8 channel groups."""
    xgroups = (w + stem_px - 1) // stem_px
    return h * ((xgroups * 8 + 255) // 256)


def stem_piece(stem_px: int = 8) -> int:
    return (256 // 8) * stem_px


# ---------------------------------------------------------------------------------------------- inputs
def _planted_value(ch, img):
    return 5.0 + ((7 * ch + 3 * img) % 96 + 1) / 32.0


def _planted_negative(ch, img):
    return -(0.25 + ((7 * ch + 3 * img) % 64) / 256.0)


def neg_channels(c: int, img: int):
    return sorted({(1 + img) % c, (c - 2 + img) % c})


@functools.lru_cache(maxsize=8)
def planted(c: int, h: int, w: int, n: int, precision: int, P: int):
    """-> dict(x, res, w0, w2, wsa, y0 inputs; where [n][c] planted pixel; negpix bool [n][hw]); c0 = 8, cy = c0 + Cp + 8."""
    hw, cp = h * w, pad(c, precision)
    q = Q[precision]
    tag = f"{c}x{h}x{w}"
    z = torch.from_numpy(synth.normal("cbam_x" + tag, 1, (n, c, hw))).clamp(-4.0, 4.0)
    x = z.clone()
    pos = list(positions(h, w, P).values())
    where = torch.zeros(n, c, dtype=torch.long)
    negpix = torch.zeros(n, hw, dtype=torch.bool)
    for i in range(n):
        if hw == 1:                                  # one pixel: image 0 carries (a), the others are the all-negative pixel
            if i > 0:
                negpix[i, 0] = True
        else:
            free = [p for p in range(hw) if p not in pos]
            sel = [p for p in free if p % 5 == 3] or free[:1]
            negpix[i, sel] = True
        for ch in neg_channels(c, i):
            x[i, ch] = -(1.0 + z[i, ch].abs())
        x[i][:, negpix[i]] = -(M_NEG + z[i][:, negpix[i]].abs())
        if hw == 1 and i > 0:
            continue
        for ch in range(c):
            p = pos[(ch + i) % len(pos)]
            where[i, ch] = p
            x[i, ch, p] = _planted_negative(ch, i) if ch in neg_channels(c, i) else _planted_value(ch, i)
    x = q(x.reshape(n, c, h, w))
    res = torch.from_numpy(synth.normal("cbam_r" + tag, 2, (n, c, h, w), 1.0, 0.3)).clone()
    if hw == 1:
        res[1:] += 1.5                               # the all-negative image: the ReLU stays open often enough there too
    res = q(res)
    w0 = torch.from_numpy(synth.normal("cbam_0" + tag, 3, (c // 16, c, 1, 1), 0.25 * float(np.sqrt(1.0 / c))))
    if float((w0[0, :, 0, 0].double() * x[0].double().amax((1, 2))).sum()) <= 0.0:
        w0[0] = -w0[0]                               # hidden unit 0 is open on image 0's maxima: with c = 16 it is the only one
    # fc[2] small enough that ca stays inside about (0.2, 0.8): where every channel is negative the channel maximum of ca * x is
    # the product nearest zero, and a ca near 0 would leave nothing for a wrongly winning zero to change
    w2 = torch.from_numpy(synth.normal("cbam_2" + tag, 4, (c, c // 16, 1, 1), 0.2 * float(np.sqrt(16.0 / c))))
    # the taps on the mean map N(0, 0.2), those on the maximum map +-(0.02 + 0.04 |z|), none near zero; the centre taps (the only
    # ones a 1x1 image reaches) +-0.5 on the maximum map and -+0.3 on the mean map: where every channel is negative the two
    # about cancel (0.5 x -2.5 against -0.3 x -3.5) and the sigmoid is on its slope, where a maximum map clamped at 0 shows most
    wsa = torch.from_numpy(synth.normal("cbam_s" + tag, 5, (1, 2, 7, 7), 0.2)).clone()
    zs = wsa[0, 1] / 0.2
    wsa[0, 1] = torch.sign(zs) * (0.02 + 0.04 * zs.abs())
    wsa[0, 1, 3, 3] = 0.5 * torch.sign(zs[3, 3])
    wsa[0, 0, 3, 3] = -0.3 * torch.sign(zs[3, 3])
    cy = 8 + cp + 8
    y0 = q(torch.from_numpy(synth.normal("cbam_y" + tag, 6, (n, cy, h, w))))
    return dict(x=x, res=res, w0=w0, w2=w2, wsa=wsa, y0=y0, where=where, negpix=negpix, c0=8, cy=cy, cp=cp)


# ---------------------------------------------------------------------------------------------- float64 steps
def ref_partial(x, P):
    """x [n][c][h][w] -> float64 [n][P][c][2]: (sum, max) per slab, (0, -inf) where the slab is empty."""
    n, c = x.shape[:2]
    v = x.double().reshape(n, c, -1)
    out = torch.zeros(n, P, c, 2, dtype=torch.float64)
    out[..., 1] = -float("inf")
    for s, (p0, p1) in enumerate(slab_bounds(v.shape[-1], P)):
        if p1 > p0:
            out[:, s, :, 0] = v[:, :, p0:p1].sum(-1)
            out[:, s, :, 1] = v[:, :, p0:p1].amax(-1)
    return out


def _fc(v, w0, w2):
    return F.conv2d(F.relu(F.conv2d(v, w0)), w2)


def ref_ca(partial, hw, w0, w2):
    """partial [n][P][c][2] (any float dtype: the device's, read exactly) -> ca float64 [n][c]: the slabs reduced in float64,
    avg = sum_s / HW, max_s, then the shared MLP on both and the sigmoid of the sum."""
    p = partial.double()
    avg = (p[..., 0].sum(1) / hw)[:, :, None, None]
    mx = p[..., 1].amax(1)[:, :, None, None]
    return torch.sigmoid(_fc(avg, w0.double(), w2.double()) + _fc(mx, w0.double(), w2.double()))[:, :, 0, 0]


def ref_maps(x, ca, clamp_max_at_zero=False):
    """-> float64 [n][h][w][2]: (mean_c, max_c) of ca * x over the real channels.  clamp_max_at_zero: the defect of a padding
    channel's zero winning the maximum (host test only)."""
    u = ca.double()[:, :, None, None] * x.double()
    mx = u.amax(1)
    if clamp_max_at_zero:
        mx = mx.clamp_min(0.0)
    return torch.stack([u.mean(1), mx], -1)


def ref_y(x, res, ca, maps, wsa, relu, dtype=torch.float64):
    """y = [relu](sigmoid(conv7x7(maps)) * ca * x [+ res]) on the real channels."""
    m = maps.to(dtype).permute(0, 3, 1, 2)
    sa = torch.sigmoid(F.conv2d(m, wsa.to(dtype), padding=3))
    y = (sa * ca.to(dtype)[:, :, None, None]) * x.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return F.relu(y) if relu else y


def ref_all(x, res, w0, w2, wsa, relu, P, clamp_max_at_zero=False):
    part = ref_partial(x, P)
    ca = ref_ca(part, x.shape[-2] * x.shape[-1], w0, w2)
    maps = ref_maps(x, ca, clamp_max_at_zero)
    return dict(partial=part, ca=ca, maps=maps, y=ref_y(x, res, ca, maps, wsa, relu))


def sum_bound(v, p0, p1):
    """Any-order float32 summation of m numbers: |float32 sum - exact| <= (m - 1) 2^-24 sum|v| to first order (Higham, Accuracy
    and Stability of Numerical Algorithms, eq. 4.4).  v float64 [..., HW] -> bound [...]."""
    return (p1 - p0 - 1) * EPS24 * v[..., p0:p1].abs().sum(-1)


# ---------------------------------------------------------------------------------------------- float32 emulations
def emu_partial(x, P):
    """The slab sums in float32 (torch's order); the maxima are exact in any order."""
    n, c = x.shape[:2]
    v = x.float().reshape(n, c, -1)
    out = torch.zeros(n, P, c, 2)
    out[..., 1] = -float("inf")
    for s, (p0, p1) in enumerate(slab_bounds(v.shape[-1], P)):
        if p1 > p0:
            out[:, s, :, 0] = v[:, :, p0:p1].sum(-1)
            out[:, s, :, 1] = v[:, :, p0:p1].amax(-1)
    return out


def emu_ca(partial, hw, w0, w2):
    p = partial.float()
    a = torch.zeros_like(p[:, 0, :, 0])
    for s in range(p.shape[1]):                      # ca_mlp keeps the slab order of the sum
        a = a + p[:, s, :, 0]
    avg = (a / float(hw))[:, :, None, None]
    mx = p[..., 1].amax(1)[:, :, None, None]
    return torch.sigmoid(_fc(avg, w0, w2) + _fc(mx, w0, w2))[:, :, 0, 0]


def emu_maps(x, ca):
    """float32, cbam_maps' order: a thread sums its 8 channels in turn, the groups are added in turn; the mean is the sum
    divided by C.  The maximum of the float32 products is exact in any order: the max map is held bit for bit."""
    u = ca.float()[:, :, None, None] * x.float()
    n, c, h, w = u.shape
    g = u.reshape(n, c // 8, 8, h, w)
    s8 = torch.zeros(n, c // 8, h, w)
    for i in range(8):
        s8 = s8 + g[:, :, i]
    s = torch.zeros(n, h, w)
    for k in range(c // 8):
        s = s + s8[:, k]
    return torch.stack([s / float(c), u.amax(1)], -1)


def emu_y(x, res, ca, maps, wsa, relu, precision):
    return Q[precision](ref_y(x.float(), None if res is None else res.float(), ca.float(), maps.float(), wsa, relu, torch.float32))


def bound(ref, emu, q):
    """The rule: 2 x E_emu + q x max|ref|  ->  (bound, E_emu, scale)."""
    scale = ref.abs().max().item()
    e = (emu.double() - ref).abs().max().item()
    return 2.0 * e + q * scale, e, scale


# ---------------------------------------------------------------------------------------------- the stem
STEM_SPIKE = 20.0


@functools.lru_cache(maxsize=8)
def stem_inputs(h: int, w: int, n: int = 2, piece: int = 256):
    """x [n][1][h][w]: seeded N(0, 1) with one spike per row piece, at a position that cycles with row + image through the
    piece's first and last pixel, both sides of an 8-pixel group's border and the piece's middle; conv1 weights whose centre
    tap is the largest by far, positive in the even channels (the spike's pixel is the piece's maximum there) and negative in
    the odd ones (their maximum falls wherever the reference says)."""
    x = torch.from_numpy(synth.normal(f"stem_x{h}x{w}", 1, (n, 1, h, w))).clone()
    spikes = []
    for i in range(n):
        for r in range(h):
            for k, p0 in enumerate(range(0, w, piece)):
                p1 = min(w, p0 + piece)
                cand = [p0, p1 - 1, min(p1 - 1, p0 + 7), min(p1 - 1, p0 + 8), (p0 + p1) // 2]
                px = cand[(r + i * h + k) % len(cand)]
                x[i, 0, r, px] = STEM_SPIKE
                spikes.append((i, r, px))
    wt = torch.from_numpy(synth.normal("stem_w", 2, (64, 1, 3, 3), 0.1)).clone()
    centre = 0.5 + torch.from_numpy(synth.normal("stem_wc", 3, (64,))).abs()
    wt[:, 0, 1, 1] = torch.where(torch.arange(64) % 2 == 0, centre, -centre)
    b = torch.from_numpy(synth.normal("stem_b", 4, (64,), 0.5))
    return dict(x=x, w=wt, b=b, spikes=spikes)


def ref_stem(x, w, b, relu, dtype=torch.float64):
    y = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), padding=1)
    return F.relu(y) if relu else y


def emu_stem(x, w, b, relu, precision):
    return Q[precision](ref_stem(x, w, b, relu, torch.float32))


def stem_pieces(w: int, piece: int = 256):
    return [(p0, min(w, p0 + piece)) for p0 in range(0, w, piece)]


# ---------------------------------------------------------------------------------------------- case tables
SHAPES = ((1, 1, 2), (2, 3, 2), (4, 4, 2), (7, 9, 2), (5, 13, 2), (16, 32, 2), (17, 33, 2), (40, 36, 3))     # (h, w, n)
ALL_C = (16, 24, 32, 48, 64, 96, 128, 256, 264, 384, 400, 512)
C_REFUSED = 528
EVERY_SHAPE_C = (16, 48, 64, 264)
EVERY_C_SHAPES = ((17, 33, 2), (5, 13, 2))
FUSED_SHAPES = ((4, 4, 2), (16, 32, 2), (17, 33, 2), (40, 36, 3))
SLAB_CASES = tuple((64, (17, 33, 2), P) for P in (1, 7, 8, 9, 63)) + ((64, (24, 32, 2), 768), (64, (32, 32, 2), 1024))
STEM_SHAPES = ((1, 1), (3, 21), (5, 8), (4, 256), (2, 264))


def spatial_supported(cp: int) -> bool:
    g = cp // 8
    return 1 <= g <= 32 and (g & (g - 1)) == 0


def _pairs():
    out = [(c, s) for c in ALL_C for s in EVERY_C_SHAPES]
    out += [(c, s) for s in SHAPES for c in EVERY_SHAPE_C if (c, s) not in out]
    return out


def cbam_cases():
    """[(c, (h, w, n), precision, res_relu, fused, slabs)]"""
    out = []
    for c, s in _pairs():
        for p in (0, 1, 2):
            for rr in (False, True):
                out.append((c, s, p, rr, 0, 0))
                if s in FUSED_SHAPES and spatial_supported(pad(c, p)):
                    out.append((c, s, p, rr, 1, 0))
    for c, s, P in SLAB_CASES:
        for p in (0, 1, 2):
            out.append((c, s, p, True, 0, P))
    return out


def case_id(case):
    c, (h, w, n), p, rr, fused, slabs = case
    return f"c{c}-{h}x{w}-{PNAME[p]}-{'res_relu' if rr else 'plain'}-{'fused' if fused else 'maps_apply'}" + (f"-P{slabs}" if slabs else "")


def stem_cases():
    return [(h, w, p, relu) for h, w in STEM_SHAPES for p in (0, 1, 2) for relu in (0, 1)]
