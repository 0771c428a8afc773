"""Everything behind stage 4, cut out of the network and restated in plain torch — test helper, never shipped.

  * head_section / output_section: the two sections in float64, written as the reference model writes them
    (models/seg_hrnet.py:461-469, 313-340; seg_hrnet3.py:506-520): up-sample, concatenate, convolve.  BatchNorm is folded
    in float64 (fold64).  Nothing here uses the per-branch linearity the kernels live on.
  * head_emulation / output_emulation: the same two sections on the same inputs with the roundings of a tensor format put
    where that format stores — split-bf16 (oracle.emulate_split_bf16's split / rq), bf16 (oracle.emulate_bf16's q),
    fp16 (fp16_emu.q16) and plain torch float32 for the fp32-grade mode.  The structure of each is its emulator's own head
    (the part of oracle.emulate_*.forward behind stage 4); tests/test_head_host.py holds them to those forwards bit for bit
    where the emulator exposes its stage-4 tensors.
  * regimes: the two weight regimes of the head tests (one branch at a time; ReLU open).
  * head_form / final_form / needs_ulo: which form the plan runs at a shape, read from esahrnet_op_desc_get (no GPU needed).
  * Config / GPU_CASES: the configurations and crops of tests/test_gpu_head.py, shared with the host sweep that checks every
    claimed form (tests/test_head_host.py).
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_emu  # noqa: E402
import resample_ref as R  # noqa: E402
from oracle import emulate_bf16 as EB  # noqa: E402
from oracle import emulate_split_bf16 as ES  # noqa: E402

BN_EPS = 1e-5
STEM = 64                      # stem width: the skip channels of seg_hrnet3's second concat


# ---------------------------------------------------------------------------------------------- float64 sections
def fold64(sd, name, bn):
    """Conv + eval-mode BatchNorm as one convolution, float64: (w [co, ci, k, k], b [co])."""
    w = sd[name + ".weight"].double()
    b = sd.get(name + ".bias")
    b = torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b.double()
    if bn:
        g = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + BN_EPS)
        w = w * g[:, None, None, None]
        b = (b - sd[bn + ".running_mean"].double()) * g + sd[bn + ".bias"].double()
    return w, b


def _cat_up(ys, dtype):
    size = ys[0].shape[-2:]
    return torch.cat([ys[0].to(dtype)] + [F.interpolate(t.to(dtype), size=size, mode="bilinear", align_corners=False)
                                          for t in ys[1:]], 1)


def _head(sd, ys, dtype):
    w0, b0 = fold64(sd, "last_layer.0", "last_layer.1")
    w3, b3 = fold64(sd, "last_layer.3", "last_layer.4")
    pre = F.conv2d(_cat_up(ys, dtype), w0.to(dtype), b0.to(dtype), padding=(w0.shape[-1] - 1) // 2)
    h0 = F.relu(pre)
    return dict(pre=pre, head0=h0, head3=F.relu(F.conv2d(h0, w3.to(dtype), b3.to(dtype))))


def head_section(sd, ys, variant=0):
    """ys = stage 4's four tensors -> {pre, head0, head3} in float64: relu(W3 . relu(W0 . cat(ys[0], up(ys[1..3])))) with
    align_corners=False up-sampling; seg_hrnet3 (variant 1): the same with its 3x3 last_layer[0] (the kernel size is the
    weight's own, so `variant` only documents the call)."""
    assert (sd["last_layer.0.weight"].shape[-1] == 3) == (variant == 1)
    return _head(sd, ys, torch.float64)


def head3_section(sd, h0):
    """head0 -> head3 alone (seg_hrnet3 materialises head0): float64."""
    w3, b3 = fold64(sd, "last_layer.3", "last_layer.4")
    return F.relu(F.conv2d(h0.double(), w3, b3))


def _output(sd, h3, x0, dtype):
    up = F.interpolate(h3.to(dtype), scale_factor=2, mode="bilinear", align_corners=True)
    return F.conv2d(torch.cat([up, x0.to(dtype)], 1), sd["output_layer.0.weight"].to(dtype), sd["output_layer.0.bias"].to(dtype),
                    padding=1)


def output_section(sd, h3, x0):
    """conv3x3(cat(up2(h3, align_corners=True), x0)), float64.  x0 is the crop (seg_hrnet / seg_hrnet2) or seg_hrnet3's
    CBAM(stem skip), which the library keeps as the first STEM channels of head_cat2 ([skip | heat-maps]: the weight's input
    channels stay in the reference's order here, [heat-maps | skip])."""
    return _output(sd, h3, x0, torch.float64)


# ---------------------------------------------------------------------------------------------- per-format emulations
QSTORE = {0: ES.rq, 1: EB.q, 2: lambda t: t, 3: fp16_emu.q16}
# one storage quantum of the format's output relative to the scale (the issue's q); the output layer's result is f32
QUANTUM = {0: 2.0 ** -17, 1: 2.0 ** -9, 2: 2.4e-7, 3: 2.0 ** -12}
Q_F32 = 2.4e-7


def _sb3(x, w, stride=1):
    """The split-bf16 product of oracle.emulate_split_bf16.Emu.conv: hi.hi + hi.lo + lo.hi, f32 accumulation, nothing stored."""
    wh, wl = ES.split(w)
    xh, xl = ES.split(x)
    pad = (w.shape[-1] - 1) // 2
    return F.conv2d(xh, wh, None, stride, pad) + F.conv2d(xh, wl, None, stride, pad) + F.conv2d(xl, wh, None, stride, pad)


def _conv(precision, x, w, b, relu):
    """One convolution of the format: w, b folded f32; the result stored in the format.  (conv_ref.conv is the one definition,
    with stride and residual; conv_ref imports this module, hence the late import.)"""
    import conv_ref
    return conv_ref.conv(precision, x, w, b, relu=relu)


def _fold32(sd, name, bn):
    w, b = fold64(sd, name, bn)
    return w.float(), b.float()


def head_emulation(sd, ys, variant, precision):
    """{head0, head3} as the format computes them from ys (f32 tensors that are data of the format).
    precision 2: torch float32 of the section as written (test_op_conv_fp32_grade's yardstick).
    seg_hrnet / seg_hrnet2, the other formats: the emulators' own head — last_layer[0] slice by slice on each branch's grid,
    every slice stored, up-sampled and summed in f32, ReLU, stored; last_layer[3] as any convolution.  Split-bf16 adds the
    bias behind the sum (oracle.emulate_split_bf16.forward), bf16 / fp16 in the branch-0 slice (oracle.emulate_bf16.forward).
    seg_hrnet3: the concat stored in the format, then the 3x3 and the 1x1 as any convolution."""
    with torch.no_grad():
        if precision == 2:
            r = _head(sd, [t.float() for t in ys], torch.float32)
            return dict(head0=r["head0"], head3=r["head3"])
        q = QSTORE[precision]
        w0, b0 = _fold32(sd, "last_layer.0", "last_layer.1")
        w3, b3 = _fold32(sd, "last_layer.3", "last_layer.4")
        size = ys[0].shape[-2:]
        if variant == 1:
            cat = torch.cat([ys[0]] + [q(F.interpolate(t, size=size, mode="bilinear", align_corners=False)) for t in ys[1:]], 1)
            h0 = _conv(precision, cat, w0, b0, True)
        else:
            off, acc = 0, None
            for b, t in enumerate(ys):
                c = t.shape[1]
                tb = _conv(precision, t, w0[:, off:off + c].contiguous(), b0 if (b == 0 and precision != 0) else None, False)
                off += c
                tb = tb if b == 0 else F.interpolate(tb, size=size, mode="bilinear", align_corners=False)
                acc = tb if acc is None else acc + tb
            if precision == 0:
                acc = acc + b0[None, :, None, None]
            h0 = q(F.relu(acc))
        return dict(head0=h0, head3=_conv(precision, h0, w3, b3, True))


def head3_emulation(sd, h0, precision):
    with torch.no_grad():
        if precision == 2:
            w3, b3 = fold64(sd, "last_layer.3", "last_layer.4")
            return F.relu(F.conv2d(h0.float(), w3.float(), b3.float()))
        w3, b3 = _fold32(sd, "last_layer.3", "last_layer.4")
        return _conv(precision, h0, w3, b3, True)


def output_emulation(sd, h3, x0, variant, precision, form):
    """The output layer as the format computes it; the result is f32 and not rounded again, except seg_hrnet3's split-bf16
    result (stored in the format before the NCHW copy).
    form "valu" (final_kernel's VALU path, and every fp32-grade output layer): torch float32, as both emulators' forwards end.
    form "mfma" (final_mfma_kernel, head.hip): the layer is split-bf16 in every mode — the interpolated value and the crop
    split into hi + lo, the weights hi + lo, three products, f32 accumulation.
    seg_hrnet3 (form "conv"): the up-sampled map is stored in the second concat in the format, then a convolution of the format
    with an f32 result (bf16) or a stored one (split-bf16)."""
    with torch.no_grad():
        w, b = sd["output_layer.0.weight"].float(), sd["output_layer.0.bias"].float()
        up = F.interpolate(h3.float(), scale_factor=2, mode="bilinear", align_corners=True)
        if precision == 2 or form == "valu":
            return F.conv2d(torch.cat([up, x0.float()], 1), w, b, padding=1)
        if form == "mfma":
            return _sb3(torch.cat([up, x0.float()], 1), w) + b[None, :, None, None]
        assert form == "conv" and variant == 1
        cat = torch.cat([QSTORE[precision](up), x0.float()], 1)
        if precision == 0:
            return ES.rq(_sb3(cat, w) + b[None, :, None, None])
        return F.conv2d(cat, QSTORE[precision](w), None, 1, 1) + b[None, :, None, None]


# ---------------------------------------------------------------------------------------------- weight regimes
# ReLU open: last_layer.1's folded bias is its BatchNorm beta plus a term that does not depend on beta, so adding a constant
# to beta shifts the folded bias by that constant.  With the synth weights (gain 0.5, unit-scale BatchNorm) the pre-activation of
# head0 has a standard deviation of about 0.5 at every width used here; 1.25 leaves it positive at > 97 % of the elements of
# the f64 reference (tests/test_head_host.py measures it with the oracle's forward and asserts >= 90 %; the GPU test asserts
# the same on the reference of the tapped inputs).  One branch at a time: a quarter of the variance, the same shift.
OPEN_SHIFT = 1.25
REGIMES = ("b0", "b1", "b2", "b3", "open")


def regime_sd(sd, widths, regime):
    """A copy of sd with the head weights of `regime`: "open" shifts last_layer.1.bias by OPEN_SHIFT; "b<i>" does the same and
    zeroes every input slice of last_layer.0 but branch i's."""
    out = dict(sd)
    out["last_layer.1.bias"] = sd["last_layer.1.bias"] + OPEN_SHIFT
    if regime != "open":
        i = int(regime[1])
        offs = np.concatenate([[0], np.cumsum(widths)])
        w = torch.zeros_like(sd["last_layer.0.weight"])
        w[:, offs[i]:offs[i + 1]] = sd["last_layer.0.weight"][:, offs[i]:offs[i + 1]]
        out["last_layer.0.weight"] = w
    return out


def open_fraction(pre):
    return float((pre > 0).double().mean())


# ---------------------------------------------------------------------------------------------- which form runs
HEAD_KERNELS = ("head_fused", "head_fused2", "head_fused_bf", "head_fused_bf<fp16>", "head_x6")


def head_ops(lib, handle, nops, n, h, w, first=0):
    """[(index, kernel, label)] of the ops from `first` on that run at this shape (esahrnet_op_desc_get leaves the kernel of a
    plan alternative the shape does not take empty)."""
    from esa_pose_estimation_amd import _lib
    rows = []
    d = _lib.OpDesc()
    for i in range(first, nops):
        rc = lib.esahrnet_op_desc_get(handle, i, n, h, w, C.byref(d))
        assert rc == 0, lib.esahrnet_last_error()
        if d.kernel:
            rows.append((i, d.kernel.decode(), d.label.decode()))
    return rows


def first_head_op(lib, handle, nops):
    """Index behind the op that writes stage4.3: everything from there on is head and output layer."""
    rows = head_ops(lib, handle, nops, 2, 64, 64)
    last = max(i for i, k, lab in rows if lab == "fuse -> stage4.3")
    return last + 1


def head_form(rows, variant):
    """The head form of an op list, and a check that exactly one alternative is listed.
    seg_hrnet / seg_hrnet2: one of HEAD_KERNELS, or "unfused" (slice convolutions + fuse -> head0 + the 1x1);
    seg_hrnet3: "gather" (head_gather + the branch-0/1 3x3 with its result as residual) or "direct"."""
    kernels = [k for _, k, _ in rows]
    labels = [lab for _, _, lab in rows]
    if variant == 1:
        gather = kernels.count("head_gather")
        l0 = [lab for lab in labels if lab.startswith("last_layer.0") and "#taps" not in lab]
        assert len(l0) == 1 and labels.count("last_layer.3") == 1, labels
        assert gather == (0 if l0[0] == "last_layer.0" else 1), labels
        return "gather" if gather else "direct"
    fused = [k for k in kernels if k in HEAD_KERNELS]
    unfused = labels.count("fuse -> head0")
    assert len(fused) + unfused == 1, kernels                       # exactly one producer of head0
    assert labels.count("last_layer.3") == unfused, labels          # the 1x1 as its own launch only behind the materialised sum
    assert kernels.count("head_t") == (2 if fused == ["head_fused2"] else 0), kernels
    nslices = sum(1 for lab in labels if lab.startswith("last_layer.0[:, ") and "+" not in lab and "T layout" not in lab)
    assert nslices == (4 if unfused else 0 if fused == ["head_fused2"] else 3), labels     # head_fused2 makes t_1 itself
    assert sum(1 for k in kernels if k.startswith("final_kernel")) == 1, kernels
    return fused[0] if fused else "unfused"


def final_form(lib, handle, variant, precision, h, w):
    """ "mfma" / "valu" (seg_hrnet / seg_hrnet2; op_desc_get names both final_kernel — the matrix-core one is the one that
    leaves per-tile maxima, esahrnet_partial_tiles) or "conv" (seg_hrnet3: a convolution of the plan)."""
    if variant == 1:
        return "conv"
    nt = C.c_int(-1)
    assert lib.esahrnet_partial_tiles(handle, h, w, C.byref(nt)) == 0
    return "mfma" if nt.value > 0 else "valu"


def _bf16_exact(v):
    return bool((v.astype(np.float32).view(np.uint32) & 0xFFFF == 0).all())


def needs_ulo(h, w):
    """head_fused2_supported's rule for carrying the lo part of U: some product of a row weight and a column weight of some
    branch is not a bf16 number (level sizes under the level-1 grid of a h x w crop)."""
    chain = R.chain2((h + 1) // 2, (w + 1) // 2)
    H, W = chain[0]
    for th, tw in chain[1:]:
        _, _, ly0, ly1 = R.taps(th, H)
        i0, i1, lx0, lx1 = R.taps(tw, W)
        wx0 = np.where(i0 == i1, lx0 + lx1, lx0).astype(np.float32)
        for ly in (ly0, ly1):
            for lx in (wx0, lx1):
                if not _bf16_exact(np.outer(ly, lx)):
                    return True
    return False


# ---------------------------------------------------------------------------------------------- configurations and cases
W18, W32, W48 = (18, 36, 72, 144), (32, 64, 128, 256), (48, 96, 192, 384)
Config = namedtuple("Config", "variant widths K precision switches")
PRECISION_NAME = {0: "bf16x3", 1: "bf16", 2: "fp32", 3: "fp16"}
VARIANT = {"seg_hrnet": 0, "seg_hrnet2": 0, "seg_hrnet3": 1}
CIN = {"seg_hrnet": 3, "seg_hrnet2": 1, "seg_hrnet3": 1}


def cfg_id(c):
    w = {W18: "w18", W32: "w32", W48: "w48"}[c.widths]
    return f"{c.variant[4:] or 'hrnet'}-{w}-k{c.K}-p{c.precision}" + "".join("-" + s.lower() for s in c.switches)


def H2(widths, precision, *switches, K=11):
    return Config("seg_hrnet2", widths, K, precision, tuple(switches))


def H3(precision, *switches):
    return Config("seg_hrnet3", W32, 30, precision, tuple(switches))


# The crops of the issue's table.  Boundary crops (the window predicates, from the host sweep) are appended per form below.
S16, S18, S70, S36, S48, S104 = (16, 16, 2), (18, 34, 2), (70, 50, 2), (36, 132, 3), (48, 80, 2), (104, 72, 2)
TABLE = (S16, S18, S70, S36, S48, S104)

# (configuration, crops, head form, output-layer form).  The host sweep (tests/test_head_host.py) found no legal crop with
# sides 16..512 at which a window predicate (head_fused2 / head_fused / head_fused_bf / head_x6 / head_gather) rejects: the
# fallbacks are reached through the switches and the channel rules only, so there is no boundary crop to add.
GPU_CASES = [
    # ---- W32, split-bf16: second generation, first generation, materialised; the VALU output layer
    (H2(W32, 0), TABLE, "head_fused2", "mfma"),
    (H2(W32, 0, "HEAD_V1"), TABLE, "head_fused", "mfma"),
    (H2(W32, 0, "UNFUSED"), TABLE, "unfused", "mfma"),
    (H2(W32, 0, "FINAL_VALU"), (S18, S36), "head_fused2", "valu"),
    # ---- W32, bf16 and fp16
    (H2(W32, 1), TABLE, "head_fused_bf", "mfma"),
    (H2(W32, 1, "BF_HEAD_VALU"), TABLE, "head_fused_bf", "mfma"),
    (H2(W32, 1, "BF_UNFUSED_HEAD"), TABLE, "unfused", "mfma"),
    (H2(W32, 1, "FINAL_VALU"), (S18, S36), "head_fused_bf", "valu"),
    (H2(W32, 3), TABLE, "head_fused_bf<fp16>", "mfma"),
    (H2(W32, 3, "BF_UNFUSED_HEAD"), (S16, S18, S70, S36), "unfused", "mfma"),
    # ---- W32, fp32-grade
    (H2(W32, 2), TABLE, "head_x6", "valu"),
    (H2(W32, 2, "X6_UNFUSED_HEAD"), (S16, S18, S70, S36), "unfused", "valu"),
    # ---- W48: C0p 64, C1p 96, head_t<6> and head_t<12>; C0p 128 in the 16-bit modes
    (H2(W48, 0), (S18, S48), "head_fused2", "mfma"),
    (H2(W48, 1), (S18, S48), "head_fused_bf", "mfma"),
    (H2(W48, 3), (S18, S48), "head_fused_bf<fp16>", "mfma"),
    # ---- W18: 144 -> 160 channels is no head_t count, the first generation runs
    (H2(W18, 0), (S18,), "head_fused", "mfma"),
    # ---- K: the 16- / 32-channel pitch of head3, a partial cout tile, final_mfma_supported's channel groups; cin = 3 once
    (H2(W32, 0, K=16), (S18,), "head_fused2", "mfma"),
    (H2(W32, 0, K=17), (S18,), "head_fused2", "mfma"),
    (H2(W32, 0, K=32), (S18,), "head_fused2", "mfma"),
    (H2(W32, 1, K=16), (S18,), "head_fused_bf", "mfma"),
    (H2(W32, 1, K=17), (S18,), "head_fused_bf", "mfma"),
    (H2(W32, 1, K=32), (S18,), "head_fused_bf", "mfma"),
    (H2(W32, 2, K=17), (S18,), "head_x6", "valu"),
    (H2(W32, 2, K=32), (S18,), "head_x6", "valu"),
    (Config("seg_hrnet", W32, 32, 0, ()), (S18,), "head_fused2", "mfma"),
    # ---- seg_hrnet3 in the precisions it has
    (H3(0), (S16, S70, S36), "gather", "conv"),
    (H3(0, "HEAD3_DIRECT"), (S16, S70, S36), "direct", "conv"),
    (H3(2), (S16, S70, S36), "gather", "conv"),
    (H3(2, "HEAD3_DIRECT"), (S70,), "direct", "conv"),
    (H3(1), (S16, S70, S36), "direct", "conv"),
]
# head_fused2 carries the lo part of U where the interpolation weights are no bf16 numbers
ULO = {S16[:2]: False, S18[:2]: True, S70[:2]: True, S36[:2]: True, S48[:2]: False, S104[:2]: True}


def expect_final(c):
    """plan_options' rule for the output layer, restated: matrix cores unless fp32-grade, seg_hrnet3, ESAHRNET_FINAL_VALU or
    a channel-group count (K + cin in groups of 8) outside 2..5."""
    if VARIANT[c.variant] == 1:
        return "conv"
    cg = (c.K + CIN[c.variant] + 7) // 8
    return "mfma" if c.precision != 2 and "FINAL_VALU" not in c.switches and 1 <= c.K <= 32 and 2 <= cg <= 5 else "valu"


def expect_fused_possible(c):
    """plan_options' channel rules, restated: the fused forms the plan may list for this configuration."""
    p32 = lambda v: (v + 31) // 32 * 32
    p64 = lambda v: (v + 63) // 64 * 64
    w, sw = c.widths, set(c.switches)
    if VARIANT[c.variant] == 1:
        return {"direct"} if c.precision in (1, 3) or "HEAD3_DIRECT" in sw else {"gather"}
    if c.precision == 0:
        if "UNFUSED" in sw or p32(w[0]) not in (32, 64):
            return set()
        head_t = lambda cp: cp // 32 in (2, 3, 4, 6, 8, 12)
        second = "HEAD_V1" not in sw and p32(w[1]) in (64, 96) and head_t(p32(w[2])) and head_t(p32(w[3]))
        return {"head_fused2", "head_fused"} if second else {"head_fused"}
    if c.precision in (1, 3):
        if "BF_UNFUSED_HEAD" in sw or p64(w[0]) not in (64, 128):
            return set()
        return {"head_fused_bf" if c.precision == 1 else "head_fused_bf<fp16>"}
    return set() if "X6_UNFUSED_HEAD" in sw or p32(w[0]) not in (32, 64) else {"head_x6"}


# ---------------------------------------------------------------------------------------------- nets
def build_net(c, seed=7):
    """(net on the CPU, its seeded synth state dict) of a Config.  The plan switches are read from the environment when the
    net is created: the caller sets ESAHRNET_<switch> first (monkeypatch.setenv)."""
    import importlib
    from esa_pose_estimation_amd import config, synth
    mod = importlib.import_module(f"esa_pose_estimation_amd.{c.variant}")
    net = mod.get_seg_model(config.make_config(widths=c.widths), precision=PRECISION_NAME[c.precision], num_keypoints=c.K)
    sd = synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=seed)
    return net, sd


def oracle_cfg(c):
    from oracle import hrnet_ref
    return hrnet_ref.default_cfg(CIN[c.variant], c.K, widths=c.widths, variant=VARIANT[c.variant])


def crops(c, shape, seed=7):
    from esa_pose_estimation_amd import synth
    h, w, n = shape
    return synth.make_crops(n, CIN[c.variant], h, w, seed=seed)
