"""Host side of the CBAM / pooling-stem tests (no GPU): the step references of tests/cbam_ref.py against the project's oracle,
the self-check that keeps the GPU bounds of tests/test_gpu_cbam.py from being vacuous or loose, the slab geometry against the
constants in the sources, and the conditions on the planted inputs — all on the float64 reference, none on a kernel's output.

M_NEG and the weights (cbam_ref.planted): where every real channel is negative the channel maximum of ca * x is the product
nearest zero, -min_c ca[c] |x[c]|, and a padding channel's zero winning it moves the maximum map by that much.  For y to move
by ten times the bf16 bound (about 3 x 2^-9 of max|y|) that has to be large and the spatial sigmoid on its slope there: the
all-negative pixels hold -(M_NEG + |z|) with M_NEG = 6, fc[2] is small enough that ca stays inside about (0.2, 0.8), the centre
tap on the maximum map is +-0.5 and the one on the mean map -+0.3, so that the two about cancel at such a pixel.  With these
test_clamped_maximum_map_is_far_outside_the_bound finds at least 19 times the bound in every case with C < Cp (it prints each
ratio); with N(0, 0.2) taps, M_NEG = 3 and fc[2] of unit gain the smallest was 0.02.  The residual has mean 0.3 so that the ReLU
stays open at 40 % or more although a fifth of the pixels is far below zero."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cbam_ref as CR  # noqa: E402
from oracle import hrnet_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "esa-pose-estimation_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# the cases without the launch form: the reference does not know it
HOST_CASES = sorted({(c, s, p, rr, slabs) for c, s, p, rr, _, slabs in CR.cbam_cases()})


def _hid(case):
    c, (h, w, n), p, rr, slabs = case
    return f"c{c}-{h}x{w}-{CR.PNAME[p]}-{'res_relu' if rr else 'plain'}" + (f"-P{slabs}" if slabs else "")


def _inputs(case):
    c, (h, w, n), p, rr, slabs = case
    P = CR.slab_rule(h * w, slabs)
    return CR.planted(c, h, w, n, p, P), P


def _chain(case):
    """The float64 reference of every step and the float32 emulation of the same step ON THE SAME INPUTS (the reference's own
    outputs of the step before): what the GPU test does with the device's outputs."""
    d, P = _inputs(case)
    c, (h, w, n), p, rr, slabs = case
    res = d["res"] if rr else None
    r = CR.ref_all(d["x"], res, d["w0"], d["w2"], d["wsa"], rr, P)
    e = dict(ca=CR.emu_ca(r["partial"].float(), h * w, d["w0"], d["w2"]),
             maps=CR.emu_maps(d["x"], r["ca"].float()),
             y=CR.emu_y(d["x"], res, r["ca"].float(), r["maps"].float(), d["wsa"], rr, p))
    return d, P, r, e


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("case", [k for k in HOST_CASES if k[2] == 2 and not k[3] and not k[4]], ids=_hid)
def test_steps_compose_to_the_oracle(case):
    d, P = _inputs(case)
    sd = {"ca.fc.0.weight": d["w0"].double(), "ca.fc.2.weight": d["w2"].double(), "sa.conv1.weight": d["wsa"].double()}
    want = hrnet_ref._cbam(sd, "", d["x"].double())
    for slabs in {P, 1, min(7, d["x"].shape[-1] * d["x"].shape[-2])}:         # the slab count does not change the operation
        got = CR.ref_all(d["x"], None, d["w0"], d["w2"], d["wsa"], False, slabs)["y"]
        assert (got - want).abs().max().item() <= 1e-12


# ---------------------------------------------------------------------------------------------- the bounds are neither vacuous nor loose
@pytest.mark.parametrize("case", HOST_CASES, ids=_hid)
def test_reference_self_check(case):
    d, P, r, e = _chain(case)
    c, (h, w, n), p, rr, slabs = case
    for step, ref, emu in (("ca", r["ca"], e["ca"]), ("mean map", r["maps"][..., 0], e["maps"][..., 0]), ("y", r["y"], e["y"])):
        scale = 1.0 if step == "ca" else ref.abs().max().item()
        err = (emu.double() - ref).abs().max().item()
        assert 0.0 < err, (step, err)
        if p == 2 or step != "y":               # float32 arithmetic: partial, ca and maps in every mode, y in the fp32-grade one
            assert err < 1e-5 * scale, (step, err, scale)
        else:                                   # y stored in the format: half an ulp, at most 2 quanta of the scale
            assert err < 2.0 * CR.QUANTUM[p] * scale + 1e-5 * scale, (step, err, scale)
    assert torch.equal(e["maps"][..., 1].double(), (r["ca"].float()[:, :, None, None] * d["x"]).amax(1).double())
    # the slab sums: a float32 sum in another order stays inside the any-order bound, and the planted values stand out of it
    v = d["x"].double().reshape(n, c, -1)
    ep = CR.emu_partial(d["x"], P)
    for s, (p0, p1) in enumerate(CR.slab_bounds(h * w, P)):
        if p1 <= p0:
            assert bool((r["partial"][:, s, :, 0] == 0).all()) and bool((r["partial"][:, s, :, 1] == -float("inf")).all())
            continue
        b = CR.sum_bound(v, p0, p1)
        assert bool(((ep[:, s, :, 0].double() - r["partial"][:, s, :, 0]).abs() <= b).all())
        assert torch.equal(ep[:, s, :, 1].double(), r["partial"][:, s, :, 1])
        inside = (d["where"] >= p0) & (d["where"] < p1)
        planted = v.gather(2, d["where"][:, :, None])[:, :, 0].abs()
        assert bool((planted[inside] > 4.0 * b[inside]).all()), (s, planted[inside].min().item(), b[inside].max().item())


# ---------------------------------------------------------------------------------------------- geometry against the sources
def test_slab_geometry_and_case_table():
    plan, cbam, stem = _src("host_util.h"), _src("cbam.hip"), _src("stem.hip")     # (host_util.h: what plan.hip and op_abi.hip share)
    pool_slabs = int(re.search(r"static constexpr int POOL_SLABS = (\d+);", plan).group(1))
    stem_px = int(re.search(r"constexpr int STEM_PX = (\d+);", stem).group(1))
    stem_max = int(re.search(r"constexpr int STEM_POOL_SLABS_MAX = (\d+);", plan).group(1))
    th, tw = (int(v) for v in re.search(r"constexpr int CS_TH = (\d+), CS_TW = (\d+)", cbam).groups())
    assert CR.slab_rule(10 ** 6, 0) == pool_slabs == 64 and CR.stem_piece(stem_px) == 256 == CR.stem_piece()
    assert "const int S = (HW + P - 1) / P;" in cbam and "const int p0 = slab * S, p1 = min(HW, p0 + S);" in cbam
    assert "slab = (size_t)y * gridDim.x + blockIdx.x" in stem
    assert re.search(r"Cp > 512 \|\| Cr > 64", cbam)                      # ca_mlp's limit: c = 512 is the last one served

    def geo(h, w):
        P = CR.slab_rule(h * w, 0, pool_slabs)
        return P, -(-h * w // P), CR.last_slab(h * w, P), CR.slab_bounds(h * w, P)
    shapes = {(h, w): n for h, w, n in CR.SHAPES}
    assert geo(1, 1)[0] == 1 and shapes[(1, 1)] == 2
    assert 2 * 3 < 8 and max(2, 3) < 7 and (2, 3) in shapes                  # ca_mlp's tail loop alone; smaller than the window
    assert geo(4, 4)[0] == 16 and (4, 4) in shapes                            # two full 8-slab steps
    assert 7 * 9 == 63 == geo(7, 9)[0] and (7, 9) in shapes                   # P = HW below 64; window as high as the image
    P, S, L, b = geo(5, 13)
    assert (P, S, L) == (64, 2, 32) and all(p1 <= p0 for p0, p1 in b[33:]) and (5, 13) in shapes
    assert (16, 32) == (th, tw) and (16, 32) in shapes                        # exactly one cbam_spatial tile
    P, S, L, b = geo(17, 33)
    assert 17 == th + 1 and 33 == tw + 1 and L == 62 and 0 < b[62][1] - b[62][0] < S and b[63][1] <= b[63][0]
    assert shapes[(40, 36)] == 3
    for c in CR.EVERY_SHAPE_C:                                                # blocks of cbam_maps / cbam_apply straddle images
        if (40 * 36) % (256 // (CR.pad(c, 0) // 8)):
            break
    else:
        raise AssertionError("no channel count whose blocks straddle images at 40x36")
    assert 16 // 16 == 1 and CR.pad(16, 0) == 32 and CR.pad(16, 1) == 64      # Cr = 1; half / three quarters padding
    assert 24 % 16 and {32, 48, 64, 96, 128, 256} <= set(CR.ALL_C)
    assert CR.pad(264, 0) // 8 == 36 and 256 // 36 == 7 and 256 - 7 * 36 > 0      # 33 groups hold channels, 36 with the padding: 7 pixels a block, idle threads
    assert CR.pad(384, 0) // 8 == 48 < 49 and CR.pad(400, 0) // 8 == 52 > 49
    assert CR.pad(512, 0) // 8 == 64 and 512 // 16 == 32 and max(CR.ALL_C) == 512 and CR.pad(CR.C_REFUSED, 0) > 512
    cases = CR.cbam_cases()
    seen = {(c, s, p, rr, f) for c, s, p, rr, f, P in cases if not P}
    for p in (0, 1, 2):
        for rr in (False, True):
            assert all((c, s, p, rr, 0) in seen for c in CR.ALL_C for s in CR.EVERY_C_SHAPES)
            assert all((c, s, p, rr, 0) in seen for c in CR.EVERY_SHAPE_C for s in CR.SHAPES)
            for s in CR.FUSED_SHAPES:
                for c in (CR.ALL_C if s in CR.EVERY_C_SHAPES else CR.EVERY_SHAPE_C):
                    assert ((c, s, p, rr, 1) in seen) == CR.spatial_supported(CR.pad(c, p))
    assert {P for c, s, p, rr, f, P in cases if P and s == (17, 33, 2)} == {1, 7, 8, 9, 63}
    for (h, w), P in (((24, 32), 768), ((32, 32), 1024)):                     # the pooling stem's slab counts: one pixel a slab
        assert (64, (h, w, 2), P) in CR.SLAB_CASES and h * w == P <= stem_max and -(-h * w // P) == 1
    # the stem: slabs_out restated, and what each shape is there for
    for h, w in CR.STEM_SHAPES:
        assert CR.stem_slabs(h, w, stem_px) == h * -(-w // 256) == h * len(CR.stem_pieces(w))
    assert 21 % stem_px and 256 % stem_px == 0 and len(CR.stem_pieces(256)) == 1
    assert CR.stem_pieces(264) == [(0, 256), (256, 264)] and 264 - 256 == stem_px


# ---------------------------------------------------------------------------------------------- conditions on the inputs
@pytest.mark.parametrize("case", [k for k in HOST_CASES if not k[3]], ids=_hid)
def test_planted_inputs(case):
    d, P = _inputs(case)
    c, (h, w, n), p, rr, slabs = case
    hw = h * w
    x = d["x"]
    assert torch.equal(CR.Q[p](x), x) and torch.equal(CR.Q[p](d["res"]), d["res"])          # numbers of the format
    v = x.double().reshape(n, c, hw)
    imgs = [0] if hw == 1 else list(range(n))
    # (a) the planted pixel is the channel's strict maximum; every position class is occupied
    pos = CR.positions(h, w, P)
    assert set(pos) >= set(CR.POSITION_CLASSES) - {"first of slab 1"} and ("first of slab 1" in pos) == (P > 1)
    for i in imgs:
        top = v[i].argmax(1)
        assert torch.equal(top, d["where"][i])
        val = v[i].gather(1, top[:, None])[:, 0]
        neg = CR.neg_channels(c, i)
        assert bool((val[[k for k in range(c) if k not in neg]] > 5.0).all())
        assert set(top.tolist()) == set(pos.values())
        # without its planted pixel the slab's maximum is another (or the slab is empty)
        S = -(-hw // P)
        cut = v[i].clone()
        cut.scatter_(1, top[:, None], -float("inf"))
        for ch in range(c):
            s = int(top[ch]) // S
            assert cut[ch, s * S:min(hw, s * S + S)].max().item() < val[ch].item()
        # (c) negative everywhere
        assert len(neg) >= (2 if c > 2 else 1) and bool((v[i][neg] < 0).all())
    # (b) all-negative pixels: at least 10 % (at least one where HW < 10); a one-pixel image cannot hold (a) and (b) both
    allneg = (v < 0).all(1)
    for i in range(n):
        k = int(allneg[i].sum())
        assert torch.equal(allneg[i] & d["negpix"][i], d["negpix"][i])
        if hw == 1:
            assert k == (1 if i > 0 else 0)
        else:
            assert k >= max(1, -(-hw // 10) if hw >= 10 else 1), (i, k, hw)


CLAMP_CASES = [k for k in HOST_CASES if k[0] < CR.pad(k[0], k[2])]


@pytest.mark.parametrize("case", CLAMP_CASES, ids=_hid)
def test_clamped_maximum_map_is_far_outside_the_bound(case):
    """C < Cp: a padding channel's zero winning the maximum must move y by at least ten times the case's bound."""
    d, P, r, e = _chain(case)
    c, (h, w, n), p, rr, slabs = case
    bound, e_emu, scale = CR.bound(r["y"], e["y"], CR.QUANTUM[p])
    bad = CR.ref_all(d["x"], d["res"] if rr else None, d["w0"], d["w2"], d["wsa"], rr, P, clamp_max_at_zero=True)["y"]
    moved = (bad - r["y"]).abs().max().item()
    print(f"{_hid(case)}: clamped maximum map moves y by {moved:.3e} = {moved / bound:.1f} x bound ({bound:.3e})")
    assert moved >= 10.0 * bound, (moved, bound)


@pytest.mark.parametrize("case", [k for k in HOST_CASES if k[3]], ids=_hid)
def test_relu_is_open_often_enough(case):
    d, P = _inputs(case)
    pre = CR.ref_all(d["x"], d["res"], d["w0"], d["w2"], d["wsa"], False, P)["y"]
    frac = (pre > 0).double().mean().item()
    assert frac >= 0.40, frac


def test_every_shape_class_also_runs_without_relu():
    cases = CR.cbam_cases()
    for c, s in {(c, s) for c, s, *_ in cases if not _[-1]}:
        assert {rr for cc, ss, p, rr, f, P in cases if (cc, ss) == (c, s) and not P} == {False, True}


# ---------------------------------------------------------------------------------------------- the stem
@pytest.mark.parametrize("hw", CR.STEM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stem_reference_self_check(hw):
    h, w = hw
    d = CR.stem_inputs(h, w)
    for relu in (0, 1):
        ref = CR.ref_stem(d["x"], d["w"], d["b"], relu)
        scale = ref.abs().max().item()
        for p in (0, 1, 2):
            err = (CR.emu_stem(d["x"], d["w"], d["b"], relu, p).double() - ref).abs().max().item()
            assert 0.0 < err < (1e-5 if p == 2 else 2.0 * CR.QUANTUM[p] + 1e-5) * scale, (p, relu, err, scale)
        if relu:
            assert (ref > 0).double().mean().item() >= 0.40


def test_stem_maxima_fall_on_every_position_class():
    """On the reference: over the stem cases, some channel's slab maximum lies on the piece's first pixel, its last pixel, the
    row's last pixel in a partial piece, the first pixel of a second piece, both sides of an 8-pixel group's border and in a
    partial last group."""
    hit = set()
    for h, w in CR.STEM_SHAPES:
        d = CR.stem_inputs(h, w)
        ref = CR.ref_stem(d["x"], d["w"], d["b"], 0)
        for k, (p0, p1) in enumerate(CR.stem_pieces(w)):
            at = ref[:, :, :, p0:p1].argmax(-1).flatten().tolist()
            for a in set(at):
                x = p0 + a
                hit |= {name for name, ok in (("piece first", a == 0), ("piece last of 256", a == 255), ("row last, partial piece", x == w - 1 and (p1 - p0) < 256),
                                              ("second piece first", k == 1 and a == 0), ("group last", x % 8 == 7), ("group first", x % 8 == 0 and a > 0),
                                              ("partial last group", w % 8 != 0 and x >= w - w % 8)) if ok}
    assert hit == {"piece first", "piece last of 256", "row last, partial piece", "second piece first", "group last", "group first",
                   "partial last group"}, hit


def test_hooks_are_declared_and_abi_stays():
    from esa_pose_estimation_amd import _lib
    with open(os.path.join(ROOT, "include", "esahrnet.h")) as f:
        header = f.read()
    assert "int esahrnet_op_cbam_steps(" in header and "int esahrnet_op_stem(" in header
    assert "row * pieces + piece" in header                                   # the slab layout stem.hip documents
    assert {"esahrnet_op_cbam_steps", "esahrnet_op_stem"} <= set(_lib.exported_symbols())
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == _lib.ABI_VERSION     # entries were only added
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "esahrnet_op_cbam_steps(" in doc and "esahrnet_op_stem(" in doc
