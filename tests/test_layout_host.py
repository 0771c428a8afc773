"""Host side of tests/test_gpu_layout.py (no GPU): the integer statements of tests/layout_ref.py against torch's conversions and
the emulators every other operator test rests on, the conditions on the inputs (asserted on the float64 reference alone), the
facts of the case tables, the refusals of the three test entries and their declarations.

Where the statements and the emulators differ — on non-finite inputs only, class by class (DIFFERENCES below):
  bf16 of a NaN     the statement quiets the NaN and keeps its sign and upper payload (0xffa00000 -> 0xffe0); torch's
                    .to(bfloat16) returns one NaN, 0x7fc0, for all of them.  Both are NaN: one class under layout_ref.same_*.
  split of a NaN    (NaN, NaN) in both; the join is a NaN in both (the payload is the adder's).
  fp16 of a NaN     fp16_emu.q16 keeps the NaN (torch.clamp propagates it); the statement follows the device's store,
                    layout_ref.F16_NAN_STORE = +65504 for a NaN of either sign.
On +-inf and on every finite input, 0x7f7f8000 and above included, they agree bit for bit.
kernels.h's host_f16 is not held here: the library exports no way to reach it."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_emu  # noqa: E402
import layout_ref as LR  # noqa: E402
import resample_ref as RR  # noqa: E402
from oracle import emulate_bf16 as EB  # noqa: E402
from oracle import emulate_split_bf16 as ES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIFFERENCES = ("bf16 of a NaN: payload", "join of a split NaN: payload", "fp16 of a NaN: +65504 against NaN")


@pytest.fixture(scope="module")
def lib():
    from esa_pose_estimation_amd import _lib
    return _lib.lib()


def _t(u):
    return torch.from_numpy(LR.f32(u).copy())


# ---------------------------------------------------------------------------------------------- statements against torch
def test_value_table_holds_every_class():
    u = LR.VALUES
    assert len(u) >= 4096 + 100 and u.dtype == np.uint32
    for name, pred in LR.VALUE_CLASSES.items():
        assert int(pred(u[:len(u) - 4096]).sum()) >= 1, name                  # in the hand-written part, not by luck
    for v in (0x00008000, 0x3F7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x477FE000, 0x477FEFFF, 0x477FF000, 0x501502F9, 0x33000000,
              0x33000001, 0x00000001, 0x007FFFFF, 0x80000000):
        assert v in u, hex(v)
    t = LR.values_tensor()
    assert t.shape == (1, 8, 1, len(u))
    for c in range(8):                                                        # every value at every lane position of a group
        assert np.array_equal(np.sort(t[0, c, 0]), np.sort(u))


def test_bf16_statement_is_torchs():
    u = LR.VALUES
    fin = ~LR.is_nan32(u)
    want = _t(u).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).astype(np.uint32)
    got = LR.bf16_bits(u)
    assert np.array_equal(got[fin], want[fin])                                # +-inf and the carry into inf included
    assert LR.is_nan_bf(got[~fin]).all() and LR.is_nan_bf(want[~fin]).all()   # DIFFERENCES[0]
    assert np.array_equal(LR.q_bf_bits(u)[fin], LR.bits(EB.q(_t(u)))[fin])
    assert np.array_equal(LR.q_bf_bits(u)[fin], LR.bits(RR.q_bf(_t(u)))[fin])
    # hand-checked: ties to even, the carry into the exponent and into inf, the tie below the smallest subnormal
    for v, h in ((0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3F807FFF, 0x3F80), (0x3F808001, 0x3F81), (0x3F7FFFFF, 0x3F80),
                 (0x7F7F7FFF, 0x7F7F), (0x7F7F8000, 0x7F80), (0x00008000, 0x0000), (0x00008001, 0x0001), (0x00018000, 0x0002),
                 (0x007FFFFF, 0x0080), (0x7F800001, 0x7FC0), (0xFFA00000, 0xFFE0)):
        assert int(LR.bf16_bits(np.array([v], dtype=np.uint32))[0]) == h, hex(v)


def test_split_statement_is_the_emulators():
    u = LR.VALUES
    t = _t(u)
    hi, lo = LR.split_bits(u)
    thi, tlo = ES.split(t)
    ok = ~LR.is_nan32(u)
    assert np.array_equal(LR.bf16_to_f32_bits(hi)[ok], LR.bits(thi)[ok])
    assert LR.same_f32(LR.bf16_to_f32_bits(lo), LR.bits(tlo))[ok].all()       # (inf - inf: a NaN in both)
    finite_join = ok & ((u & 0x7FFFFFFF) < 0x7F7F8000)
    for q in (ES.rq, RR.q_sb):
        got = LR.bits(q(t))
        assert np.array_equal(LR.q_sb_bits(u)[finite_join], got[finite_join])
        assert LR.same_f32(LR.q_sb_bits(u), got).all()                        # DIFFERENCES[1]
    # +-inf and every finite |v| from 0x7f7f8000 up join to NaN: hi is inf, the residual the opposite inf (or inf - inf)
    beyond = (u & 0x7FFFFFFF) >= 0x7F7F8000
    assert LR.is_nan32(LR.q_sb_bits(u)[beyond]).all() and not LR.is_nan32(LR.q_sb_bits(u)[~beyond]).any()
    assert int(beyond.sum()) >= 10
    # the join of a split is within 2^-16 of the value (16 significand bits), and exact for 16-bit significands
    with np.errstate(invalid="ignore"):
        rel = np.abs(LR.f32(LR.q_sb_bits(u)).astype(np.float64) - LR.f32(u).astype(np.float64))
    normal = finite_join & ((u & 0x7FFFFFFF) >= 0x08000000)           # (below 2^-111 the lo part runs into bf16 subnormals)
    assert (rel[normal] <= np.abs(LR.f32(u[normal]).astype(np.float64)) * 2.0 ** -16).all()
    # hand-checked: a residual that is itself a tie goes to even
    for v, (h, l) in ((0x3F804040, (0x3F80, 0x3B00)), (0x3F8040C0, (0x3F80, 0x3B02)), (0x3F80BFC0, (0x3F81, 0xBB00)),
                      (0x007FFFFF, (0x0080, 0x8000)), (0x7F7F8000, (0x7F80, 0xFF80))):
        hh, ll = LR.split_bits(np.array([v], dtype=np.uint32))
        assert (int(hh[0]), int(ll[0])) == (h, l), hex(v)


def test_fp16_statement_is_torchs():
    u = LR.VALUES
    t = _t(u)
    fin = ~LR.is_nan32(u)
    want = t.to(torch.float16).view(torch.int16).numpy().view(np.uint16).astype(np.uint32)
    assert np.array_equal(LR.f16_bits(u)[fin], want[fin])                     # unsaturated: subnormals, ties, the carry into inf
    assert LR.is_nan_f16(LR.f16_bits(u)[~fin]).all()
    assert np.array_equal(LR.q_hf_bits(u)[fin], LR.bits(fp16_emu.q16(t))[fin])           # saturated: +-inf -> +-65504
    assert (LR.sat16_bits(u)[~fin] == LR.F16_NAN_STORE).all() and torch.isnan(fp16_emu.q16(t))[torch.from_numpy(~fin)].all()   # DIFFERENCES[2]
    # every binary16 pattern back to f32: torch's conversion, bit for bit on the numbers
    h = np.arange(1 << 16, dtype=np.uint32)
    back = torch.from_numpy(h.astype(np.uint16).view(np.int16)).view(torch.float16).float()
    num = ~LR.is_nan_f16(h)
    assert np.array_equal(LR.f16_to_f32_bits(h)[num], LR.bits(back)[num]) and LR.is_nan32(LR.f16_to_f32_bits(h)[~num]).all()
    assert np.array_equal(LR.f16_bits(LR.f16_to_f32_bits(h))[num], h[num])               # and the round trip is the identity
    for v, b in ((0x477FE000, 0x7BFF), (0x477FEFFF, 0x7BFF), (0x477FF000, 0x7BFF), (0x501502F9, 0x7BFF), (0xFF800000, 0xFBFF),
                 (0x33000000, 0x0000), (0x33000001, 0x0001), (0x33C00000, 0x0002), (0x34200000, 0x0002), (0x387FE000, 0x0400),
                 (0x387FFFFF, 0x0400), (0x3F801000, 0x3C00), (0x3F803000, 0x3C02), (0x3F7FF000, 0x3C00), (0x00000001, 0x0000),
                 (0x7FC00000, LR.F16_NAN_STORE), (0xFFC00000, LR.F16_NAN_STORE), (0x7F800001, LR.F16_NAN_STORE)):
        assert int(LR.sat16_bits(np.array([v], dtype=np.uint32))[0]) == b, hex(v)
    assert int(LR.f16_bits(np.array([0x477FF000], dtype=np.uint32))[0]) == 0x7C00


def test_pack_and_unpack_are_the_documented_layouts():
    x = LR.layout_x((2, 9, 4, 7))
    n, c, h, w = x.shape
    for p in (0, 1, 2, 3):
        cp = LR.layout_cps(c, p)[0]
        raw = LR.pack(x, p, cp)
        assert raw.nbytes == n * h * w * cp * LR.elem_bytes(p)
        back = LR.unpack(raw, p, n, c, h, w, cp)
        assert np.array_equal(back, LR.QBITS[p](x))
        assert np.array_equal(LR.bits(LR.Q[p](torch.from_numpy(LR.f32(x).copy()))), back)         # the suite's rounding of the format
    raw = LR.pack(x, 0, 32)                                                   # SB by hand: pixel (1, 2, 3), channel 8 -> group 1, lane 0
    hi, lo = LR.split_bits(x[1, 8, 2, 3:4])
    px = raw.reshape(n, h, w, 64)[1, 2, 3]                                    # 4 groups of [hi x 8 | lo x 8]
    assert (px[16], px[24]) == (hi[0], lo[0]) and not px[17:24].any() and not px[25:].any()
    hi, lo = LR.split_bits(x[1, 3, 2, 3:4])
    assert (px[3], px[8 + 3]) == (hi[0], lo[0])


# ---------------------------------------------------------------------------------------------- A. conditions on the stem's inputs
def test_stem_table_holds_every_class():
    seen = {(LR.stem_kernel_name(c[3], c[6]), c[6], c[3]) for c in LR.STEM_CASES}
    for p in (0, 1, 2, 3):
        for cin in (1, 2, 3, 4):                                              # every (kernel instantiation x format x cin class)
            assert (LR.stem_kernel_name(cin, p), p, cin) in seen
        for s in LR.STEM_SHAPES:                                              # stem1_body at every shape in every format
            assert any(c[:3] == s and c[3] == 1 and c[6] == p for c in LR.STEM_CASES)
        assert {c[4] for c in LR.STEM_CASES if c[6] == p} == set(LR.STEM_COUTS[p])
        assert {c[5] for c in LR.STEM_CASES if c[6] == p} == {0, 1}
    for s in LR.STEM_SHAPES:                                                  # stem_kernel at every shape too
        assert any(c[:3] == s and c[3] > 1 for c in LR.STEM_CASES)
    ws = sorted({s[2] for s in LR.STEM_SHAPES})
    assert any(w < LR.STEM_PX for w in ws) and LR.STEM_PX in ws and LR.STEM_PX + 1 in ws and any(w > 2 * LR.STEM_PX and w % LR.STEM_PX for w in ws)
    assert any(s[1] == 1 for s in LR.STEM_SHAPES) and any(s[0] == 3 for s in LR.STEM_SHAPES)
    assert any((c[0] * c[1] * c[2] * (c[4] // 8)) % 256 for c in LR.STEM_CASES)          # a thread count that is no multiple of 256
    assert all(c[4] % 64 == 0 for c in LR.STEM_CASES if c[6] in (1, 3))


@pytest.mark.parametrize("case", LR.STEM_CASES, ids=LR.stem_id)
def test_stem_inputs_meet_their_conditions(case):
    n, h, w, cin, cout, relu, p = case
    d = LR.stem_data(case, "signed")
    assert torch.equal(LR.Q[p](d["emu"]), d["emu"])                           # the emulation's outputs are data of their format
    if relu:                                                                  # ReLU cuts: neither inert nor everything
        frac = (d["ref"] > 0).double().mean().item()
        assert 0.25 <= frac <= 0.75, frac
    e = LR.stem_data(case, "edge")
    assert e["x"].min().item() >= 0.5 and e["w"].min().item() >= 0 and bool((e["b"] == 1).all())
    assert torch.equal(LR.Q[p](e["emu"]), e["emu"])
    # replicate padding instead of zero padding moves every border pixel, every channel of it, by more than EDGE_BOUNDS bounds
    bound, e_emu, scale = LR.stem_bound(e, p)
    moved = (LR.stem_ref(e["x"], e["w"], e["b"], relu, replicate=True) - e["ref"]).abs()
    m = LR.border_mask(h, w)
    assert moved[:, :, ~m].max().item() == 0 if (~m).any() else True          # and no interior pixel
    assert moved[:, :, m].min().item() > EDGE_BOUNDS[p] * bound, (moved[:, :, m].min().item() / bound, bound, e_emu, scale)


# Bounds by which the edge regime's border pixels move under replicate padding.  100 where the format allows it.  A bf16 bound is
# 2^-9 of the tensor's scale plus 2 E_emu of up to the same size each, so 100 of them are 0.2 .. 0.6 of the largest output, and a
# border pixel's out-of-image taps are 3 of 9 (5 of 9 at a corner) of a sum whose inputs span [0.5, 1.5]: no input reaches that.
# There 10 bounds are asserted (the table's smallest is 13): a kernel within one bound of the reference is nine away from the
# replicate-padded one at every border pixel.  In the signed regime ReLU is live; in the edge regime every output is >= 1.
EDGE_BOUNDS = {0: 100.0, 1: 10.0, 2: 100.0, 3: 100.0}


@pytest.mark.parametrize("case,a", LR.STEM_SAT_CASES, ids=lambda v: LR.stem_id(v) if isinstance(v, tuple) else f"a{v}")
def test_saturation_cases_leave_the_range_on_both_sides(case, a):
    d = LR.stem_data(case, "signed", a, 0)
    ref = d["ref"]
    assert int((ref > LR.F16_MAX).sum()) >= 8 and int((ref < -LR.F16_MAX).sum()) >= 8
    left_out = (ref.abs() > LR.F16_MAX * (1 - 2.0 ** -10)).double().mean().item()
    assert 0 < left_out <= 0.10, left_out


# ---------------------------------------------------------------------------------------------- B, C. case-table facts
def test_layout_table_holds_every_class():
    cs = [s[1] for s in LR.LAYOUT_SHAPES]
    assert 1 in cs and any(c < 8 for c in cs) and any(c % 8 == 1 for c in cs) and 32 in cs and 33 in cs and 65 in cs
    assert LR.layout_cps(7, 0) == [32, 64, 8] and LR.layout_cps(7, 1) == [64, 128] and LR.layout_cps(33, 2) == [64, 96, 40]
    assert LR.layout_cps(32, 0) == [32, 64] and LR.layout_cps(65, 3) == [128, 192]
    hi, lo = LR.sb_decode_pairs()
    assert len(hi) == len(lo) == len(LR.BF_SPECIAL) ** 2 + 4096
    big_lo = (lo & 0x7FFF) >= (hi & 0x7FFF)
    assert big_lo.sum() > 100 and LR.is_nan_bf(hi).any() and LR.is_nan_bf(lo).any() and ((hi & 0x7FFF) == 0x7F80).any()


def test_tile_table_holds_every_class():
    hws = {c[0] * c[1] for c in LR.TILE_CASES}
    assert hws == {1, 63, 64, 255, 256, 257, 612, 1030}
    assert {c[2] for c in LR.TILE_CASES} == {1, 7, 8, 11, 30, 32}
    assert {c[3] for c in LR.TILE_CASES} == {32, 64} and {c[4] for c in LR.TILE_CASES} == {1, 3}
    assert 1030 % LR.TILE == 6 and -(-1030 // LR.TILE) == 5
    for case in LR.TILE_CASES:                                                # every pattern reaches every case
        assert {(k + r) % 8 for r in LR.tile_rotations(case) for k in range(case[2] * case[4])} == set(range(8)), case


@pytest.mark.parametrize("case", LR.TILE_CASES, ids=LR.tile_id)
def test_tile_expect_is_argmax_by_brute_force(case):
    h, w, c, cp, n = case
    hw = h * w
    for rot in LR.tile_rotations(case):
        planes = LR.tile_planes(case, rot).reshape(n * c, hw)
        vals, idx = LR.tile_expect(planes)
        assert vals.shape == idx.shape == (n * c, -(-hw // LR.TILE))
        for k in range(n * c):
            v = LR.f32(planes[k])
            for t in range(vals.shape[1]):
                seg = v[t * LR.TILE:(t + 1) * LR.TILE]
                best = 0                                                      # the loop np.argmax stands for
                for i in range(1, len(seg)):
                    if not np.isnan(seg[best]) and (np.isnan(seg[i]) or seg[i] > seg[best]):
                        best = i
                assert best == int(np.argmax(seg))                           # (np.argmax: the first NaN, else the first maximum)
                assert idx[k, t] == t * LR.TILE + best and vals[k, t] == planes[k, t * LR.TILE + best]
            # what each pattern plants is what it says
            name = LR.TILE_PATTERNS[(k + rot) % 8]
            nan = np.isnan(v)
            if name == "random":
                assert len(np.unique(v)) == hw
            elif name == "tile edge" and hw > 1:
                top = np.flatnonzero(v == v.max())
                assert len(top) == 2 and (top[1] - top[0] == 1 and top[1] % LR.TILE == 0 if hw > LR.TILE else (top[0], top[1]) == (0, hw - 1))
            elif name == "constant":
                assert len(np.unique(v)) == 1 and (idx[k] % LR.TILE == 0).all()
            elif name == "nan after max" and hw > 1:
                assert nan.sum() == 1 and nan[hw - 1] and np.nanargmax(v) < (hw - 1) // LR.TILE * LR.TILE + (hw <= LR.TILE) * (hw - 1)
            elif name == "two nans" and hw > 1:
                p, q = np.flatnonzero(nan)
                assert p // LR.TILE == q // LR.TILE and ((q - p) % 64 == 0 or min(hw, LR.TILE) < 65 + p)
            elif name == "all -inf":
                assert (planes[k] == LR.NINF_BITS).all() and (idx[k] % LR.TILE == 0).all()
            elif name == "inf then nan" and hw > 1:
                assert planes[k, 0] == LR.PINF_BITS and nan[hw - 1] and nan.sum() == 1
            elif name == "lanes 63 64" and hw > 64:
                top = np.flatnonzero(v == v.max())
                assert len(top) == 2 and top[1] == top[0] + 1 and (top[0] % LR.TILE == 63 or min(LR.TILE, hw - top[0] // LR.TILE * LR.TILE) <= 64)
        # planted values are data of the split format, specials written literally
        raw = LR.pack(LR.tile_planes(case, rot), 0, cp, literal_specials=True)
        assert np.array_equal(LR.unpack(raw, 0, n, c, h, w, cp), LR.tile_planes(case, rot))
    assert any(LR.TILE_PATTERNS[(k + r) % 8] == "lanes 63 64" for r in LR.tile_rotations(case) for k in range(n * c))


# ---------------------------------------------------------------------------------------------- refusals and declarations
def test_entries_refuse_on_the_host(lib):
    """Every refusal comes before anything is allocated or enqueued: it runs without a device, and the buffers stay as they were."""
    buf = (C.c_float * 4096)(*([7.0] * 4096))
    ptr = C.cast(buf, C.c_void_p)
    nt = C.c_int(-5)
    err = lambda: lib.esahrnet_last_error().decode()  # noqa: E731
    stem = lambda **k: lib.esahrnet_op_stem_ex(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", ptr), ("n", 1), ("cin", 1), ("h", 4), ("w", 4), ("wt", ptr), ("b", ptr), ("cout", 64), ("relu", 0), ("p", 0), ("y", ptr), ("s", None))])
    for bad in (dict(x=None), dict(wt=None), dict(b=None), dict(y=None)):
        assert stem(**bad) != 0 and "null" in err()
    assert stem(cin=0) != 0 and "cin" in err()
    assert stem(cin=5) != 0 and "cin" in err()
    assert stem(cout=48) != 0 and "cout" in err()
    assert stem(cout=0) != 0 and "cout" in err()
    assert stem(cout=32, p=1) != 0 and "64" in err()
    assert stem(cout=32, p=3) != 0 and "64" in err()
    assert stem(p=4) != 0 and "precision" in err()
    assert stem(p=-1) != 0 and "precision" in err()
    assert stem(n=0) != 0 and stem(h=0) != 0 and stem(w=-1) != 0
    lay = lambda **k: lib.esahrnet_op_layout(*[k.get(a, d) for a, d in (  # noqa: E731
        ("dir", 0), ("x", ptr), ("n", 1), ("c", 9), ("h", 4), ("w", 4), ("cp", 32), ("p", 0), ("raw", ptr), ("y", ptr), ("s", None))])
    for bad in (dict(x=None), dict(raw=None), dict(y=None), dict(dir=1, raw=None)):
        assert lay(**bad) != 0 and "null" in err()
    assert lay(dir=2) != 0 and "dir" in err()
    assert lay(p=4) != 0 and "precision" in err()
    assert lay(cp=8) != 0 and "cp" in err()                                   # cp < c
    assert lay(cp=36) != 0 and "cp" in err()                                  # not a multiple of 8
    assert lay(c=0) != 0 and lay(n=0) != 0
    assert lay(raw=C.c_void_p(ptr.value + 4)) != 0 and "aligned" in err()
    tm = lambda **k: lib.esahrnet_op_tile_max(*[k.get(a, d) for a, d in (  # noqa: E731
        ("raw", ptr), ("n", 1), ("c", 11), ("h", 4), ("w", 4), ("cp", 32), ("p", 0), ("store", 1), ("y", ptr), ("part", ptr),
        ("nt", C.byref(nt)), ("kp", None), ("idx", None), ("s", None))])
    for bad in (dict(raw=None), dict(part=None), dict(nt=None), dict(y=None)):
        assert tm(**bad) != 0 and ("null" in err() or "needs y_dev" in err())
    assert tm(p=1) != 0 and "precision" in err()
    assert tm(p=3) != 0 and "precision" in err()
    assert tm(c=33, cp=64) != 0 and "c=33" in err()
    assert tm(c=0) != 0
    assert tm(cp=8) != 0 and "cp" in err()
    assert tm(cp=36) != 0 and "cp" in err()
    assert tm(store=2) != 0 and "store" in err()
    assert tm(h=0) != 0
    assert nt.value == -5 and all(v == 7.0 for v in buf)                      # outputs untouched


def test_entries_are_declared_and_abi_stays():
    from esa_pose_estimation_amd import _lib
    with open(os.path.join(ROOT, "include", "esahrnet.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    names = ("esahrnet_op_stem_ex", "esahrnet_op_layout", "esahrnet_op_tile_max")
    for n in names:
        assert f"int {n}(" in header and n in _lib.exported_symbols() and f"`{n}(" in doc, n
    assert "test use only" in header[header.index("esahrnet_op_stem_ex") - 1400:header.index("esahrnet_op_stem_ex")]
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == _lib.ABI_VERSION     # entries were only added
    pkg = os.path.join(ROOT, "esa-pose-estimation_amd")
    for fn in os.listdir(pkg):                                                # on no forward path: no module of the package but the bindings
        if fn.endswith(".py") and fn != "_lib.py":
            with open(os.path.join(pkg, fn)) as f:
                assert not any(n in f.read() for n in names), fn
    src = {}
    for fn in ("plan.hip", "op_abi.hip", "host_util.h"):
        with open(os.path.join(pkg, "csrc", fn)) as f:
            src[fn] = f.read()
    # one packing: its definition and esahrnet_commit (2) in plan.hip, the three stem entries in op_abi.hip, the declaration they share
    assert [src[fn].count("pack_stem_w(") for fn in src] == [3, 3, 1]
    assert "std::vector<float> esa::pack_stem_w(" in src["plan.hip"] and src["host_util.h"].count("std::vector<float> pack_stem_w(") == 1
    assert sum(s.count("* 9 + t) * 8 + (co & 7)]") for s in src.values()) == 1  # and no copy of it written inline
