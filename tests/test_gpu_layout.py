"""The boundary between the caller's f32 NCHW tensors and the internal formats, each piece on its own: stem.hip's conv1 outside
esahrnet_op_stem's one configuration, layout.hip's conversions (the measuring instrument of every other operator test, and what
esahrnet_tap_read is built on) and the tile-maximum kernels with their NHWC finish — through the test-only entries
esahrnet_op_stem_ex, esahrnet_op_layout and esahrnet_op_tile_max.  References, integer statements of the roundings, byte layouts,
the value table and the case tables: tests/layout_ref.py; what holds those: tests/test_layout_host.py.  Every device buffer a
test hands in lies between two 256-byte guard bands, prefilled with 0xa5 and asserted untouched; a failed library call of a valid
case ends the session.

A. Stem.  The rule of the other operator modules, taken against the reference only:
       |HIP - f64|_max <= 2 x E_emu + q x max|ref|,     E_emu = max |torch f32 conv2d + bias (+ ReLU), rounded to the format - f64|
   q = conv_ref.QUANTUM[precision]; the reference is F.conv2d in float64 of the raw f32 crop (the stem reads it as it is).
     shapes (n, h, w)   (1,1,1) one thread's worth; (1,3,7) a row shorter than STEM_PX = 8: stem1_body's tail in the only x-group;
                        (2,5,8) exactly one group; (3,2,9) one pixel into the second group, three images (the per-image base);
                        (2,3,17), (1,4,33) several groups and a tail of one; (2,1,40) H = 1, no tail.  Thread counts that are no
                        multiple of 256 throughout.
     table              cin 1 (stem1_kernel<false>, stem1_hf_kernel) at every shape in every precision; cin 2, 3, 4 (stem_kernel
                        <false> / <true>, weights in LDS) at two shapes each per precision, all seven over the table; cout 32, 64,
                        96, 128 (64, 128 in the 16-bit formats); ReLU alternating; regimes "signed" and "edge" (x >= 0.5, weights
                        > 0, bias +1: replicate padding instead of zero padding moves every border output by > 100 bounds, > 10 in
                        bf16 — test_layout_host.py says why 100 cannot be had there)
     formats            one f32 accumulation, four stores: SB == split(F32 output), BF == bf16(F32 output), HF == sat16(F32
                        output) bit for bit by the integer statements, in stem1_body and in stem_kernel
     order              stem.hip's "same order as stem_kernel": cin 1 equals cin 2 with the second channel's weights zero, by value,
                        in every format, at shapes with and without a row tail
     entries            esahrnet_op_stem == esahrnet_op_stem_ex at cin 1, cout 64, bit for bit (one packing function)
     scaling            y(2^a x, 2^b w, 2^(a+b) bias) == 2^(a+b) y bit for bit at (12, -7), (-12, 7), precisions 0, 1, 2
     fp16 saturation    x scaled by 2^15: >= 8 reference outputs beyond +-65504 on either side come out as exactly +-65504 with the
                        reference's sign; the rule on the elements with |ref| <= 65504 (1 - 2^-10) (>= 90 % of the case)
B. Conversions.  (n, c, h, w) = (1,1,1,1), (3,7,3,5) less than a group, (2,9,4,7) one past a group, (2,32,8,8) a whole padding
   unit, (2,33,5,3) one past it, (1,65,2,9) one past 64; cp = the format's padding, one unit more, and (SB, F32) 8 ceil(c / 8).
     dir 0              N(0, 1) data: raw_dev is the host packer's bytes exactly (SB [pixel][c8][hi|lo][8]; padding channels +0 in
                        both parts; every byte written), y the host decode of those bytes
     value table        layout_ref.VALUES through every lane position of a group, in all four formats: ties and carries into the
                        exponent, f32 and fp16 subnormals, the fp16 boundary 65504 / 65520, |v| >= 0x7f7f8000 (split: NaN), +-inf,
                        quiet and signalling NaNs, 4096 random patterns — raw bytes and y are the integer statements'
     dir 1              bytes no split produces (every special bf16 pattern against every other as (hi, lo), 4096 random pairs)
                        decode to bf16(hi) + bf16(lo), one f32 addition; all 65536 bf16 and fp16 patterns decode to the statement;
                        the f32 format is a copy; padding lanes and groups hold 0xa5 and are not read
C. Tile maxima.  h x w = 1x1, 7x9 (63), 8x8 (64: one lane step), 15x17 (255), 16x16 (256), 1x257 (one pixel in the second tile),
   34x18 (612: a tail of 100), 10x103 (1030: five tiles, the last of 6 pixels); c = 1, 7, 8, 11, 30, 32; cp 32 and once 64 (groups
   past the ones read, filled with 0xa5); n = 1 and 3; precisions 0 and 2; store 0 and 1.  Planes cycle through eight planted
   patterns (layout_ref.TILE_PATTERNS; cases with fewer than 8 planes run once per rotation): distinct values; the maximum at a
   tile's last pixel and the next tile's first; constant; a NaN in the last tile behind a larger number; two NaNs 64 k pixels apart
   in one tile; all -inf; +inf then a NaN; equal maxima at pixels 63 and 64.  Every part[plane][tile] equals tile_expect's (value
   bits, index); store 1: y is the format-held values; store 0: y's buffer untouched; esahrnet_keypoints_finish(y, part) ==
   esahrnet_keypoints_ex(y) == the NHWC finish through the entry, kp and idx bit for bit, and idx is the plane's np.argmax.
Refusals: each entry with device pointers — non-zero, a message, 0xa5-filled outputs untouched, a good call afterwards.

Measured on an MI355X: 275 cases (276 tests) in 0.5 s of case time, 2.7 s for the module; the slowest case 0.09 s (the first:
the library's load).  Worst error / bound per stem kernel and precision, with the HIP error and E_emu of that case:
  stem1_kernel<false>   split-bf16 0.325 (3.059e-5, 3.044e-5; n2 5x8 cin 1 cout 96 edge)   bf16 0.393 (1.516e-2, 1.516e-2; n2 3x17
                        cout 128 relu edge)   fp32 0.357 (6.939e-7, 4.460e-7; n2 5x8 cout 32 edge)
  stem1_hf_kernel       fp16 0.394 (1.919e-3, 1.919e-3; n2 3x17 cout 128 relu edge)
  stem_kernel<false>    split-bf16 0.306 (3.093e-5, 3.092e-5; n2 3x17 cin 2 cout 96 edge)   bf16 0.392 (1.555e-2, 1.555e-2; n3 2x9
                        cin 3 cout 64 relu edge)   fp32 0.469 (2.196e-6, 1.549e-6; n1 3x7 cin 4 cout 64 relu edge)
  stem_kernel<true>     fp16 0.385 (9.660e-4, 9.660e-4; n3 2x9 cin 4 cout 64 relu signed)
In the stored formats kernel and emulation round to the same value at the worst element (error == E_emu); the f32 format shows
the order of the 9 cin fmaf steps against torch's (error up to 1.56 E_emu).  No form needed a factor above the rule's 2 (FACTOR
is empty).  Every exact check held at the first run, the source's "same order as stem_kernel" included.  No defect was found in
the kernels; launch_stem now refuses a bf16 cout that is no multiple of 64 (it checked fp16 only; sb.h defines both layouts in
64-channel blocks); esahrnet_op_stem_ex refuses such a cout before it reaches the launcher (test_layout_host.py).
The two classes nobody had measured (layout_ref.F16_NAN_STORE, layout_ref.SUBNORMALS; DESIGN.md 3a / 3c, sb.h):
  fp16 NaN      pack2_f16 stores +65504 for a NaN of either sign, quiet or signalling, in layout.hip and in both fp16 stem
                stores' shared path — the packed min returns the operand that is a number.  fp16_emu.q16 keeps the NaN: its
                docstring now says so.
  subnormals    kept everywhere: f32-subnormal inputs are read as they are, bf16- and fp16-subnormal results are stored, the
                split's subtraction and the join's addition flush nothing; the device's bytes equal the IEEE statement on every
                entry of the table.  NaN payloads too came out as the statement's (quieted, sign and upper payload kept), though
                the comparisons take all NaNs of a format as one value.

Teeth, each checked once on a scratch build with one arithmetic mutation that widens no index range, this module and the rest of
the GPU suite (2362 tests) run against it:
  1. ESA_HF_NOCLAMP=1 (pack2_f16 without its saturation): both test_stem_fp16_saturation cases fail (0x7c00 where 65504 is
     due) and test_conversion_of_the_value_table[fp16] (14640 raw elements); nothing else in the module moves.  7 existing tests
     noticed: test_gpu_fp16.py's three test_op_conv_fp16_saturates_at_65504 cases and test_op_fuse_fp16_saturates,
     test_gpu_resample.py::test_fuse_fp16_saturates_on_the_chain, test_gpu_stats.py::test_saturation_is_visible and
     test_a_nonfinite_input_is_located[hrnet2-fp16].
  2. stem1_body reading the clamped in-image sample where it puts the out-of-image zero: all 56 cin-1 cases of test_stem fail at
     the rule, both regimes (errors of 3 .. 4 against bounds of 2e-5 .. 6e-5 in the split format), all 16
     test_stem1_sums_in_stem_kernels_order cases, the three cin-1 scaling cases and the cin-1 saturation case; the 48 stem_kernel
     cases of test_stem pass, as they must, and so do the format and entry equalities (both sides share the wrong sum).  91 existing
     tests noticed: test_gpu_cbam.py's pooling stem, test_gpu_conv.py's stem_x6_kernel cases (against esahrnet_op_stem), and the
     seg_hrnet2 / seg_hrnet3 networks of every precision against goldens, oracles and emulations.
  3. One argmax_take step of to_nchw_part_kernel's cross-lane reduction as a plain `>`: 30 of the 60 test_tile_maxima cases fail,
     on the planes "nan after max", "two nans", "inf then nan" (a NaN never crosses a lane) and "lanes 63 64" (lane 0 keeps its
     pixel 64 against lane 63's equal pixel 63).  "constant" and "tile edge" pass under this mutation — lane 0, which writes,
     already holds a tile's lowest index, and `>` never replaces it on a tie; they are there for a `>=`.  9 existing tests
     noticed: the three test_ties_and_nan / test_hrnet3_partials_ties_and_nan families on seg_hrnet3 (their NaN block).
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu

# (kernel, precision name) -> factor on E_emu where a form needed more than the rule's 2, with its case, the measured ratio and
# the reason read from the kernel's arithmetic (see the docstring)
FACTOR = {}
GUARD = 256          # bytes on both sides of every device buffer the tests hand in
FILL = 0xA5          # what the guard bands (and unwritten outputs) hold: f32 0xa5a5a5a5 = -2.87e-16, not a value any case makes


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    e = dict(lib=_lib.lib(), L=_lib, worst={}, t0=time.time(), cases=0, slowest=(0.0, ""))
    yield e
    print(f"\n{e['cases']} cases in {time.time() - e['t0']:.1f} s, the slowest {e['slowest'][0]:.2f} s ({e['slowest'][1]}); "
          "worst error / bound per stem kernel and precision:")
    for key in sorted(e["worst"]):
        ratio, err, e_emu, cid = e["worst"][key]
        print(f"  {key[0]:<22} {key[1]:<7} {ratio:.3f}  ({err:.3e}, {e_emu:.3e}; {cid})")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    assert t.dtype == torch.float32 and t.is_contiguous()
    return t.numpy().ctypes.data_as(C.c_void_p)


def _call(env, rc):
    """A refused or failed call of a valid case ends the session: nothing more is started on the device after an error."""
    if rc != 0:
        pytest.exit("library call failed: " + env["lib"].esahrnet_last_error().decode(errors="replace"), returncode=3)


def _timed(env, t0, cid):
    env["cases"] += 1
    dt = time.time() - t0
    if dt > env["slowest"][0]:
        env["slowest"] = (dt, cid)


class Buf:
    """A device buffer of `nbytes` between two guard bands of GUARD bytes, all prefilled with FILL; `data` (a numpy array of
    nbytes) goes into the payload.  ptr: the payload (256-byte aligned, as torch's allocations are)."""

    def __init__(self, nbytes, data=None):
        self.nbytes = int(nbytes)
        host = np.full(self.nbytes + 2 * GUARD, FILL, dtype=np.uint8)
        if data is not None:
            d = np.ascontiguousarray(data).view(np.uint8).ravel()
            assert d.size == self.nbytes, (d.size, self.nbytes)
            host[GUARD:GUARD + self.nbytes] = d
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 256 == 0
        self.ptr = C.c_void_p(self.t.data_ptr() + GUARD)

    def read(self, dtype):
        """(payload as dtype, guard bands intact)"""
        host = self.t.cpu().numpy()
        intact = bool((host[:GUARD] == FILL).all() and (host[GUARD + self.nbytes:] == FILL).all())
        return host[GUARD:GUARD + self.nbytes].copy().view(dtype), intact

    def payload(self, dtype):
        got, intact = self.read(dtype)
        assert intact, "a guard band was written"
        return got


def _f32buf(t):
    """torch f32 CPU tensor (or f32-bit array) -> guarded device copy"""
    a = t.contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return Buf(a.nbytes, a)


# ============================================================================================== A. the stem
def _stem(env, case, d, entry="ex"):
    """esahrnet_op_stem_ex (or esahrnet_op_stem) on a case's data -> y f32 bits [n][cout][h][w]; guard bands asserted."""
    n, h, w, cin, cout, relu, p = case
    xb = _f32buf(d["x"])
    yb = Buf(n * cout * h * w * 4)
    lib = env["lib"]
    if entry == "ex":
        rc = lib.esahrnet_op_stem_ex(xb.ptr, n, cin, h, w, _ptr(d["w"]), _ptr(d["b"]), cout, relu, p, yb.ptr, _stream())
    else:
        assert cin == 1 and cout == 64
        rc = lib.esahrnet_op_stem(xb.ptr, n, h, w, _ptr(d["w"]), _ptr(d["b"]), relu, 0, p, yb.ptr, None, None, _stream())
    _call(env, rc)
    xb.payload(np.uint32)
    return yb.payload(np.uint32).reshape(n, cout, h, w)


def _t32(u):
    return torch.from_numpy(LR.f32(u).copy())


def _hold(env, key, cid, got, d, p, mask=None):
    """|HIP - f64| <= factor x E_emu + q x max|ref| over the masked elements, printed before it is asserted."""
    ref, emu = d["ref"], d["emu"]
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (key, cid)
    if mask is not None:
        got, ref, emu = got[mask], ref[mask], emu[mask]
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    e_emu = (emu.double() - ref).abs().max().item()
    bound = FACTOR.get(key, (2.0,))[0] * e_emu + LR.QUANTUM[p] * scale
    ratio = err / bound if bound > 0 else 0.0
    print(f"  {cid}: {key[0]} {key[1]}: HIP vs f64 {err:.3e}   E_emu {e_emu:.3e}   scale {scale:.3f}   error / bound {ratio:.3f}")
    if ratio > env["worst"].get(key, (0.0,))[0]:
        env["worst"][key] = (ratio, err, e_emu, cid)
    assert err <= bound, (key, cid, err, e_emu, scale, bound)


@pytest.mark.parametrize("regime", LR.STEM_REGIMES)
@pytest.mark.parametrize("case", LR.STEM_CASES, ids=LR.stem_id)
def test_stem(env, case, regime):
    """Every stem kernel in every format and cin class under the rule; the output is data of its format."""
    t0 = time.time()
    n, h, w, cin, cout, relu, p = case
    d = LR.stem_data(case, regime)
    y = _stem(env, case, d)
    assert np.array_equal(LR.QBITS[p](y), y), "not data of its format"
    cid = f"{LR.stem_id(case)}-{regime}"
    _hold(env, (LR.stem_kernel_name(cin, p), LR.PNAME[p]), cid, _t32(y), d, p)
    _timed(env, t0, cid)


FORMAT_CASES = [(n, h, w, cin, cout, relu) for (n, h, w), cin, cout, relu in (
    ((1, 3, 7), 1, 64, 1), ((3, 2, 9), 1, 128, 0), ((2, 3, 17), 1, 64, 1), ((1, 1, 1), 2, 64, 0), ((2, 5, 8), 3, 128, 1), ((1, 4, 33), 4, 64, 0))]


@pytest.mark.parametrize("regime", LR.STEM_REGIMES)
@pytest.mark.parametrize("fc", FORMAT_CASES, ids=lambda c: "n%d-%dx%d-c%d-%d-relu%d" % c)
def test_stem_formats_share_one_accumulation(env, fc, regime):
    """One f32 accumulation, four stores: the SB output is split(F32 output), the BF output bf16(F32 output), the HF output
    sat16(F32 output), bit for bit by the integer statements — in stem1_body and in stem_kernel."""
    t0 = time.time()
    d = LR.stem_data((*fc, 2), regime)
    y32 = _stem(env, (*fc, 2), d)
    assert not LR.is_nan32(y32).any()
    for p in (0, 1, 3):
        y = _stem(env, (*fc, p), d)
        bad = np.flatnonzero(y.ravel() != LR.QBITS[p](y32).ravel())
        assert bad.size == 0, (LR.PNAME[p], bad[:4], [hex(v) for v in y32.ravel()[bad[:4]]], [hex(v) for v in y.ravel()[bad[:4]]])
    _timed(env, t0, "formats-%d-%d-%d-%d-%d-%d-" % fc + regime)


@pytest.mark.parametrize("p", (0, 1, 2, 3))
@pytest.mark.parametrize("shape", ((1, 3, 7), (3, 2, 9), (2, 3, 17), (2, 1, 40)), ids=lambda s: "n%d-%dx%d" % s)
def test_stem1_sums_in_stem_kernels_order(env, shape, p):
    """stem.hip: stem1_body sums in the "same order as stem_kernel" — cin 1 equals cin 2 with the second channel's weights all
    zero (fmaf(v, 0, acc) is acc for finite v), by value, in every format, row tails included."""
    t0 = time.time()
    case1 = (*shape, 1, 64, 1, p)
    d1 = LR.stem_data(case1, "signed")
    n, h, w = shape
    x2 = torch.cat([d1["x"], LR._n("x2nd%dx%dx%d" % shape, 64, (n, 1, h, w))], 1).contiguous()
    w2 = torch.cat([d1["w"], torch.zeros_like(d1["w"])], 1).contiguous()
    y1 = _stem(env, case1, d1)
    y2 = _stem(env, (*shape, 2, 64, 1, p), dict(x=x2, w=w2, b=d1["b"]))
    assert torch.equal(_t32(y1), _t32(y2))
    _timed(env, t0, "order")


@pytest.mark.parametrize("p", (0, 1, 2))
@pytest.mark.parametrize("shape", ((2, 5, 8), (2, 3, 17), (1, 4, 33)), ids=lambda s: "n%d-%dx%d" % s)
def test_op_stem_is_op_stem_ex(env, shape, p):
    t0 = time.time()
    case = (*shape, 1, 64, 1, p)
    d = LR.stem_data(case, "signed")
    assert np.array_equal(_stem(env, case, d, "plain"), _stem(env, case, d))
    _timed(env, t0, "op_stem")


@pytest.mark.parametrize("case", LR.STEM_SCALE_CASES, ids=LR.stem_id)
def test_stem_power_of_two_scaling(env, case):
    """y(2^a x, 2^b w, 2^(a+b) bias) == 2^(a+b) y bit for bit at (a, b) = (12, -7), (-12, 7), precisions 0, 1, 2."""
    t0 = time.time()
    base = _t32(_stem(env, case, LR.stem_data(case, "signed")))
    for a, b in LR.STEM_SCALES:
        d = LR.stem_data(case, "signed", a, b)
        y = _t32(_stem(env, case, d))
        assert torch.equal(y, base * 2.0 ** (a + b)), (a, b)
        _hold(env, (LR.stem_kernel_name(case[3], case[6]), LR.PNAME[case[6]]), f"{LR.stem_id(case)}-2^({a},{b})", y, d, case[6])
    _timed(env, t0, "scaling")


@pytest.mark.parametrize("case,a", LR.STEM_SAT_CASES, ids=lambda v: LR.stem_id(v) if isinstance(v, tuple) else f"a{v}")
def test_stem_fp16_saturation(env, case, a):
    """Outputs beyond +-65504 in the float64 reference (>= 8 on each side: test_layout_host.py) are stored as exactly +-65504
    with the reference's sign; the rule holds on the elements with |ref| <= 65504 (1 - 2^-10), at least 90 % of the case."""
    t0 = time.time()
    d = LR.stem_data(case, "signed", a, 0)
    y = _stem(env, case, d)
    ref = d["ref"]
    over, under = (ref > LR.F16_MAX).numpy(), (ref < -LR.F16_MAX).numpy()
    assert over.sum() >= 8 and under.sum() >= 8
    assert (y[over] == 0x477FE000).all() and (y[under] == 0xC77FE000).all()
    assert np.array_equal(LR.QBITS[3](y), y)
    mask = ref.abs() <= LR.F16_MAX * (1 - 2.0 ** -10)
    assert mask.double().mean().item() >= 0.9
    cid = f"{LR.stem_id(case)}-2^{a}"
    _hold(env, (LR.stem_kernel_name(case[3], 3), "fp16"), cid, _t32(y), d, 3, mask)
    _timed(env, t0, cid)


# ============================================================================================== B. the conversions
def _layout(env, direction, xbits, shape, p, cp, raw=None):
    """esahrnet_op_layout -> (raw bytes as uint16 / uint32, y f32 bits); guard bands asserted.  dir 0: raw_dev prefilled with
    FILL; dir 1: with `raw`."""
    n, c, h, w = shape
    nbytes = n * h * w * cp * LR.elem_bytes(p)
    xb = _f32buf(xbits) if direction == 0 else None
    rb = Buf(nbytes, raw)
    yb = Buf(n * c * h * w * 4)
    _call(env, env["lib"].esahrnet_op_layout(direction, xb.ptr if xb else None, n, c, h, w, cp, p, rb.ptr, yb.ptr, _stream()))
    if xb:
        assert np.array_equal(xb.payload(np.uint32).ravel(), np.asarray(xbits).ravel())          # the input is not modified
    return rb.payload(np.uint32 if p == 2 else np.uint16), yb.payload(np.uint32).reshape(n, c, h, w)


def _same_raw(got, want, p):
    """Raw bytes against the host packer's: exact, all NaNs of the format one value (layout_ref.NAN_PAYLOAD)."""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    ok = LR.same_f32(got, want) if p == 2 else LR.same_16(got, want, p)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (LR.PNAME[p], bad[:6], [hex(int(v)) for v in got[bad[:6]]], [hex(int(v)) for v in want[bad[:6]]])


def _same_y(got, want):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    bad = np.flatnonzero(~LR.same_f32(got, want))
    assert bad.size == 0, (bad[:6], [hex(int(v)) for v in got[bad[:6]]], [hex(int(v)) for v in want[bad[:6]]])


@pytest.mark.parametrize("case", LR.layout_cases(), ids=LR.layout_id)
def test_conversion_round_trip(env, case):
    """dir 0 on N(0, 1) data: raw_dev is the host packer's bytes (padding channels exact +0, every byte written), y the host
    decode of those bytes, the bands untouched."""
    t0 = time.time()
    shape, p, cp = case
    x = LR.layout_x(shape)
    raw, y = _layout(env, 0, x, shape, p, cp)
    want = LR.pack(x, p, cp)
    assert np.array_equal(raw.ravel(), want.ravel())                          # finite data: bit for bit
    n, c, h, w = shape
    if p == 0:                                                                # +0 in both the hi and the lo part
        r = raw.reshape(n, h, w, cp // 8, 2, 8)
        assert not r[..., 0, :].reshape(n, h, w, cp)[..., c:].any() and not r[..., 1, :].reshape(n, h, w, cp)[..., c:].any()
    else:
        assert not raw.reshape(n, h, w, cp)[..., c:].any()
    assert np.array_equal(y, LR.unpack(raw, p, n, c, h, w, cp)) and np.array_equal(y, LR.QBITS[p](x))
    _timed(env, t0, LR.layout_id(case))


@pytest.mark.parametrize("p", (0, 1, 2, 3))
def test_conversion_of_the_value_table(env, p):
    """VALUES through every lane position of a group: ties, carries, subnormals, the fp16 saturation boundary, values whose hi
    part is inf, +-inf and NaNs — raw bytes and y are the integer statements' (a NaN is a NaN, whichever)."""
    t0 = time.time()
    x = LR.values_tensor()
    shape = x.shape
    cp = 8 if p in (0, 2) else 64
    raw, y = _layout(env, 0, x, shape, p, cp)
    _same_raw(raw, LR.pack(x, p, cp), p)
    n, c, h, w = shape
    _same_y(y, LR.unpack(raw, p, n, c, h, w, cp))
    _same_y(y, LR.QBITS[p](x))
    if p == 2:
        assert np.array_equal(y, x)                                           # a copy: NaN payloads too
    if p == 0:                                                                # +-inf and every |v| >= 0x7f7f8000 join to NaN
        beyond = (x & 0x7FFFFFFF) >= 0x7F7F8000
        assert LR.is_nan32(y[beyond]).all() and not LR.is_nan32(y[~beyond]).any() and beyond.sum() >= 80
    if p == 3:                                                                # +-inf and beyond-range values are +-65504; so is a NaN
        big = ((x & 0x7FFFFFFF) >= 0x477FF000) & ~LR.is_nan32(x)
        assert (y[big] == (0x477FE000 | (x[big] & 0x80000000))).all() and big.sum() >= 80
        assert (y[LR.is_nan32(x)] == LR.f16_to_f32_bits(np.array([LR.F16_NAN_STORE], dtype=np.uint32))[0]).all()
    sub = ((x & 0x7FFFFFFF) > 0) & ((x & 0x7FFFFFFF) < 0x00800000)            # layout_ref.SUBNORMALS == "ieee"
    assert sub.sum() >= 16 and LR.SUBNORMALS == "ieee"
    _timed(env, t0, f"values-{LR.PNAME[p]}")


def test_decode_of_bytes_no_split_produces(env):
    """dir 1, split-bf16: raw (hi, lo) pairs no split produces — a lo part as large as the hi part, inf or NaN in either part —
    decode to bf16(hi) + bf16(lo), one f32 addition, exactly: what esahrnet_tap_read promises ("exact f32 copies of what the
    device holds").  Padding groups and channels hold FILL and are not read."""
    t0 = time.time()
    hi, lo = LR.sb_decode_pairs()
    m = len(hi)
    c, cp, w = 11, 32, -(-m // 11)
    hh = np.resize(hi, w * c).reshape(w, c)
    ll = np.resize(lo, w * c).reshape(w, c)
    raw = np.full((1, 1, w, cp // 8, 2, 8), 0xA5A5, dtype=np.uint16)
    flat_h = np.full((w, cp), 0xA5A5, dtype=np.uint16)
    flat_l = flat_h.copy()
    flat_h[:, :c], flat_l[:, :c] = hh, ll
    raw[0, 0, :, :, 0, :] = flat_h.reshape(w, cp // 8, 8)
    raw[0, 0, :, :, 1, :] = flat_l.reshape(w, cp // 8, 8)
    got_raw, y = _layout(env, 1, None, (1, c, 1, w), 0, cp, raw)
    assert np.array_equal(got_raw.ravel(), raw.ravel())                       # dir 1 writes nothing into raw_dev
    _same_y(y, LR.join_bits(hh, ll).T.reshape(1, c, 1, w))
    _same_y(y, LR.unpack(raw, 0, 1, c, 1, w, cp))
    _timed(env, t0, "decode-sb")


@pytest.mark.parametrize("p", (1, 3))
def test_decode_of_every_16_bit_pattern(env, p):
    """dir 1, bf16 and fp16: all 65536 patterns — subnormals, inf, NaNs — decode to the integer statement (bf16: the bits, NaN
    payloads included)."""
    t0 = time.time()
    c, cp, w = 33, 64, -(-65536 // 33)
    pat = np.resize(np.arange(1 << 16, dtype=np.uint16), w * c).reshape(w, c)
    raw = np.full((1, 1, w, cp), 0xA5A5, dtype=np.uint16)
    raw[0, 0, :, :c] = pat
    _, y = _layout(env, 1, None, (1, c, 1, w), p, cp, raw)
    want = LR.unpack(raw, p, 1, c, 1, w, cp)
    if p == 1:
        assert np.array_equal(y, want)
    _same_y(y, want)
    num = ~LR.is_nan32(want)
    assert np.array_equal(y[num], want[num])
    _timed(env, t0, f"decode-{LR.PNAME[p]}")


def test_decode_f32_is_a_copy(env):
    t0 = time.time()
    x = LR.values_tensor()
    n, c, h, w = x.shape
    raw = LR.pack(x, 2, 16)
    raw[..., c:] = 0xA5A5A5A5
    _, y = _layout(env, 1, None, x.shape, 2, 16, raw)
    assert np.array_equal(y, x)
    _timed(env, t0, "decode-f32")


# ============================================================================================== C. the tile maxima
def _tile_cases():
    return [(case, rot, p) for case in LR.TILE_CASES for rot in LR.tile_rotations(case) for p in (0, 2)]


def _tile_max(env, raw, case, p, store, finish):
    h, w, c, cp, n = case
    nt = -(-h * w // LR.TILE)
    rb = Buf(raw.nbytes, raw)
    yb = Buf(n * c * h * w * 4)
    pb = Buf(n * c * nt * 8)
    kb, ib = Buf(n * c * 12), Buf(n * c * 4)
    ntiles = C.c_int(-1)
    _call(env, env["lib"].esahrnet_op_tile_max(rb.ptr, n, c, h, w, cp, p, store, yb.ptr, pb.ptr, C.byref(ntiles),
                                               kb.ptr if finish else None, ib.ptr if finish else None, _stream()))
    assert np.array_equal(rb.payload(np.uint8), np.ascontiguousarray(raw).view(np.uint8).ravel())       # the input is not modified
    part = pb.payload(np.uint32).reshape(n * c, nt, 2)
    return dict(ntiles=ntiles.value, part=part, y=yb.payload(np.uint32).reshape(n, c, h, w), ybuf=yb,
                kp=kb.payload(np.uint32).reshape(n * c, 3), idx=ib.payload(np.int32))


@pytest.mark.parametrize("tc", _tile_cases(), ids=lambda t: f"{LR.tile_id(t[0])}-rot{t[1]}-{LR.PNAME[t[2]]}")
def test_tile_maxima(env, tc):
    """Planted planes through to_nchw_part_kernel<F32, STORE> and the finishes: every part[plane][tile] is tile_expect's (value
    bits, index) exactly; store 1: y is the format-held values; store 0: y's buffer untouched; esahrnet_keypoints_finish(y, part)
    == esahrnet_keypoints_ex(y) == the NHWC finish of the entry, kp and idx bit for bit."""
    t0 = time.time()
    case, rot, p = tc
    h, w, c, cp, n = case
    planes = LR.tile_planes(case, rot)
    raw = LR.pack(planes, p, cp, literal_specials=True)
    if p == 0:                                                                # everything past the c real channels holds FILL, not zeros:
        r = raw.reshape(n, h, w, cp * 2)                                      # [group][hi|lo][8] seen as [group * 16 + part * 8 + lane]
        lane = np.arange(cp * 2) // 16 * 8 + np.arange(cp * 2) % 8            # -> channel: the last group's padding lanes, the groups past it
        r[..., lane >= c] = 0xA5A5
    else:
        raw[..., c:] = 0xA5A5A5A5
    held = LR.unpack(raw, p, n, c, h, w, cp)
    assert np.array_equal(held, planes)                                       # the planted values are data of the format
    want_v, want_i = LR.tile_expect(held.reshape(n * c, h * w))
    lib = env["lib"]
    r1 = _tile_max(env, raw, case, p, 1, True)
    r0 = _tile_max(env, raw, case, p, 0, True)
    for r in (r1, r0):
        assert r["ntiles"] == -(-h * w // LR.TILE)
        bad = np.flatnonzero((r["part"][:, :, 0] != want_v).ravel() | (r["part"][:, :, 1].astype(np.int32) != want_i).ravel())
        assert bad.size == 0, ([(int(b) // want_v.shape[1], LR.TILE_PATTERNS[(int(b) // want_v.shape[1] + rot) % 8], int(b) % want_v.shape[1],
                                 hex(int(r["part"].reshape(-1, 2)[b, 0])), int(r["part"].reshape(-1, 2)[b, 1]), hex(int(want_v.ravel()[b])),
                                 int(want_i.ravel()[b])) for b in bad[:6]])
    assert np.array_equal(r1["y"], held)
    assert (r0["y"] == 0xA5A5A5A5).all()                                      # store 0 leaves y alone
    assert np.array_equal(r0["kp"], r1["kp"]) and np.array_equal(r0["idx"], r1["idx"])
    # the finishes on the NCHW copy: over the tile maxima, and the full sweep
    yb = r1["ybuf"]
    pb = Buf(r1["part"].nbytes, r1["part"])
    outs = []
    for finish in (True, False):
        kb, ib = Buf(n * c * 12), Buf(n * c * 4)
        if finish:
            rc = lib.esahrnet_keypoints_finish(yb.ptr, pb.ptr, r1["ntiles"], n, c, h, w, kb.ptr, ib.ptr, _stream())
        else:
            rc = lib.esahrnet_keypoints_ex(yb.ptr, n, c, h, w, kb.ptr, ib.ptr, _stream())
        _call(env, rc)
        torch.cuda.synchronize()
        outs.append((kb.payload(np.uint32).reshape(n * c, 3), ib.payload(np.int32)))
    (kf, idf), (ke, ide) = outs
    assert np.array_equal(idf, ide) and np.array_equal(kf, ke)
    assert np.array_equal(r1["idx"], ide) and np.array_equal(r1["kp"], ke)
    # and the index is the plane's: the first NaN, otherwise the first maximum (an all -inf plane: 0)
    flat = held.reshape(n * c, h * w)
    nan = LR.is_nan32(flat)
    with np.errstate(invalid="ignore"):
        whole = np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, LR.f32(flat)).argmax(axis=1))
    assert np.array_equal(ide, whole.astype(np.int32))
    assert np.array_equal(ke[:, 2], flat[np.arange(n * c), whole])            # the peak is the raw value's bits
    _timed(env, t0, f"{LR.tile_id(case)}-rot{rot}-{LR.PNAME[p]}")


# ============================================================================================== refusals
def test_refusals_leave_the_device_alone(env):
    """The three entries with device pointers: non-zero, a message, FILL-filled outputs untouched, a good call afterwards."""
    lib = env["lib"]
    err = lambda: lib.esahrnet_last_error().decode()  # noqa: E731
    case = (1, 3, 7, 1, 64, 0, 0)
    d = LR.stem_data(case, "signed")
    xb, yb, rb = _f32buf(d["x"]), Buf(64 * 21 * 4), Buf(21 * 64 * 4)
    assert lib.esahrnet_op_stem_ex(xb.ptr, 1, 5, 3, 7, _ptr(d["w"]), _ptr(d["b"]), 64, 0, 0, yb.ptr, _stream()) != 0 and "cin" in err()
    assert lib.esahrnet_op_stem_ex(xb.ptr, 1, 1, 3, 7, _ptr(d["w"]), _ptr(d["b"]), 48, 0, 0, yb.ptr, _stream()) != 0 and "cout" in err()
    assert lib.esahrnet_op_stem_ex(xb.ptr, 1, 1, 3, 7, _ptr(d["w"]), _ptr(d["b"]), 32, 0, 1, yb.ptr, _stream()) != 0
    assert lib.esahrnet_op_stem_ex(xb.ptr, 1, 1, 3, 7, _ptr(d["w"]), _ptr(d["b"]), 32, 0, 3, yb.ptr, _stream()) != 0
    assert lib.esahrnet_op_stem_ex(xb.ptr, 1, 1, 3, 7, _ptr(d["w"]), _ptr(d["b"]), 64, 0, 4, yb.ptr, _stream()) != 0 and "precision" in err()
    assert lib.esahrnet_op_layout(0, xb.ptr, 1, 1, 3, 7, 12, 0, rb.ptr, yb.ptr, _stream()) != 0 and "cp" in err()
    assert lib.esahrnet_op_layout(0, xb.ptr, 1, 9, 1, 2, 8, 0, rb.ptr, yb.ptr, _stream()) != 0 and "cp" in err()
    assert lib.esahrnet_op_layout(3, xb.ptr, 1, 1, 3, 7, 32, 0, rb.ptr, yb.ptr, _stream()) != 0 and "dir" in err()
    nt = C.c_int(-7)
    assert lib.esahrnet_op_tile_max(rb.ptr, 1, 33, 3, 7, 64, 0, 1, yb.ptr, xb.ptr, C.byref(nt), None, None, _stream()) != 0
    assert lib.esahrnet_op_tile_max(rb.ptr, 1, 8, 3, 7, 32, 1, 1, yb.ptr, xb.ptr, C.byref(nt), None, None, _stream()) != 0 and "precision" in err()
    assert lib.esahrnet_op_tile_max(rb.ptr, 1, 8, 3, 7, 32, 0, 1, None, xb.ptr, C.byref(nt), None, None, _stream()) != 0
    torch.cuda.synchronize()
    assert nt.value == -7
    assert (yb.payload(np.uint8) == FILL).all() and (rb.payload(np.uint8) == FILL).all()
    assert np.array_equal(xb.payload(np.uint32), LR.bits(d["x"]).ravel())
    y = _stem(env, case, d)                                                   # and good calls afterwards
    assert not (y == 0xA5A5A5A5).any()
    raw = LR.pack(LR.bits(d["x"]), 2, 8)                                      # store 0 takes a NULL y_dev
    tb, pb = Buf(raw.nbytes, raw), Buf(8)
    _call(env, lib.esahrnet_op_tile_max(tb.ptr, 1, 1, 3, 7, 8, 2, 0, None, pb.ptr, C.byref(nt), None, None, _stream()))
    part = pb.payload(np.uint32)
    assert nt.value == 1 and int(part[0]) == int(LR.bits(d["x"].max().reshape(1))[0]) and int(part[1]) == int(d["x"].argmax())
