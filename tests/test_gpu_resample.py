"""The resampling kernels held to a float64 reference, operator by operator: launch_fuse (fuse_kernel in its four formats,
fuse2x2_kernel's cell and selection paths, the host reordering, all 14 (NS, NU) instantiations), resample_slice (both
align_corners rules, the copy path, the channel offset) and zero_slice.  References, tap rule and case tables:
tests/resample_ref.py; what the CPU can check at every size is in tests/test_resample_host.py.

Bounds, none invented here:
  * precision 2 (fp32-grade): |HIP - f64| <= 2 x |torch f32 - f64| + 2.4e-7 x scale, the rule and slack of
    tests/test_gpu_fp32.py::test_op_conv_fp32_grade (max over the tensor; scale = max |reference|).  A pure copy (one
    same-resolution term, h == H) must return the bits;
  * precision 0 (split-bf16): 5e-5 absolute, tests/test_gpu_parity.py::test_op_fuse_matches_torch_cpu's bound for four
    unit-normal terms (every case here has at most four);
  * precisions 1 / 3 (bf16 / fp16): inputs rounded with the emulators of tests/test_gpu_bf16.py (qb) and tests/fp16_emu.py
    (q16, the qh of tests/test_gpu_fp16.py), the f64 result on those, one output rounding of the format plus those tests' floor:
    |y - ref| <= 2^-8 |ref| + 2e-6 (bf16), 2^-11 |ref| + 2e-6 (fp16), element by element; the output is data of the format;
    the fp16 saturation check is test_op_fuse_fp16_saturates' own.
A wrong tap, clamp or slice offset moves an output by O(0.1) against these.

What each case is there to catch (fuse.hip / cbam.hip):
  chain18x34      fuse2x2_kernel's 3x3 selection (selx / sely, column c / row c) at ratios 2, 3.6 / 3.78 and 6 / 6.8
  cell16x32       the one-cell path with ry != rx, cell_mask per term
  nocell16x32     `exact` needing both directions: a cell in y only would take the wrong column for X + 1
  ratio16_32      in - 1 = 0: i1 = i0 at every pixel, the clamp of i0
  fallback_h / _w a ratio below 2 (10 -> 18, 18 -> 34) and fuse_kernel<.., FMT_F32> with two blocks per row.  They do not
                  test the 2 * h <= H predicate itself: the 2x2 kernel's claim holds at every ratio >= 1, the predicate is
                  a matter of speed
  odd9x17         odd grids stay on fuse_kernel (the 2x2 kernel would write past the last row / column)
  chain36x132     blockIdx.x > 0 in both kernels, n = 3: the row -> (n, y) decomposition and the per-image source base
  nsXnuY          every instantiation of the switch; the shuffled order fails if launch_fuse does not reorder x, h, w and the
                  scales together
  resample        lerp_any's two rules, the copy path, y_c0 / y_pix_bytes addressing; c = 12: the partial last group
  zero_slice      the group count and offset; nothing but the slice is touched

Measured on an MI355X (every case prints its figure beside its bound, run with -s; worst over the cases of a precision):
  precision 2   fuse 5.41e-6 (torch f32 itself 5.31e-6; 10x18 -> 18x34), resample 7.25e-6 (torch's own figure; 35x25 -> 70x50,
                align 1): the f32 weight src - i0 carries an ulp of src; never above 0.48 of the bound
  precision 0   fuse 4.89e-5 (36x132 chain, n = 3: four terms and the output each rounded to 16 bits; bound 5e-5),
                resample 2.84e-5
  precision 1   worst error / bound 0.996 (1.56e-2 at |ref| ~ 4: half a bf16 ulp at the bottom of a binade is the bound)
  precision 3   worst error / bound 0.995 (1.95e-3)
fuse2x2_kernel's selection, checked once on a scratch build that takes column a where b is due (`c0[r][1] = v[r][0][i]`):
chain18x34 (both relu), nocell16x32 (both) and ns1nu3 fail with an error of 6.8 against a bound of 5.8e-6; cell16x32 and
odd9x17, which do not run that line, pass.  fp16_emu.q16 is the `qh` of tests/test_gpu_fp16.py."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_emu  # noqa: E402
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return dict(lib=_lib.lib(), L=_lib)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _op_fuse(env, xs, sizes, n, c, hw, relu, precision):
    lib, L = env["lib"], env["L"]
    k = len(xs)
    xd = [t.cuda() for t in xs]
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in xd])
    hs = (C.c_int * k)(*[s[0] for s in sizes])
    ws = (C.c_int * k)(*[s[1] for s in sizes])
    y = torch.full((n, c) + tuple(hw), NAN, device="cuda")
    L.check(lib.esahrnet_op_fuse_ex(ptrs, hs, ws, k, n, c, hw[0], hw[1], relu, y.data_ptr(), precision, _stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _op_resample(env, x, y0, c0, align, precision):
    lib, L = env["lib"], env["L"]
    n, c, h, w = x.shape
    _, cy, H, W = y0.shape
    xd, y = x.cuda(), y0.cuda()
    L.check(lib.esahrnet_op_resample(xd.data_ptr(), n, c, h, w, y.data_ptr(), cy, c0, H, W, align, precision, _stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _op_zero(env, y0, c0, nchan, precision):
    lib, L = env["lib"], env["L"]
    n, cy, H, W = y0.shape
    y = y0.cuda()
    L.check(lib.esahrnet_op_zero_slice(y.data_ptr(), n, cy, H, W, c0, nchan, precision, _stream()))
    torch.cuda.synchronize()
    return y.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


Q = {0: R.q_sb, 1: R.q_bf, 2: lambda t: t, 3: fp16_emu.q16}


def _check(tag, precision, y, xs, hw, relu, ref=None, ref32=None, copy=False):
    """The bound of `precision` on a fuse / resample result y against the f64 reference; prints the measured error."""
    assert bool(torch.isfinite(y).all()), f"{tag}: the NaN prefill shows through or the kernel made one"
    if precision == 2:
        err = (y.double() - ref).abs().max().item()
        err32 = (ref32.double() - ref).abs().max().item()
        scale = ref.abs().max().item()
        print(f"{tag} p2: HIP vs f64 {err:.3e}   torch f32 vs f64 {err32:.3e}   scale {scale:.2f}")
        if copy:
            assert _same_bits(y, ref32)
        assert err <= 2.0 * err32 + 2.4e-7 * scale, (err, err32, scale)
    elif precision == 0:
        err = (y.double() - ref).abs().max().item()
        print(f"{tag} p0: HIP vs f64 {err:.3e}   (bound 5e-5)")
        assert err <= 5e-5, err
    else:
        rel = 2.0 ** -8 if precision == 1 else 2.0 ** -11
        assert torch.equal(Q[precision](y), y)                    # the output IS data of the format
        d = (y.double() - ref).abs()
        bound = ref.abs() * rel + 2e-6
        print(f"{tag} p{precision}: HIP vs f64 of rounded inputs {d.max().item():.3e}   worst error / bound {(d / bound).max().item():.3f}")
        bad = d > bound
        assert not bool(bad.any()), (d.max().item(), int(bad.sum()))


def _fuse_case(env, tag, n, c, hw, sizes, relu, precision):
    sizes = tuple(sizes)
    xs = R.fuse_inputs(tag, n, c, sizes)
    y = _op_fuse(env, xs, sizes, n, c, hw, relu, precision)
    if precision in (0, 2):
        ref, ref32 = R.fuse_refs(tag, n, c, tuple(hw), sizes, relu)
    else:
        ref, ref32 = R.fuse([Q[precision](t) for t in xs], hw[0], hw[1], relu), None
    _check(f"fuse {tag} relu={relu}", precision, y, xs, hw, relu, ref, ref32, copy=R.fuse_is_copy(hw, sizes))


# ------------------------------------------------------------------------------------------------ fuse, fp32-grade
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", R.FUSE_TABLE, ids=lambda c: c[0])
def test_fuse_fp32_grade(env, case, relu):
    tag, n, c, hw, sizes = case
    _fuse_case(env, tag, n, c, hw, sizes, relu, 2)


@pytest.mark.parametrize("nsnu", R.NSNU, ids=lambda p: f"ns{p[0]}nu{p[1]}")
def test_fuse_every_instantiation_shuffled_terms(env, nsnu):
    """One case per (NS, NU) of launch_fuse's switch, output 18x34 (fuse2x2_kernel whenever NU > 0), terms handed over as
    [up, same, up, same]: the host must sort them, with their sizes and scales."""
    ns, nu = nsnu
    sizes = R.nsnu_sizes(ns, nu)
    assert sum(s == (18, 34) for s in sizes) == ns and len(sizes) == ns + nu
    if ns and nu:
        assert sizes[0] != (18, 34)                  # really out of order
    _fuse_case(env, f"ns{ns}nu{nu}", 2, 8, (18, 34), sizes, (ns + nu) & 1, 2)


# ------------------------------------------------------------------------------------------------ fuse, the other formats
@pytest.mark.parametrize("precision", [0, 1, 3])
@pytest.mark.parametrize("case", R.FUSE_LOWP, ids=lambda c: c[0])
def test_fuse_other_formats(env, case, precision):
    tag, n, c, hw, sizes = case
    _fuse_case(env, tag, n, c, hw, sizes, 0 if tag.startswith("ns3") else 1, precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_fuse_kernel_several_blocks_per_row(env, precision):
    tag, n, c, hw, sizes = R.FUSE_LOWP_WIDE
    _fuse_case(env, tag, n, c, hw, sizes, 0, precision)


def test_fuse_fp16_saturates_on_the_chain(env):
    """test_op_fuse_fp16_saturates' check, unchanged, at the network's non-exact ratios: a sum that leaves the range is
    +-65504, never inf, and inside the range the result is the rounding of the sum to that test's 2^-11 |ref| + 1e-2.
    The same-resolution term is N(0, 3e4) as there; the up-sampled ones are N(0, 3e3) (resample_ref.sat_inputs): their
    weights are not dyadic here, and where the terms cancel the f32 roundings of products of 3e4 would alone reach 1e-2."""
    n, c, hw, sizes = R.SAT_CASE
    xs = R.sat_inputs()
    ref = R.fuse([fp16_emu.q16(t) for t in xs], hw[0], hw[1], 0)
    y = _op_fuse(env, xs, sizes, n, c, hw, 0, 3)
    assert bool(torch.isfinite(y).all())
    over, under = ref > 65600.0, ref < -65600.0
    assert int(over.sum()) > 20 and int(under.sum()) > 20
    assert bool((y[over] == F16_MAX).all()) and bool((y[under] == -F16_MAX).all())
    inside = ref.abs() < 65400.0
    d = (y.double() - ref).abs()
    print(f"fuse fp16 saturation: {int(over.sum())} over, {int(under.sum())} under; inside the range worst error beyond "
          f"2^-11 |ref|: {(d - ref.abs() * 2.0 ** -11)[inside].max().item():.3e} (floor 1e-2)")
    assert bool((d[inside] <= (ref.abs() * 2.0 ** -11 + 1e-2)[inside]).all())


# ------------------------------------------------------------------------------------------------ resample_slice
def _ref_input(precision, x):
    """bf16 / fp16: the reference starts from the rounded inputs; split-bf16 and fp32-grade answer for the plain ones."""
    return Q[precision](x) if precision in (1, 3) else x


def _y0(tag, n, cy, HW, c0, cw):
    """y before the call: finite unit-normal values everywhere, NaN in the channels the kernel has to write."""
    y0 = R.resample_input("y0_" + tag, n, cy, HW).clone()
    y0[:, c0:c0 + cw] = NAN
    return y0


def _outside_unchanged(precision, y, y0, c0, cw):
    keep = torch.ones(y0.shape[1], dtype=torch.bool)
    keep[c0:c0 + cw] = False
    if precision == 2:
        assert _same_bits(y[:, keep], y0[:, keep])              # f32 holds them exactly: the bits
    else:
        assert _same_bits(y[:, keep], Q[precision](y0[:, keep]))      # their rounding to the format, nothing else


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("size", R.RESAMPLE_SIZES, ids=lambda s: s[0])
def test_resample_slice(env, size, align, precision):
    tag, hw, HW = size
    n, c, cy, c0 = 2, 8, 24, 8
    x = R.resample_input(tag, n, c, hw)
    y0 = _y0(tag, n, cy, HW, c0, c)
    y = _op_resample(env, x, y0, c0, align, precision)
    xq = Q[precision](x)
    ref = R.resample(_ref_input(precision, x), HW[0], HW[1], align)
    _check(f"resample {tag} align={align}", precision, y[:, c0:c0 + c], None, HW, 0, ref, R.resample32(x, HW[0], HW[1], align),
           copy=hw == HW)
    if hw == HW and precision != 2:
        assert _same_bits(y[:, c0:c0 + c], xq)                   # the copy path moves stored values
    _outside_unchanged(precision, y, y0, c0, c)


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("c0", [0, 8, 104])
def test_resample_slice_placement(env, c0, precision):
    """c = 40 into cy = 160 (padded 160; bf16: 192) at the first group, the second, and one past the 64-channel block."""
    n, c, cy, hw, HW = 2, 40, 160, (5, 9), (9, 17)
    x = R.resample_input("place", n, c, hw)
    y0 = _y0("place", n, cy, HW, c0, c)
    y = _op_resample(env, x, y0, c0, 0, precision)
    ref = R.resample(_ref_input(precision, x), HW[0], HW[1], 0)
    _check(f"resample place c0={c0}", precision, y[:, c0:c0 + c], None, HW, 0, ref, R.resample32(x, HW[0], HW[1], 0))
    _outside_unchanged(precision, y, y0, c0, c)


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_resample_slice_partial_last_group(env, precision):
    """c = 12: resample_slice's thread is (pixel, 8-channel group of the SOURCE) and G = (C + 7) / 8, so the second group is
    written whole: channels c0 + 12 .. c0 + 15 of y receive the source's channels 12..15 — its padding, zeros — and whatever
    lay there is overwritten.  The groups on either side are not touched.  This agrees with the plan: every slice starts on a
    group (launch_resample_slice refuses y_c0 % 8), a slice that ends inside a group is the last one of its tensor
    (head_cat2's heat-maps), and the zero_slice behind it starts at the next group ((K + 7) & ~7): the resample owns the rest
    of its last group and must leave zeros there, which is asserted here."""
    n, c, cy, c0, hw, HW = 2, 12, 32, 8, (5, 9), (9, 17)
    x = R.resample_input("partial", n, c, hw)
    y0 = R.resample_input("y0_partial", n, cy, HW).clone()
    y0[:, c0:c0 + c] = NAN                                       # 20..23 stay finite and non-zero: they must turn to zero
    y = _op_resample(env, x, y0, c0, 0, precision)
    ref = R.resample(_ref_input(precision, x), HW[0], HW[1], 0)
    _check("resample c=12", precision, y[:, c0:c0 + c], None, HW, 0, ref, R.resample32(x, HW[0], HW[1], 0))
    assert bool((y0[:, c0 + 12:c0 + 16] != 0).all())
    assert bool((_bits(y[:, c0 + 12:c0 + 16]) == 0).all())       # +0, the source's padding
    _outside_unchanged(precision, y, y0, c0, 16)


def test_resample_and_zero_slice_refuse_bad_slices(env):
    """Argument errors come back before anything is enqueued: y is untouched."""
    lib = env["lib"]
    x = torch.zeros((1, 8, 2, 2), device="cuda")
    y = torch.full((1, 32, 4, 4), 3.0, device="cuda")
    a = (x.data_ptr(), 1, 8, 2, 2, y.data_ptr(), 32)
    assert lib.esahrnet_op_resample(*a, 4, 4, 4, 0, 2, _stream()) != 0           # c0 not a multiple of 8
    assert lib.esahrnet_op_resample(*a, 32, 4, 4, 0, 2, _stream()) != 0          # slice outside y
    assert lib.esahrnet_op_resample(*a, 0, 4, 4, 0, 3, _stream()) != 0           # fp16: not served
    assert b"precision" in lib.esahrnet_last_error()
    z = (y.data_ptr(), 1, 32, 4, 4)
    assert lib.esahrnet_op_zero_slice(*z, 4, 8, 2, _stream()) != 0
    assert lib.esahrnet_op_zero_slice(*z, 8, 12, 2, _stream()) != 0
    assert lib.esahrnet_op_zero_slice(*z, 24, 16, 2, _stream()) != 0
    assert lib.esahrnet_op_zero_slice(*z, 0, 8, 3, _stream()) != 0
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())


# ------------------------------------------------------------------------------------------------ zero_slice
ZERO_CASES = [
    # cy, c0, nchan
    (64, 0, 8),         # first group
    (64, 24, 16),       # a middle offset, two groups
    (64, 56, 8),        # the last group
    (40, 40, 24),       # as the plan uses it: only channel padding (bf16: 40..63 of 64; else 40..63 of 64) — nothing visible moves
]


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("case", ZERO_CASES, ids=lambda c: "x".join(map(str, c)))
def test_zero_slice(env, case, precision):
    cy, c0, nchan = case
    n, HW = 2, (9, 17)
    finite = R.resample_input("zero", n, cy, HW)
    nan = torch.full_like(finite, NAN)
    _bits(nan)[:, :, ::2] = 0x7FC12345                           # NaN bit patterns with a payload, and 0x7fc00000
    for name, y0 in (("finite", finite), ("nan", nan)):
        y = _op_zero(env, y0, c0, nchan, precision)
        hi = min(cy, c0 + nchan)
        assert bool((_bits(y[:, c0:hi]) == 0).all()), name       # exactly +0
        keep = torch.ones(cy, dtype=torch.bool)
        keep[c0:hi] = False
        if precision == 2:
            assert _same_bits(y[:, keep], y0[:, keep]), name
        elif name == "nan":
            assert bool(torch.isnan(y[:, keep]).all())           # a NaN stays a NaN through the format (its payload may not)
        else:
            assert _same_bits(y[:, keep], Q[precision](y0[:, keep]))
    print(f"zero_slice cy={cy} c0={c0} nchan={nchan} p{precision}: slice +0, rest unchanged")
