"""CBAM (cbam.hip) and the pooling stem (stem.hip: launch_stem_pool) held to a float64 reference step by step.

esahrnet_op_cbam_steps makes the launches of esahrnet_op_cbam and hands out the buffers the steps leave: pool_partial's per-slab
(sum, max), ca_mlp's ca, cbam_maps' maps, and y.  Each step's reference (tests/cbam_ref.py) reads the DEVICE's outputs of the
step before, copied back exactly, so a bound has to leave room for one step only:
  partial   per slab: the maximum equals the slab's maximum of the format-held x bit for bit; empty slabs read (0, -inf); the sum
            is within the any-order float32 summation bound (m - 1) 2^-24 sum|v| of the float64 sum (m pixels in the slab)
  ca        from the device partials reduced in float64; the rule with scale 1; padding channels exact zeros
  maps      (cbam_maps + cbam_apply only) from x and the device ca: the maximum map equals max_{c<C} f32(ca[c] * x[c]) bit for
            bit, the mean map follows the rule
  y         from x, res, the device ca and the device maps (cbam_spatial: float64 maps of the device ca); in the 16-bit mode
            data of its format; padding channels of the slice exact zeros; channels outside the slice untouched
The rule, taken against the reference only (tests/test_gpu_head.py has the same):
    |HIP - f64|_max <= 2 x E_emu + q x max|ref|,      E_emu = max |float32 emulation of the step - f64| on the same inputs
q = 2.4e-7 for partial, ca, maps and for y in the fp32-grade mode; for y otherwise the storage quantum 2^-17 (split-bf16) or
2^-9 (bf16).  Inputs: cbam_ref.planted — planted channel maxima at the slab borders, pixels and channels that are negative
throughout (the only inputs on which a padding channel's zero or a pool started at 0 shows); tests/test_cbam_host.py holds the
conditions on them.  Shapes, channel counts and slab counts: cbam_ref's tables; what each is there for: test_cbam_host.py::
test_slab_geometry_and_case_table.  Every case prints the error, E_emu and error / bound of each step (run with -s); the
module prints the worst per step, form and precision at the end.

The stem: esahrnet_op_stem runs conv1 (cin 1, cout 64) through launch_stem_pool / launch_stem.  y follows the rule against a
float64 conv2d (emulation: torch float32 rounded to the format), pooled and unpooled y are the same bits, every slab's maximum
is that of its row piece of the returned y bit for bit (bf16: of the rounded values, as stem.hip says), every slab's sum is
within the summation bound, slabs_out = h * ceil(w / 256).

Measured on an MI355X (439 cases in 6.0 s, 3.8 s of it in the cases themselves, 9 ms a case on average — tests/test_gpu_head.py: 393
cases in 27 s; worst error / bound per step, form and precision, with the HIP error and E_emu of that case):
  partial  slab sums / summation bound   split-bf16 1.00   bf16 0.77   fp32-grade 1.00   (5x13, two pixels a slab: the bound
           is then one rounding of the sum, and it is attained); maxima and empty slabs exact everywhere
  ca       split-bf16 0.21 (8.6e-8, 9.0e-8; c264 1x1)   bf16 0.20 (7.4e-8, 6.1e-8; c48 4x4)   fp32-grade 0.20
  maps     mean map: split-bf16 0.41 (8.0e-7, 5.6e-7; c264 4x4)   bf16 0.54 (1.78e-6, 1.23e-6; c384 17x33)
           fp32-grade 0.38 (1.12e-6, 1.05e-6; c384 17x33); maximum map exact everywhere
  y        cbam_maps + cbam_apply   split-bf16 0.32 (3.0e-5, 3.0e-5; c64 32x32 P = 1024)   bf16 0.39 (1.50e-2, 1.50e-2; c32 17x33)
                                    fp32-grade 0.41 (6.2e-7, 3.6e-7; c264 7x9)
           cbam_spatial             split-bf16 0.31 (3.0e-5, 3.0e-5; c128 17x33)   bf16 0.39 (1.50e-2, 1.50e-2; c32 17x33)
                                    fp32-grade 0.33 (8.0e-7, 6.5e-7; c48 17x33)
  stem     y: split-bf16 0.31 (4.9e-4, 4.9e-4; 3x21)   bf16 0.39 (0.249, 0.249)   fp32-grade 0.25 (8.9e-6, 8.9e-6)   (|y| up to 77)
           slab sums / summation bound: split-bf16 0.28   bf16 0.04   fp32-grade 0.39; maxima exact
A ratio near 0.3 .. 0.5 in the 16-bit formats means kernel and emulation round to the same value at the worst element.  No step
needed a factor above the rule's 2 (FACTOR is empty), and no emulation needed a rounding point added after the measurement.

One defect found, in stem.hip: in the split-bf16 format launch_stem_pool pooled its f32 accumulators, not the hi + lo values it
stores (the bf16 format already pooled the rounded values), so a slab's maximum was not that of the tensor and differed from
what pool_partial finds in it by up to 2^-17 relative.  test_stem_and_its_pool's bit-for-bit maximum holds the fix.
Channel count 264: 33 groups of 8 hold channels, the padded tensor has 36 (288 channels; bf16: 40), 7 (6) pixels a block.

Teeth, each checked once on a scratch build with one arithmetic mutation of cbam.hip (none widens an index range):
  1. pool_partial stops one pixel short of a slab's end (p1 - 1): all 407 CBAM cases fail at the first slab's maximum, bit for
     bit (the planted maxima sit on slab ends; one-pixel slabs turn empty).  This form of the mutation is blunt — the one-pixel
     slabs of every branch of 64 pixels or fewer read (0, -inf) — so test_op_cbam_* (28 of 32) and 26 seg_hrnet3 network tests
     noticed it too.
  2. cbam_maps and cbam_spatial without the `< C` guards on the maximum: all 234 cases with C < Cp fail (c = 16, 24, 48, 264, 400
     in every format, 32 and 96 in bf16) — the 176 two-kernel cases at the maximum map, bit for bit, the 58 cbam_spatial cases at
     y by 23 .. 1.2e6 times the bound; the 173 cases with C = Cp pass, as they must.  None of the 111 existing tests that run
     these kernels (test_op_cbam_*, the seg_hrnet3 network, golden and intermediate tests of every precision) noticed.
  3. cbam_spatial's 7x7 window one column off (px + min(kx + 1, 6)): all 98 cbam_spatial cases fail at y by 51 .. 2.4e6 times
     the bound, every two-kernel case passes.  Of the existing tests the 8 fused cases of test_op_cbam_bf16_* and 14 network
     tests noticed (goldens at 128x128, test_hrnet3_*cbam_forms_agree, W48); no operator test runs cbam_spatial in the
     split-bf16 or fp32-grade format.
"""
import ctypes as C
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cbam_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu

NEG_INF = -float("inf")
FACTOR = {}              # step -> factor on E_emu where a step needed more than the rule's 2 (none did: see the docstring)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    e = dict(lib=_lib.lib(), L=_lib, worst={}, t0=time.time(), cases=0)
    yield e
    print(f"\n{e['cases']} cases in {time.time() - e['t0']:.1f} s; worst error / bound per step, form and precision:")
    for key in sorted(e["worst"]):
        ratio, err, e_emu, cid = e["worst"][key]
        print(f"  {key[0]:<9} {key[1]:<11} {key[2]:<7} {ratio:.3f}  ({err:.3e}, {e_emu:.3e}; {cid})")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return t.numpy().ctypes.data_as(C.c_void_p)


def _call(env, rc):
    """A refused or failed call of a valid case ends the session: nothing more is started on the device after an error."""
    if rc != 0:
        pytest.exit("library call failed: " + env["lib"].esahrnet_last_error().decode(errors="replace"), returncode=3)


def _hold(env, key, cid, got, ref, emu, q, scale=None):
    """|HIP - f64| <= factor x E_emu + q x scale (scale: max|ref| unless given), printed before it is asserted."""
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), key
    scale = ref.abs().max().item() if scale is None else scale
    err = (got.double() - ref).abs().max().item()
    e_emu = (emu.double() - ref).abs().max().item()
    bound = FACTOR.get(key[0], 2.0) * e_emu + q * scale
    ratio = err / bound
    print(f"  {key[0]}: HIP vs f64 {err:.3e}   E_emu {e_emu:.3e}   scale {scale:.3f}   error / bound {ratio:.3f}")
    if ratio > env["worst"].get(key, (0.0,))[0]:
        env["worst"][key] = (ratio, err, e_emu, cid)
    assert err <= bound, (key, err, e_emu, scale, bound)


def _run_steps(env, d, c, h, w, n, p, rr, fused, slabs, P, want_maps=True):
    cp = d["cp"]
    yd, xd = d["y0"].cuda(), d["x"].cuda()
    rd = d["res"].cuda() if rr else None                    # (kept alive across the call)
    part = torch.full((n, P, cp, 2), float("nan"), device="cuda")
    ca = torch.full((n, cp), float("nan"), device="cuda")
    maps = torch.full((n, h, w, 2), float("nan"), device="cuda") if want_maps and not fused else None
    _call(env, env["lib"].esahrnet_op_cbam_steps(
        xd.data_ptr(), rd.data_ptr() if rr else None, n, c, h, w, _ptr(d["w0"]), _ptr(d["w2"]), _ptr(d["wsa"]), int(rr),
        yd.data_ptr(), d["cy"], d["c0"], int(fused), p, slabs, part.data_ptr(), ca.data_ptr(),
        maps.data_ptr() if maps is not None else None, _stream()))
    torch.cuda.synchronize()
    return yd.cpu(), part.cpu(), ca.cpu(), None if maps is None else maps.cpu()


@pytest.mark.parametrize("case", CR.cbam_cases(), ids=CR.case_id)
def test_cbam_steps(env, case):
    c, (h, w, n), p, rr, fused, slabs = case
    cid = CR.case_id(case)
    hw = h * w
    P = CR.slab_rule(hw, slabs)
    d = CR.planted(c, h, w, n, p, P)
    x, res, cp, c0 = d["x"], (d["res"] if rr else None), d["cp"], d["c0"]
    y, part, ca, maps = _run_steps(env, d, c, h, w, n, p, rr, fused, slabs, P)
    form, prec = ("spatial" if fused else "maps_apply"), CR.PNAME[p]
    print(f"\n{cid}: Cp {cp}, P {P}")
    env["cases"] += 1

    # ---- partial: per slab, on the values the format holds
    v = x.double().reshape(n, c, hw)
    worst = 0.0
    for s, (p0, p1) in enumerate(CR.slab_bounds(hw, P)):
        if p1 <= p0:
            assert bool((part[:, s, :, 0] == 0).all()) and bool((part[:, s, :, 1] == NEG_INF).all()), ("empty slab", s)
            continue
        assert torch.equal(part[:, s, :c, 1], x.reshape(n, c, hw)[:, :, p0:p1].amax(-1)), ("slab maximum", s)
        assert bool((part[:, s, c:] == 0).all()), ("padding channels of a slab", s)
        b = CR.sum_bound(v, p0, p1)
        e = (part[:, s, :c, 0].double() - v[:, :, p0:p1].sum(-1)).abs()
        assert bool((e <= b).all()), ("slab sum", s, e.max().item(), b.max().item())
        worst = max(worst, (e / b.clamp_min(1e-300)).max().item() if p1 - p0 > 1 else 0.0)
    print(f"  partial: maxima exact; worst sum error / summation bound {worst:.3f}")
    key = ("partial", "-", prec)
    if worst > env["worst"].get(key, (0.0,))[0]:
        env["worst"][key] = (worst, 0.0, 0.0, cid)

    # ---- ca: from the device's partials
    assert bool((ca[:, c:] == 0).all())
    _hold(env, ("ca", "-", prec), cid, ca[:, :c], CR.ref_ca(part[:, :, :c], hw, d["w0"], d["w2"]),
          CR.emu_ca(part[:, :, :c], hw, d["w0"], d["w2"]), CR.Q_F32, scale=1.0)

    # ---- maps: from x and the device's ca
    cad = ca[:, :c]
    if not fused:
        rm, em = CR.ref_maps(x, cad), CR.emu_maps(x, cad)
        assert torch.equal(maps[..., 1], em[..., 1]), "maximum map"
        _hold(env, ("maps", "mean", prec), cid, maps[..., 0], rm[..., 0], em[..., 0], CR.Q_F32)
        ry = CR.ref_y(x, res, cad, maps, d["wsa"], rr)
        ey = CR.emu_y(x, res, cad, maps, d["wsa"], rr, p)
    else:
        ry = CR.ref_y(x, res, cad, CR.ref_maps(x, cad), d["wsa"], rr)
        ey = CR.emu_y(x, res, cad, CR.emu_maps(x, cad), d["wsa"], rr, p)

    # ---- y
    if p == 1:
        assert torch.equal(CR.Q[1](y), y)                                                   # data of its format
    _hold(env, ("y", form, prec), cid, y[:, c0:c0 + c], ry, ey, CR.QUANTUM[p])
    assert bool((y[:, c0 + c:c0 + cp] == 0).all())                                          # padding channels of the slice
    assert torch.equal(y[:, :c0], d["y0"][:, :c0]) and torch.equal(y[:, c0 + cp:], d["y0"][:, c0 + cp:])   # outside: untouched


def test_op_cbam_is_op_cbam_steps(env):
    """esahrnet_op_cbam is the same body: the same bits, and the default slab rule."""
    c, h, w, n, p = 48, 17, 33, 2, 0
    d = CR.planted(c, h, w, n, p, 64)
    y, part, ca, maps = _run_steps(env, d, c, h, w, n, p, True, 0, 0, 64)
    yd, xd, rd = d["y0"].cuda(), d["x"].cuda(), d["res"].cuda()
    _call(env, env["lib"].esahrnet_op_cbam(xd.data_ptr(), rd.data_ptr(), n, c, h, w, _ptr(d["w0"]), _ptr(d["w2"]), _ptr(d["wsa"]),
                                               1, yd.data_ptr(), d["cy"], d["c0"], 0, p, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), y)


def test_refusals_enqueue_nothing(env):
    lib = env["lib"]
    c, h, w, n, p = 64, 4, 4, 2, 2
    d = CR.planted(c, h, w, n, p, 16)
    xd, y0 = d["x"].cuda(), d["y0"].cuda()
    yd = y0.clone()
    buf = torch.full((n, 16, 64, 2), 7.0, device="cuda")

    def steps(c=c, cy=d["cy"], fused=0, slabs=0, maps=None, precision=p, w0=d["w0"]):
        return lib.esahrnet_op_cbam_steps(xd.data_ptr(), None, n, c, h, w, _ptr(w0), _ptr(d["w2"]), _ptr(d["wsa"]), 0, yd.data_ptr(),
                                          cy, d["c0"], fused, precision, slabs, buf.data_ptr(), None, maps, _stream())
    big = CR.C_REFUSED                                     # 528 channels: 544 padded, past ca_mlp's 512
    w0big = torch.zeros(big // 16, big, 1, 1)
    assert steps(c=big, cy=8 + 544 + 8, w0=w0big) != 0
    assert b"512" in lib.esahrnet_last_error()
    assert steps(fused=1, maps=buf.data_ptr()) != 0 and b"maps_out" in lib.esahrnet_last_error()
    assert steps(slabs=-1) != 0 and steps(slabs=h * w + 1) != 0 and b"slabs" in lib.esahrnet_last_error()
    assert steps(precision=3) != 0
    assert steps(c=CR.pad(264, 0), cy=8 + 288 + 8, fused=1) != 0                            # 36 groups: no power of two
    x1 = torch.zeros(n, 1, h, w, device="cuda")
    ys = torch.full((n, 64, h, w), 7.0, device="cuda")
    wz, bz, k = torch.zeros(64, 1, 3, 3), torch.zeros(64), C.c_int(-1)
    stem = lib.esahrnet_op_stem
    assert stem(x1.data_ptr(), n, h, w, _ptr(wz), _ptr(bz), 0, 1, 2, ys.data_ptr(), None, C.byref(k), _stream()) != 0
    assert stem(x1.data_ptr(), n, h, w, _ptr(wz), _ptr(bz), 0, 1, 2, ys.data_ptr(), buf.data_ptr(), None, _stream()) != 0
    assert stem(x1.data_ptr(), n, h, w, _ptr(wz), _ptr(bz), 0, 0, 3, ys.data_ptr(), None, None, _stream()) != 0
    assert stem(x1.data_ptr(), n, 0, w, _ptr(wz), _ptr(bz), 0, 0, 2, ys.data_ptr(), None, None, _stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(yd, y0) and bool((buf == 7.0).all()) and bool((ys == 7.0).all()) and k.value == -1


@pytest.mark.parametrize("case", CR.stem_cases(), ids=lambda k: f"{k[0]}x{k[1]}-{CR.PNAME[k[2]]}-{'relu' if k[3] else 'raw'}")
def test_stem_and_its_pool(env, case):
    h, w, p, relu = case
    n = 2
    cid = f"stem {h}x{w}-{CR.PNAME[p]}-{'relu' if relu else 'raw'}"
    d = CR.stem_inputs(h, w, n)
    lib = env["lib"]
    slabs = CR.stem_slabs(h, w)
    xd = d["x"].cuda()
    ys = [torch.full((n, 64, h, w), float("nan"), device="cuda") for _ in range(2)]
    part = torch.full((n, slabs, 64, 2), float("nan"), device="cuda")
    k = C.c_int(-1)
    _call(env, lib.esahrnet_op_stem(xd.data_ptr(), n, h, w, _ptr(d["w"]), _ptr(d["b"]), relu, 1, p, ys[0].data_ptr(), part.data_ptr(),
                                 C.byref(k), _stream()))
    _call(env, lib.esahrnet_op_stem(xd.data_ptr(), n, h, w, _ptr(d["w"]), _ptr(d["b"]), relu, 0, p, ys[1].data_ptr(), None, None, _stream()))
    torch.cuda.synchronize()
    y, y1, part = ys[0].cpu(), ys[1].cpu(), part.cpu()
    env["cases"] += 1
    print(f"\n{cid}: {slabs} slabs")
    assert k.value == slabs == h * -(-w // 256)
    assert torch.equal(y, y1)                                                               # pooled and unpooled: the same bits
    if p == 1:
        assert torch.equal(CR.Q[1](y), y)
    _hold(env, ("stem y", "pooled", CR.PNAME[p]), cid, y, CR.ref_stem(d["x"], d["w"], d["b"], relu),
          CR.emu_stem(d["x"], d["w"], d["b"], relu, p), CR.QUANTUM[p])
    v = y.double()
    worst = 0.0
    pieces = CR.stem_pieces(w)
    for r in range(h):
        for j, (p0, p1) in enumerate(pieces):
            s = r * len(pieces) + j
            assert torch.equal(part[:, s, :, 1], y[:, :, r, p0:p1].amax(-1)), ("slab maximum", r, j)
            b = CR.sum_bound(v[:, :, r], p0, p1)
            e = (part[:, s, :, 0].double() - v[:, :, r, p0:p1].sum(-1)).abs()
            assert bool((e <= b).all()), ("slab sum", r, j, e.max().item(), b.max().item())
            worst = max(worst, (e / b.clamp_min(1e-300)).max().item() if p1 - p0 > 1 else 0.0)
    print(f"  partial: maxima exact; worst sum error / summation bound {worst:.3f}")
    key = ("stem pool", "-", CR.PNAME[p])
    if worst > env["worst"].get(key, (0.0,))[0]:
        env["worst"][key] = (worst, 0.0, 0.0, cid)
