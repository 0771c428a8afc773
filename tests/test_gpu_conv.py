"""Every convolution launcher held to a float64 reference, kernel by kernel (conv_mfma.hip, conv_s2c32.hip, conv1x1.hip,
conv_x6.hip, bblock32.hip, stem_fused.hip), through test-only entries that say which kernel a case runs and hand back the
padding channels: esahrnet_op_conv_kernel (host: conv_kernel_name), esahrnet_op_conv_group (launch_conv, or ONE merged launch of
2 .. 6 members under the plan's job-group rule), esahrnet_op_conv_multi (launch_conv_s2c32_multi), esahrnet_op_block32
(launch_bblock32), esahrnet_op_stem2 (launch_stem_fused / launch_stem_fused_x6) and the hook esahrnet_debug_set_cu_limit, which
caps the CU count the launchers size with.  References, emulations, inputs, launch geometry and the case tables: tests/
conv_ref.py; what holds those: tests/test_conv_host.py.

The rule (tests/test_gpu_head.py and tests/test_gpu_cbam.py have the same), taken against the reference only:
    |HIP - f64|_max <= 2 x E_emu + q x max|ref|,      E_emu = max |float32 emulation of the format - f64| on the same inputs
q = conv_ref.QUANTUM[precision] (2^-17 split-bf16, 2^-9 bf16, 2^-12 fp16, 2.4e-7 fp32-grade).  The reference is F.conv2d in
float64 of the inputs the format holds, over the whole batch.  Beside the rule every output's padding channels are exact +0 and
the output is data of its format.
  single launches   every row of conv_ref.TABLE — at least one under every kernel name the dispatch can return, at the chunk
                    counts, cout slices, channel paddings and spatial classes the table's comment lists — in every precision
                    that serves it, signed and all-positive inputs; esahrnet_op_conv_kernel and the launch both report the name
                    the row is filed under (the names the build cannot reach: conv_ref.EXCLUDED, with the reason)
  CU-limit sweeps   the persistent and stream kernels of every format, the 1x1 kernels across kern2 / nsplit / the fp32-grade
                    cout slices, bblock32: three images under a limit of 1, 2, 3 CUs (a workgroup walks >= 4 items across cout
                    slices and image boundaries; the stream kernel leaves its double-buffered variant) — the rule AND the bits
                    of the unlimited launch
  merged launches   2 .. 4 (1x1 and fp32-grade: .. 6) members of unequal size, given in an order the launcher's longest-first
                    sort changes, 3x3 stride 1, 3x3 stride 2 and 1x1 in every format that merges them: each member under the rule
                    AND the bits of the same member launched alone
  multi-head        2 and 3 heads, 64- and 32-cout workgroups, mixed ReLU flags: the rule AND the bits of launch_conv_s2c32 of the
                    head alone
  bblock32, stems   the spatial classes, signed inputs and the `edge` regime (first bias +1, first weights and x >= 0: a mid
                    pixel outside the image that is not forced to zero moves y by > 100 bounds, test_conv_host.py); stem_fused on
                    each path (Coutp 64, two cout tiles a workgroup, one), cin 1 .. 4, 1 .. 3 mid chunks; stem_x6_kernel also
                    equals esahrnet_op_stem + the stride-2 convolution bit for bit
  scaling           y(2^a x, 2^b w, 2^(a+b) bias, 2^(a+b) res) == 2^(a+b) y bit for bit at (a, b) = (12, -7), (-12, 7), one row a
                    kernel family, precisions 0, 1, 2, bblock32, the stems, a multi-head launch
  refusals          every new entry: non-zero, a message, NaN-filled outputs untouched, good calls afterwards
Every case prints its error, E_emu and error / bound (run with -s); the module prints the worst per kernel or form and precision.

Measured on an MI355X: 720 cases (691 tests) in 3.1 s of case time, 5.5 s for the module; the slowest case 0.27 s (its float64
reference).  Worst error / bound per kernel and precision, with the HIP error and E_emu of that case (signed unless marked +,
the all-positive regime):
  split-bf16   conv_s2c32_kernel<1, 8, 4, false> 0.356 (2.81e-4, 2.57e-4; + 256 -> 64 20x24 res relu)   <1, 8, 2, false> 0.344 (+)
               <2, 4, 4, false> 0.357 (+ 256 -> 64 8x32)   <2, 4, 2, false> 0.336 (+)   conv_mfma_ring_kernel<1, 8, 2> 0.388 (3.32e-4,
               2.53e-4; + 512 -> 64 16x16)   <1, 16, 2> 0.405 (3.42e-4, 2.52e-4; + 480 -> 64 8x17)   conv_mfma_kernel<3, 1, 16, 2,
               true> 0.320   conv1x1_kernel 0.336   conv_mfma_kernel<1, 1, 16, 2, false> 0.350   jobs kernels 0.313 .. 0.321
               multi-head 0.335   bblock32 0.321 / edge 0.369   stem_fused 0.313 .. 0.325 / edge 0.327 .. 0.356
  bf16         stream stride 1 0.394, stride 2 0.396, conv1x1_kernel<bf16> 0.395 (all +), jobs kernels 0.388 .. 0.391
  fp16         stream stride 1 0.394, stride 2 0.396, conv1x1_kernel<fp16> 0.391 (all +), jobs kernels 0.371 .. 0.384
  fp32-grade   conv_x6_kernel<3, 1, 4, 8, 4, 2, 2> 0.456 (2.01e-5, 1.67e-5; + 480 -> 48 9x17)   <3, 2, 4, 4, 4, 2, 1> 0.450 (2.54e-5,
               2.08e-5; + 960 -> 64 9x9)   <3, 1, 2, 4, 4, 2, 2> 0.334 (+)   <3, 2, 2, 2, 4, 2, 1> 0.245 (+)   <1, 1, 4, 8, 4, 2, 2> 0.163
               <1, 1, 2, 4, 4, 2, 2> 0.189   conv1x1_x6_kernel 0.198 (+)   jobs kernels 0.115 .. 0.272   stem_x6_kernel 0.191 / 0.202
A ratio of 0.3 .. 0.4 in the stored formats means kernel and emulation round to the same value at the worst element (error ==
E_emu in most rows); the deep all-positive rows are where the f32 accumulation order shows (error up to 1.35 E_emu), and
where the fp32-grade mode comes nearest its bound — the case without cancellation that conv_x6.hip's header measures on its own.
No form needed a factor above the rule's 2 (FACTOR is empty) and no emulation needed a rounding point added after the
measurement.  Every bit-equality held at the first run: CU-limit sweeps (the source's claim "same MFMAs in the same order: a
crop's result does not depend on which one a batch size selects" — double-buffered against single-buffered stream variant,
kern2, nsplit 8 / 1 / 2 / 3, a workgroup walking 18 items, bblock32's one workgroup walking 12), merged against alone in all
four formats, multi-head against alone although the multi-head launch of 64 couts runs the wave-per-cout-tile body and the head alone the 32-cout one, the fused
fp32-grade stem against its two kernels, and the power-of-two scaling.  No defect was found in the kernels.

Teeth, each checked once on a scratch build with one arithmetic mutation that widens no index range, this module and the rest of
the GPU suite (1602 tests) run against it:
  1. bblock32.hip without the out-of-image zeroing of the mid tile (`inside || true`): all 10 test_block32 cases and both
     test_block32_does_not_depend_on_the_grid cases fail at the rule — the signed regime too (its first bias is N(0, 0.1), so
     relu(b1 + ...) outside the image is not zero either); nothing else in the module moves.  Of the existing tests 23 noticed,
     all in test_gpu_parity.py: the split-bf16 networks against their goldens and the oracle (full net, odd shapes, intermediates,
     head generations, dynamic range).  No operator test ran bblock32 before.
  2. A merged launch whose second member (in launch order) reads the first member's bias, where that has as many channels
     (launch_jobs_t, launch_x6_jobs_t, launch_conv1x1_jobs): 31 of the 34 test_merged_launch cases fail — every format, 3x3
     stride 1 and 2 and 1x1 — at the rule (asserted before the member's bit-equality with its launch alone); the three that
     pass are groups whose first member in launch order has fewer couts than the second, which the mutation's range guard leaves alone.  112
     existing tests noticed (the networks of every precision against goldens, oracles and emulations).
  3. The stream kernel's cross-item prefetch one column off (conv_s2c32_body's decode for every item but a workgroup's first
     reads gx + 1, bounds test included): the 8 stream sweep cases of the split-bf16, bf16 and fp16 formats fail at the first
     limited launch (at the rule, asserted before the bits of the unlimited launch); every single launch, merged launch and multi-head case passes, as it must — at
     these sizes and 256 CUs a workgroup has one item.  16 existing tests noticed, all at network scale (batch 32 / 64 at
     256x256 or 384x384: test_op_conv_network_scale_is_exact_and_deterministic, the W48 and batch-independence tests); none of
     the small-shape operator, golden or odd-shape tests did.
"""
import ctypes as C
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu

# (kernel or form, precision name) -> factor on E_emu where a form needed more than the rule's 2, with its case, the measured
# ratio and the reason read from the kernel's arithmetic (see the docstring)
FACTOR = {}
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    e = dict(lib=_lib.lib(), L=_lib, worst={}, t0=time.time(), cases=0, slowest=(0.0, ""))
    yield e
    e["lib"].esahrnet_debug_set_cu_limit(0)
    print(f"\n{e['cases']} cases in {time.time() - e['t0']:.1f} s, the slowest {e['slowest'][0]:.2f} s ({e['slowest'][1]}); "
          "worst error / bound per kernel or form and precision:")
    for key in sorted(e["worst"]):
        ratio, err, e_emu, cid = e["worst"][key]
        print(f"  {key[0]:<44} {key[1]:<7} {ratio:.3f}  ({err:.3e}, {e_emu:.3e}; {cid})")


@pytest.fixture(autouse=True)
def _hooks_restored(env):
    yield
    env["lib"].esahrnet_debug_set_cu_limit(0)


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


def _hold(env, key, cid, got, ref, emu, q):
    """|HIP - f64| <= factor x E_emu + q x max|ref|, printed before it is asserted."""
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (key, cid)
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    e_emu = (emu.double() - ref).abs().max().item()
    bound = FACTOR.get(key, (2.0,))[0] * e_emu + q * scale
    ratio = err / bound
    print(f"  {cid}: {key[0]} {key[1]}: HIP vs f64 {err:.3e}   E_emu {e_emu:.3e}   scale {scale:.3f}   error / bound {ratio:.3f}")
    if ratio > env["worst"].get(key, (0.0,))[0]:
        env["worst"][key] = (ratio, err, e_emu, cid)
    assert err <= bound, (key, cid, err, e_emu, scale, bound)


def _zero_bits(t):
    """Exact +0: no -0 either."""
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _check_member(env, key, cid, y, m, p):
    """One convolution's padded output: the rule on the real channels, the padding exact +0, data of its format."""
    cout = m["w"].shape[0]
    assert y.shape[1] == CR.pad(cout, p)
    assert _zero_bits(y[:, cout:]), (key, cid, "padding channels")
    assert torch.equal(CR.Q[p](y), y), (key, cid, "not data of its format")
    _hold(env, key, cid, y[:, :cout], m["ref"], m["emu"], CR.QUANTUM[p])


def _member(row, regime, p, a=0, b=0):
    d = CR.conv_data(row, regime, p, a, b)
    return dict(d, relu=int(row.relu))


def _run_group(env, members, k, stride, p, expect_rc0=True):
    """esahrnet_op_conv_group on members [dict(x, w, b, res, relu)] -> ([y f32 [n][C'][oh][ow] on the CPU], kernel name, rc)."""
    lib = env["lib"]
    cnt = len(members)
    xd = [m["x"].cuda() for m in members]
    rd = [m["res"].cuda() if m.get("res") is not None else None for m in members]
    ys = []
    for m in members:
        n, _, h, w = m["x"].shape
        oh, ow = CR.out_hw(h, w, stride)
        ys.append(torch.full((n, CR.pad(m["w"].shape[0], p), oh, ow), NAN, device="cuda"))
    I = C.c_int * cnt
    V = C.c_void_p * cnt
    name = C.create_string_buffer(96)
    rc = lib.esahrnet_op_conv_group(
        cnt, V(*[t.data_ptr() for t in xd]), I(*[m["x"].shape[0] for m in members]), I(*[m["x"].shape[1] for m in members]),
        I(*[m["x"].shape[2] for m in members]), I(*[m["x"].shape[3] for m in members]), V(*[_ptr(m["w"]).value for m in members]),
        V(*[_ptr(m["b"]).value for m in members]), I(*[m["w"].shape[0] for m in members]), k, stride, I(*[m["relu"] for m in members]),
        V(*[t.data_ptr() if t is not None else None for t in rd]), V(*[t.data_ptr() for t in ys]), p, name, 96, _stream())
    if expect_rc0:
        _call(env, rc)
    torch.cuda.synchronize()
    return [t.cpu() for t in ys], name.value.decode(), rc


def _kernel_name(env, r, p):
    buf = C.create_string_buffer(96)
    _call(env, env["lib"].esahrnet_op_conv_kernel(r.n, r.cin, r.cout, r.h, r.w, r.k, r.stride, int(r.res), p, buf, 96))
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------- single launches
@pytest.mark.parametrize("regime", CR.REGIMES)
@pytest.mark.parametrize("case", CR.single_cases(), ids=CR.case_id)
def test_single_launch(env, case, regime):
    r, p, name = case
    t0 = time.time()
    cid = f"{CR.case_id(case)}-{regime}"
    assert _kernel_name(env, r, p) == name
    m = _member(r, regime, p)
    (y,), kernel, _ = _run_group(env, [m], r.k, r.stride, p)
    assert kernel == name
    print()
    _check_member(env, (name, CR.PNAME[p]), cid, y, m, p)
    _timed(env, t0, cid)


# ---------------------------------------------------------------------------------------------- CU-limit sweeps
@pytest.mark.parametrize("case", CR.SWEEP_CASES, ids=CR.sweep_id)
def test_result_does_not_depend_on_the_launch_form(env, case):
    """The same convolution under esahrnet_debug_set_cu_limit 1, 2, 3 — persistent workgroups that walk many items across cout
    slices and image boundaries, the single-buffered stream variant, kern2, fewer cout splits — is the unlimited launch bit for
    bit, and under the rule."""
    r, p, what = case
    t0 = time.time()
    cid = CR.sweep_id(case)
    m = _member(r, "signed", p)
    (base,), name, _ = _run_group(env, [m], r.k, r.stride, p)
    print()
    _check_member(env, (name + " limit -", CR.PNAME[p]), cid, base, m, p)
    for limit in CR.CU_LIMITS:
        _call(env, env["lib"].esahrnet_debug_set_cu_limit(limit))
        try:
            (y,), name2, _ = _run_group(env, [m], r.k, r.stride, p)
        finally:
            env["lib"].esahrnet_debug_set_cu_limit(0)
        assert name2 == name
        _check_member(env, (f"{name} limit {limit}", CR.PNAME[p]), cid, y, m, p)
        assert torch.equal(y, base), (cid, limit, (y - base).abs().max().item())
    _timed(env, t0, cid)


# ---------------------------------------------------------------------------------------------- merged launches
def _merged_name(p, k, s):
    if p == 2:
        return f"conv_x6_jobs_kernel<{k}, {s}>"
    if k == 1:
        return "conv1x1_jobs_kernel"
    return f"conv_s2c32_jobs_kernel<{s}, {8 if s == 1 else 4}, {'fp16' if p == 3 else 'true' if p == 1 else 'false'}>"


@pytest.mark.parametrize("case", CR.group_cases(), ids=CR.group_id)
def test_merged_launch(env, case):
    """2 .. 6 convolutions of unequal size in ONE launch: each member under the rule and bit-equal to the same member launched
    alone."""
    p, k, s, members = case
    t0 = time.time()
    cid = CR.group_id(case)
    rows = [CR.member_row(mm, k, s) for mm in members]
    ms = [_member(r, "signed", p) for r in rows]
    ys, name, _ = _run_group(env, ms, k, s, p)
    assert name == _merged_name(p, k, s)
    print()
    for j, (r, m, y) in enumerate(zip(rows, ms, ys)):
        _check_member(env, (name, CR.PNAME[p]), f"{cid} [{j}]", y, m, p)
        (alone,), _, _ = _run_group(env, [m], k, s, p)
        assert torch.equal(y, alone), (cid, j, (y - alone).abs().max().item())
    _timed(env, t0, cid)


# ---------------------------------------------------------------------------------------------- multi-head
def _multi_inputs(case, a=0, bexp=0):
    n, cin, h, w, couts, relus = case
    tag = "mh" + "x".join(map(str, (n, cin, h, w) + couts))
    x = CR.Q[0](CR._n("x" + tag, 61, (n, cin, h, w))) * 2.0 ** a
    heads = []
    for j, (co, rl) in enumerate(zip(couts, relus)):
        wt = CR._n(f"w{j}" + tag, 62, (co, cin, 3, 3), (1.0 / (cin * 9)) ** 0.5) * 2.0 ** bexp
        b = CR._n(f"b{j}" + tag, 63, (co,), 0.1) * 2.0 ** (a + bexp)
        heads.append(dict(x=x, w=wt, b=b, res=None, relu=int(rl), ref=CR.ref_conv(0, x, wt, b, 2, None, bool(rl)),
                          emu=CR.conv(0, x, wt, b, 2, None, bool(rl))))
    return x, heads


def _run_multi(env, x, heads, expect_rc0=True):
    lib = env["lib"]
    n, cin, h, w = x.shape
    oh, ow = CR.out_hw(h, w, 2)
    nh = len(heads)
    xd = x.cuda()
    ys = [torch.full((n, m["w"].shape[0], oh, ow), NAN, device="cuda") for m in heads]
    V, I = C.c_void_p * nh, C.c_int * nh
    rc = lib.esahrnet_op_conv_multi(xd.data_ptr(), n, cin, h, w, nh, V(*[_ptr(m["w"]).value for m in heads]),
                                    V(*[_ptr(m["b"]).value for m in heads]), I(*[m["w"].shape[0] for m in heads]),
                                    I(*[m["relu"] for m in heads]), V(*[t.data_ptr() for t in ys]), _stream())
    if expect_rc0:
        _call(env, rc)
    torch.cuda.synchronize()
    return [t.cpu() for t in ys], rc


@pytest.mark.parametrize("case", CR.MULTI_CASES, ids=lambda c: f"n{c[0]}-c{c[1]}-{c[2]}x{c[3]}-" + "+".join(map(str, c[4])))
def test_multi_head(env, case):
    """launch_conv_s2c32_multi: every head under the rule, exact zeros nowhere but where ReLU puts them, and the bits of
    launch_conv_s2c32 of the head alone."""
    t0 = time.time()
    cid = "multi " + "x".join(map(str, case[:4])) + " " + "+".join(map(str, case[4]))
    x, heads = _multi_inputs(case)
    ys, _ = _run_multi(env, x, heads)
    form = "multi-head %d couts" % (64 if sum(case[4]) % 64 == 0 else 32)
    print()
    for j, (m, y) in enumerate(zip(heads, ys)):
        _check_member(env, (form, "bf16x3"), f"{cid} [{j}]", y, m, 0)
        (alone,), name, _ = _run_group(env, [m], 3, 2, 0)
        assert name.startswith("conv_s2c32_kernel<2, 4,")
        assert torch.equal(y, alone), (cid, j, (y - alone).abs().max().item())
    _timed(env, t0, cid)


# ---------------------------------------------------------------------------------------------- bblock32
def _run_block(env, d, n, h, w, expect_rc0=True):
    xd = d["x"].cuda()
    y = torch.full((n, 32, h, w), NAN, device="cuda")
    rc = env["lib"].esahrnet_op_block32(xd.data_ptr(), n, h, w, _ptr(d["w1"]), _ptr(d["b1"]), _ptr(d["w2"]), _ptr(d["b2"]),
                                        y.data_ptr(), _stream())
    if expect_rc0:
        _call(env, rc)
    torch.cuda.synchronize()
    return y.cpu(), rc


@pytest.mark.parametrize("regime", CR.REGIMES2)
@pytest.mark.parametrize("shape", CR.BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block32(env, shape, regime):
    n, h, w = shape
    t0 = time.time()
    cid = f"bblock32 {n}x{h}x{w}-{regime}"
    d = CR.block_data(n, h, w, regime)
    y, _ = _run_block(env, d, n, h, w)
    assert torch.equal(CR.Q[0](y), y)
    print()
    _hold(env, ("bblock32 " + regime, "bf16x3"), cid, y, d["ref"], d["emu"], CR.QUANTUM[0])
    _timed(env, t0, cid)


@pytest.mark.parametrize("shape", CR.SWEEP_BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_block32_does_not_depend_on_the_grid(env, shape):
    """One workgroup walking every tile of three images (cross-item prefetch) against one tile a workgroup: the same bits."""
    n, h, w = shape
    t0 = time.time()
    cid = f"bblock32 {n}x{h}x{w}-sweep"
    d = CR.block_data(n, h, w, "edge")
    base, _ = _run_block(env, d, n, h, w)
    print()
    _hold(env, ("bblock32 limit -", "bf16x3"), cid, base, d["ref"], d["emu"], CR.QUANTUM[0])
    for limit in CR.CU_LIMITS:
        _call(env, env["lib"].esahrnet_debug_set_cu_limit(limit))
        try:
            y, _ = _run_block(env, d, n, h, w)
        finally:
            env["lib"].esahrnet_debug_set_cu_limit(0)
        assert torch.equal(y, base), (cid, limit, (y - base).abs().max().item())
    _timed(env, t0, cid)


# ---------------------------------------------------------------------------------------------- fused stems
def _run_stem2(env, d, case, expect_rc0=True):
    n, cin, h, w, cmid, cout, p = case
    oh, ow = CR.out_hw(h, w, 2)
    xd = d["x"].cuda()
    y = torch.full((n, CR.pad(cout, p), oh, ow), NAN, device="cuda")
    rc = env["lib"].esahrnet_op_stem2(xd.data_ptr(), n, cin, h, w, _ptr(d["w1"]), _ptr(d["b1"]), cmid, _ptr(d["w2"]), _ptr(d["b2"]),
                                      cout, p, y.data_ptr(), _stream())
    if expect_rc0:
        _call(env, rc)
    torch.cuda.synchronize()
    return y.cpu(), rc


@pytest.mark.parametrize("regime", CR.REGIMES2)
@pytest.mark.parametrize("case", CR.STEM2_CASES, ids=lambda c: "x".join(map(str, c[:6])) + "-" + CR.PNAME[c[6]])
def test_stem2(env, case, regime):
    """stem_fused (every path) and stem_x6_kernel under the rule; the fp32-grade one also equals esahrnet_op_stem followed by
    the stride-2 convolution bit for bit (the same f32 operations in the same order, as tests/test_gpu_fp32.py claims of the
    two plans)."""
    n, cin, h, w, cmid, cout, p = case
    t0 = time.time()
    cid = "stem2 " + "x".join(map(str, case[:6])) + f"-{CR.PNAME[p]}-{regime}"
    d = CR.stem2_data(n, cin, h, w, cmid, cout, regime, p)
    y, _ = _run_stem2(env, d, case)
    assert _zero_bits(y[:, cout:]) and torch.equal(CR.Q[p](y), y)
    coutp = CR.pad(cout, p)
    form = "stem_x6_kernel" if p == 2 else "stem_fused Coutp 64" if coutp == 64 else "stem_fused 2 tiles" if (coutp // 32) % 2 == 0 else "stem_fused 1 tile"
    print()
    _hold(env, (f"{form} {regime}", CR.PNAME[p]), cid, y[:, :cout], d["ref"], d["emu"], CR.QUANTUM[p])
    if p == 2:
        xd = d["x"].cuda()
        mid = torch.full((n, 64, h, w), NAN, device="cuda")
        _call(env, env["lib"].esahrnet_op_stem(xd.data_ptr(), n, h, w, _ptr(d["w1"]), _ptr(d["b1"]), 1, 0, 2, mid.data_ptr(), None, None, _stream()))
        torch.cuda.synchronize()
        (two,), _, _ = _run_group(env, [dict(x=mid.cpu(), w=d["w2"], b=d["b2"], res=None, relu=1)], 3, 2, 2)
        assert torch.equal(y, two), (cid, (y - two).abs().max().item())
    _timed(env, t0, cid)


# ---------------------------------------------------------------------------------------------- power-of-two scaling
@pytest.mark.parametrize("ab", CR.SCALES, ids=lambda ab: f"a{ab[0]}b{ab[1]}")
def test_power_of_two_scaling(env, ab):
    """y(2^a x, 2^b w, 2^(a+b) bias, 2^(a+b) res) == 2^(a+b) y bit for bit: every rounding of these formats is scale-free away
    from under- and overflow, so a difference is a scale-dependent path."""
    a, b = ab
    t0 = time.time()
    for r, precisions in CR.SCALE_ROWS:
        for p in precisions:
            (y0,), name, _ = _run_group(env, [_member(r, "signed", p)], r.k, r.stride, p)
            (ys,), _, _ = _run_group(env, [_member(r, "signed", p, a, b)], r.k, r.stride, p)
            assert torch.equal(ys, y0 * 2.0 ** (a + b)), (name, CR.row_id(r), p, ab)
            env["cases"] += 1
    n, h, w = 2, 17, 33
    y0, _ = _run_block(env, CR.block_data(n, h, w, "signed"), n, h, w)
    ys, _ = _run_block(env, CR.block_data(n, h, w, "signed", a, b), n, h, w)
    assert torch.equal(ys, y0 * 2.0 ** a), ("bblock32", ab)
    for case in ((2, 1, 17, 31, 64, 64, 0), (2, 3, 34, 30, 64, 48, 0), (2, 1, 17, 33, 64, 128, 0), (2, 1, 17, 31, 64, 64, 2)):
        y0, _ = _run_stem2(env, CR.stem2_data(*case[:6], "signed", case[6]), case)
        ys, _ = _run_stem2(env, CR.stem2_data(*case[:6], "signed", case[6], a, b), case)
        assert torch.equal(ys, y0 * 2.0 ** (a + b)), ("stem2", case, ab)
    mc = CR.MULTI_CASES[1]
    y0, _ = _run_multi(env, *_multi_inputs(mc))
    ys, _ = _run_multi(env, *_multi_inputs(mc, a, b))
    assert all(torch.equal(u, v * 2.0 ** (a + b)) for u, v in zip(ys, y0)), ("multi-head", ab)
    _timed(env, t0, f"scaling {ab}")


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_enqueue_nothing(env):
    """Each new entry refuses a bad argument before anything is enqueued: non-zero, a message, the NaN-filled outputs untouched —
    and a good call follows."""
    lib = env["lib"]
    err = lambda: lib.esahrnet_last_error().decode(errors="replace")

    def untouched(ys):
        return all(bool(torch.isnan(y).all()) for y in ys)

    pair = lambda rows, p: [_member(r, "signed", p) for r in rows]
    K1, R = CR.K1, CR.R
    # groups the predicates reject: a merged 1x1 in a 16-bit format; three chunks in conv1x1_jobs; a stride-1 member that is no
    # stream-kernel launch on its own; a residual at stride 2; seven members
    for rows, k, s, p in (([K1(2, 64, 64, 8, 8), K1(2, 128, 64, 8, 8)], 1, 1, 1), ([K1(2, 64, 64, 8, 8), K1(2, 96, 64, 8, 8)], 1, 1, 0),
                          ([R(2, 64, 64, 34, 30), R(2, 64, 64, 16, 16)], 3, 1, 0),
                          ([CR.S2(2, 64, 64, 17, 31), CR.S2(2, 64, 64, 9, 9, res=True)], 3, 2, 3)):
        ys, _, rc = _run_group(env, pair(rows, p), k, s, p, expect_rc0=False)
        assert rc != 0 and "no merged launch" in err() and untouched(ys), (rows, err())
    m = _member(K1(1, 64, 64, 8, 8, res=True), "signed", 1)                    # the 16-bit 1x1 has no residual form
    ys, _, rc = _run_group(env, [m], 1, 1, 1, expect_rc0=False)
    assert rc != 0 and "no kernel" in err() and untouched(ys)
    ys, _, rc = _run_group(env, [_member(R(1, 32, 32, 8, 8), "signed", 0)], 3, 3, 0, expect_rc0=False)
    assert rc != 0 and "unsupported" in err() and untouched(ys)
    ys, _, rc = _run_group(env, [_member(R(1, 32, 32, 8, 8), "signed", 0)], 3, 1, 4, expect_rc0=False)
    assert rc != 0 and "precision" in err() and untouched(ys)
    assert lib.esahrnet_op_conv_group(1, None, None, None, None, None, None, None, None, 3, 1, None, None, None, 0, None, 0, _stream()) != 0
    assert "null" in err()
    # multi-head: a head of 48 couts, four heads, a null input
    x, heads = _multi_inputs((1, 32, 9, 9, (32, 48), (0, 1)))
    ys, rc = _run_multi(env, x, heads, expect_rc0=False)
    assert rc != 0 and "multiple of 32" in err() and untouched(ys)
    x, heads = _multi_inputs((1, 32, 9, 9, (32, 32, 32, 32), (0, 1, 0, 1)))
    ys, rc = _run_multi(env, x, heads, expect_rc0=False)
    assert rc != 0 and "nheads" in err() and untouched(ys)
    assert lib.esahrnet_op_conv_multi(None, 1, 32, 9, 9, 2, None, None, None, None, None, _stream()) != 0 and "null" in err()
    # bblock32: an empty image, a null weight pointer
    d = CR.block_data(1, 16, 16, "signed")
    y, rc = _run_block(env, d, 1, 0, 16, expect_rc0=False)
    assert rc != 0 and untouched([y])
    yd = torch.full((1, 32, 16, 16), NAN, device="cuda")
    assert lib.esahrnet_op_block32(d["x"].cuda().data_ptr(), 1, 16, 16, None, _ptr(d["b1"]), _ptr(d["w2"]), _ptr(d["b2"]), yd.data_ptr(), _stream()) != 0
    assert "null" in err() and untouched([yd])
    # the fused stem: cin 5; the fp32-grade kernel with two input channels or 32 mid channels; a 16-bit precision; cmid 48
    for case, what in (((1, 5, 9, 9, 64, 64, 0), "cin"), ((1, 2, 9, 9, 64, 64, 2), "stem_x6_kernel"), ((1, 1, 9, 9, 32, 64, 2), "stem_x6_kernel"),
                       ((1, 1, 9, 9, 64, 64, 1), "precision"), ((1, 1, 9, 9, 48, 64, 0), "cmid")):
        d = CR.stem2_data(*case[:6], "signed", 0)
        y, rc = _run_stem2(env, d, case, expect_rc0=False)
        assert rc != 0 and what in err() and untouched([y]), (case, err())
    assert lib.esahrnet_op_stem2(None, 1, 1, 9, 9, None, None, 64, None, None, 64, 0, None, _stream()) != 0 and "null" in err()
    torch.cuda.synchronize()
    # and good calls follow
    m = _member(R(2, 64, 64, 17, 33), "signed", 0)
    (y,), _, _ = _run_group(env, [m], 3, 1, 0)
    assert bool(torch.isfinite(y).all())
    d = CR.block_data(1, 16, 16, "signed")
    y, _ = _run_block(env, d, 1, 16, 16)
    assert bool(torch.isfinite(y).all())
