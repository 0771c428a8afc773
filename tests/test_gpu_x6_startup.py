"""How a workgroup's stream starts changes no bit (conv_x6.hip: the prologue of x6_body in all its forms; the fused stem and
conv1x1_x6_kernel, whose starts are serial, pass through the same checks).

A workgroup of the tile-stream kernels stages the tile of its FIRST step in the prologue — every load of the start issued
back to back, the tile waited for with a counted vmcnt while the weights are still in flight — and the tiles of all later
steps inside the step loop.  An item's arithmetic does not depend on who walks it, so two launches of one convolution must
give EQUAL outputs:
  * the default grid — on these small tensors one workgroup per item: every item is staged by a prologue;
  * the grid capped (esahrnet_debug_set_x6_grid_limit) at one workgroup per cout slice: only a slice's first item is
    staged by a prologue, the loop stages the rest.
The caps keep the launcher's slice rule (a grid above the number of cout slices is a multiple of it); the eight-chunk case
adds caps of 3 and 5 workgroups: below the number of slices the slice changes inside a workgroup, above it the grid is
rounded down.  The shapes are the smallest that reach each start-up path; see CASES.

Against f64 the bound is test_gpu_fp32.py::test_op_conv_fp32_grade's: err <= 2 x (torch fp32 vs f64) + 2.4e-7 x scale."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [
    # n, cin, cout, h, w, k, stride, relu, res
    (1, 32, 32, 8, 16, 3, 1, True, True),         # one item, one step: the prologue is the only staging; resident body
    (2, 32, 32, 20, 24, 3, 1, True, True),        # partial tiles both ways; out-of-range units in both halves of the tile
    (2, 64, 64, 12, 20, 3, 1, True, True),        # reloading body, two chunks: step parity 0 / 1; third 0 from the prologue
    (1, 96, 64, 9, 17, 3, 1, False, False),       # three chunks: the stream ends on odd parity; a one-column tile
    (2, 256, 256, 8, 16, 3, 1, True, True),       # four cout slices, eight chunks; also capped at 3 and 5 workgroups
    (2, 32, 64, 20, 24, 3, 2, True, False),       # single-buffer stride 2, the 64-cout tiling
    (2, 32, 32, 20, 24, 3, 2, True, False),       # single-buffer stride 2, the 32-cout tiling
    (1, 32, 256, 8, 8, 3, 2, False, False),       # stride 2, one step per workgroup, four slices
    (2, 64, 32, 12, 20, 1, 1, False, False),      # the 1x1 form of x6_body
    (2, 256, 480, 8, 8, 1, 1, False, False),      # conv1x1_x6_kernel with cout slices (its grid is not capped: the pixels' rule)
]
IDS = ["x".join(map(str, c)) for c in CASES]
EXTRA_CAPS = {(2, 256, 256, 8, 16, 3, 1, True, True): [3, 5]}


def _geometry(case):
    """(items, cout slices) of the case's tile-stream launch: launch_x6_t's arithmetic (16-column tiles; 64-cout slices where
    the padded couts allow, else 32; 8 rows per tile at stride 1, 4 at stride 2)."""
    n, cin, cout, h, w, k, stride, relu, res = case
    coutp = (cout + 31) // 32 * 32
    per = 64 if coutp % 64 == 0 else 32
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
    th = 4 if stride == 2 else 8
    ctiles = coutp // per
    return n * ((oh + th - 1) // th) * ((ow + 15) // 16) * ctiles, ctiles


def _limits(case):
    """Grid caps of a case: one workgroup per cout slice (a workgroup walks its slice's items, the first one from the
    prologue), two per slice where the case has the items for it, and the case's extra caps."""
    items, ctiles = _geometry(case)
    assert items <= 512, case        # the default grid is one workgroup per item on any chip of 256 CUs and more
    out = [ctiles]
    if items >= 4 * ctiles:
        out.append(2 * ctiles)
    assert all(v % ctiles == 0 for v in out)
    return out + EXTRA_CAPS.get(case, [])


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, seg_hrnet2, synth
    from oracle import hrnet_ref
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return dict(lib=_lib.lib(), L=_lib, config=config, seg_hrnet2=seg_hrnet2, synth=synth, hrnet_ref=hrnet_ref)


@functools.lru_cache(maxsize=None)
def _data(case):
    """Inputs and the f64 / torch-f32 references of a case, made once and shared (never written to)."""
    from esa_pose_estimation_amd import synth
    n, cin, cout, h, w, k, stride, relu, use_res = case
    x = torch.from_numpy(synth.normal("sx", 31, (n, cin, h, w)))
    wt = torch.from_numpy(synth.normal("sw", 32, (cout, cin, k, k), float(np.sqrt(1.0 / (cin * k * k)))))
    b = torch.from_numpy(synth.normal("sb", 33, (cout,), 0.1))
    ref = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=(k - 1) // 2)
    ref32 = F.conv2d(x, wt, b, stride=stride, padding=(k - 1) // 2)
    res = None
    if use_res:
        res = torch.from_numpy(synth.normal("sr", 34, tuple(ref.shape)))
        ref, ref32 = ref + res.double(), ref32 + res
    if relu:
        ref, ref32 = F.relu(ref), F.relu(ref32)
    return x, wt, b, res, ref, ref32


def _op_conv(env, case, limit=None):
    lib, L = env["lib"], env["L"]
    n, cin, cout, h, w, k, stride, relu, use_res = case
    x, wt, b, res, _, _ = _data(case)
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
    xd = x.cuda()
    rd = res.cuda() if res is not None else None
    y = torch.full((n, cout, oh, ow), float("nan"), device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.esahrnet_debug_set_x6_grid_limit(limit or 0))
    try:
        L.check(lib.esahrnet_op_conv_ex(xd.data_ptr(), n, cin, h, w, wt.numpy().ctypes.data_as(C.c_void_p),
                                        b.numpy().ctypes.data_as(C.c_void_p), cout, k, stride, int(relu),
                                        rd.data_ptr() if rd is not None else None, y.data_ptr(), 2, stream))
    finally:
        L.check(lib.esahrnet_debug_set_x6_grid_limit(0))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_prologue_staged_and_loop_staged_items_agree_bit_for_bit(env, case):
    base = _op_conv(env, case)
    assert torch.isfinite(base).all()
    for limit in _limits(case):
        assert torch.equal(_op_conv(env, case, limit), base), limit


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_start_is_fp32_grade_and_deterministic(env, case):
    _, _, _, _, ref, ref32 = _data(case)
    err32 = (ref32.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    for limit in [None] + _limits(case)[:1]:
        a, b = _op_conv(env, case, limit), _op_conv(env, case, limit)
        err = (a.double() - ref).abs().max().item()
        print(f"limit {limit}: HIP vs fp64 {err:.3e}   torch fp32 vs fp64 {err32:.3e}   scale {scale:.2f}")
        assert torch.isfinite(a).all()
        assert err <= 2.0 * err32 + 2.4e-7 * scale, (limit, err, err32)
        assert torch.equal(a, b), limit


def test_forward_with_few_workgroups_equals_the_default_grid(env):
    """seg_hrnet2 W32, batch 2 at 64x64, fp32: stem_x6_kernel, and conv_x6_jobs_kernel<3, 1>, <3, 2> and <1, 1> with both
    tilings in one launch.  With every tile-stream launch (every member of a merged one) capped at 4 workgroups nearly all
    items are staged by the loop; with the default grid nearly all by a prologue.  Equal heat-maps, within the net's oracle
    bound (test_gpu_fp32.py::test_odd_shapes_match_oracle: 2e-5)."""
    lib, L = env["lib"], env["L"]
    net = env["seg_hrnet2"].get_seg_model(env["config"].make_config(widths=(32, 64, 128, 256)), precision="fp32")
    sd = env["synth"].make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    x = env["synth"].make_crops(2, 1, 64, 64, seed=0)
    outs = []
    for limit in (0, 4):
        L.check(lib.esahrnet_debug_set_x6_grid_limit(limit))
        try:
            with torch.no_grad():
                y, ops = net.forward_timed(x.cuda())
            torch.cuda.synchronize()
        finally:
            L.check(lib.esahrnet_debug_set_x6_grid_limit(0))
        outs.append(y.cpu())
        kernels = {o["kernel"] for o in ops}
        assert {"stem_x6_kernel", "conv_x6_jobs_kernel<3, 1>", "conv_x6_jobs_kernel<3, 2>", "conv_x6_jobs_kernel<1, 1>"} <= kernels, kernels
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    with torch.no_grad():
        ref = env["hrnet_ref"].forward(sd, env["hrnet_ref"].default_cfg(1, 11), x)
    err = (outs[0] - ref).abs().max().item()
    print(f"heat-map Linf vs the CPU oracle {err:.3e}")
    assert err <= 2e-5, err
