"""The two weight schemes of conv_x6.hip's tile-stream body agree bit for bit.

A 3x3 convolution of ONE 32-channel chunk whose workgroups never change their cout slice keeps all 27 weight fragments of
a wave in registers (the resident body, x6_body<..., WRES = true>: the stride-1 32-cout tiling); every other launch —
and every launch under ESAHRNET_X6_RELOAD_WEIGHTS=1 — refills two weight thirds per step (the reloading body).  Same
MFMAs, same operands, same order, so the outputs must be EQUAL, not close.  Which body a launch takes is decided on the
host from the layer and the grid alone; esahrnet_debug_set_x6_grid_limit caps the grid so that a workgroup walks many
items of a small tensor, and a cap that is no multiple of the number of cout slices gives the case that must NOT take
the resident body: a workgroup whose slice changes from item to item (the launcher rounds a grid above ctiles down to
a multiple of it; at or below ctiles the grid stays and the launch keeps reloading).

Against f64 the bound is test_gpu_fp32.py::test_op_conv_fp32_grade's: err <= 2 x (torch fp32 vs f64) + 2.4e-7 x scale."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SWITCH = "ESAHRNET_X6_RELOAD_WEIGHTS"

CASES = [
    # n, cin, cout, h, w, stride, relu, res
    (3, 32, 32, 20, 24, 1, True, True),          # partial tiles both ways; the resident tiling
    (2, 32, 32, 8, 8, 1, False, False),          # two items in all
    (3, 32, 64, 20, 24, 2, True, False),
    (3, 32, 128, 20, 24, 2, False, False),       # two cout slices
    (2, 32, 256, 12, 16, 2, False, False),       # four cout slices
    (2, 32, 96, 20, 24, 1, True, True),          # the resident tiling with THREE cout slices: where a changing slice would bite
]
IDS = ["x".join(map(str, c)) for c in CASES]


def _geometry(case):
    """(items, cout slices) of the case's launch: launch_x6_t's arithmetic (16-column tiles; 64-cout slices where the padded
    couts allow, else 32; rows per tile 8 at stride 1 in both tilings at two workgroups per CU, 4 at stride 2)."""
    n, cin, cout, h, w, stride, relu, res = case
    coutp = (cout + 31) // 32 * 32
    per = 64 if coutp % 64 == 0 else 32
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
    th = 4 if stride == 2 else 8
    ctiles = coutp // per
    return n * ((oh + th - 1) // th) * ((ow + 15) // 16) * ctiles, ctiles


def _limits(case):
    """Grid caps of a case: None (the default grid), one at which every workgroup walks >= 4 items (or, where the case has
    fewer than 4 items in all, ONE workgroup walks them all), and for more than one cout slice caps that are no multiple of
    ctiles — below it (the grid stays: slices change inside a workgroup) and above it (rounded down to a multiple)."""
    items, ctiles = _geometry(case)
    many = max(1, items // 4)
    many -= many % ctiles if many > ctiles else 0
    assert items // many >= min(4, items)
    out = [None, many]
    if ctiles > 1:
        out += [ctiles - 1, ctiles + 1, 1] if ctiles > 2 else [1, 3]
        assert all(v % ctiles for v in out[2:])
    return out


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, seg_hrnet2, synth
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return dict(lib=_lib.lib(), L=_lib, config=config, seg_hrnet2=seg_hrnet2, synth=synth)


@functools.lru_cache(maxsize=None)
def _data(case):
    """Inputs and the f64 / torch-f32 references of a case, made once and shared (never written to)."""
    from esa_pose_estimation_amd import synth
    n, cin, cout, h, w, stride, relu, use_res = case
    x = torch.from_numpy(synth.normal("rx", 21, (n, cin, h, w)))
    wt = torch.from_numpy(synth.normal("rw", 22, (cout, cin, 3, 3), float(np.sqrt(1.0 / (cin * 9)))))
    b = torch.from_numpy(synth.normal("rb", 23, (cout,), 0.1))
    ref = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=1)
    ref32 = F.conv2d(x, wt, b, stride=stride, padding=1)
    res = None
    if use_res:
        res = torch.from_numpy(synth.normal("rr", 24, tuple(ref.shape)))
        ref, ref32 = ref + res.double(), ref32 + res
    if relu:
        ref, ref32 = F.relu(ref), F.relu(ref32)
    return x, wt, b, res, ref, ref32


def _op_conv(env, case, limit=None):
    lib, L = env["lib"], env["L"]
    n, cin, cout, h, w, stride, relu, use_res = case
    x, wt, b, res, _, _ = _data(case)
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
    xd = x.cuda()
    rd = res.cuda() if res is not None else None
    y = torch.full((n, cout, oh, ow), float("nan"), device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.esahrnet_debug_set_x6_grid_limit(limit or 0))
    try:
        L.check(lib.esahrnet_op_conv_ex(xd.data_ptr(), n, cin, h, w, wt.numpy().ctypes.data_as(C.c_void_p),
                                        b.numpy().ctypes.data_as(C.c_void_p), cout, 3, stride, int(relu),
                                        rd.data_ptr() if rd is not None else None, y.data_ptr(), 2, stream))
    finally:
        L.check(lib.esahrnet_debug_set_x6_grid_limit(0))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_resident_and_reloading_weights_agree_bit_for_bit(env, monkeypatch, case):
    """Every grid of the case, switch off against switch on, and every capped grid against the default one (the items a
    workgroup walks change nothing in an item's arithmetic)."""
    monkeypatch.setenv(SWITCH, "1")
    base = _op_conv(env, case)
    assert torch.isfinite(base).all()
    for limit in _limits(case):
        monkeypatch.setenv(SWITCH, "1")
        reload_ = _op_conv(env, case, limit)
        monkeypatch.delenv(SWITCH)
        resident = _op_conv(env, case, limit)
        assert torch.equal(reload_, base), limit
        assert torch.equal(resident, base), limit


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_resident_weights_are_fp32_grade_and_deterministic(env, monkeypatch, case):
    monkeypatch.delenv(SWITCH, raising=False)
    _, _, _, _, ref, ref32 = _data(case)
    outs = [_op_conv(env, case) for _ in range(3)]
    err = (outs[0].double() - ref).abs().max().item()
    err32 = (ref32.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"HIP vs fp64 {err:.3e}   torch fp32 vs fp64 {err32:.3e}   scale {scale:.2f}")
    assert torch.isfinite(outs[0]).all()
    assert err <= 2.0 * err32 + 2.4e-7 * scale, (err, err32)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_merged_launch_agrees_with_the_reloading_loop(env, monkeypatch):
    """seg_hrnet2 W32, batch 2 at 64x64: the HRModules' branch convolutions share launches of conv_x6_jobs_kernel<3, 1> — the
    32-channel member takes the resident body, the 64-channel and wider ones the reloading one, side by side in one grid.
    The heat-maps must equal those of a net created under ESAHRNET_X6_RELOAD_WEIGHTS=1, and the launches must be the same."""
    outs = []
    for reload_ in (False, True):
        if reload_:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        net = env["seg_hrnet2"].get_seg_model(env["config"].make_config(widths=(32, 64, 128, 256)))
        sd = env["synth"].make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval()
        x = env["synth"].make_crops(2, 1, 64, 64, seed=0)
        with torch.no_grad():
            y, ops = net.forward_timed(x.cuda())
        outs.append((y.cpu(), [(o["kernel"], o["label"]) for o in ops]))
    merged = [lab for k, lab in outs[0][1] if k == "conv_x6_jobs_kernel<3, 1>"]
    assert merged and all(" + " in lab for lab in merged), outs[0][1]
    assert outs[0][1] == outs[1][1]
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0])
