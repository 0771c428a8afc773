"""seg_hrnet3 (CBAM) with the W48 widths (48/96/192/384) in the fp32-grade mode (precision="fp32", the default) and in split
bf16 (precision="bf16x3").  The 384-channel branch needs the CBAM channel pooling over more than 256 channels in the f32 and
split formats (cbam.hip: pool_partial).  A CBAM no kernel serves is refused when the plan is made, before any launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

W48 = (48, 96, 192, 384)
TOL_FP32 = 2e-5         # x max(1, |out|): test_gpu_fp32.py's bound for seg_hrnet3
GUARD = 2e-4            # split bf16 vs the oracle: test_gpu_parity.py's bound for seg_hrnet3


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, seg_hrnet3, synth
    from oracle import hrnet_ref
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return dict(lib=_lib.lib(), L=_lib, config=config, seg_hrnet3=seg_hrnet3, synth=synth, hrnet_ref=hrnet_ref)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _build(env, widths, seed, precision, gain=0.5):
    net = env["seg_hrnet3"].get_seg_model(env["config"].make_config(widths=widths), precision=precision)
    sd = env["synth"].make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=seed, gain=gain)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


# ------------------------------------------------------------------------------------------------ operator
def qsb(t):
    """The split-bf16 value of t: hi = bf16(t), lo = bf16(t - hi), both rounded to nearest (sb.h: split_bf16)."""
    hi = t.to(torch.bfloat16).to(torch.float32)
    return hi + (t - hi).to(torch.bfloat16).to(torch.float32)


def _cbam_exact(x, res, w0, w2, wsa, relu):
    x, w0, w2, wsa = x.double(), w0.double(), w2.double(), wsa.double()

    def fc(v):
        return F.conv2d(F.relu(F.conv2d(v, w0)), w2)
    ca = torch.sigmoid(fc(F.adaptive_avg_pool2d(x, 1)) + fc(F.adaptive_max_pool2d(x, 1)))
    u = ca * x
    sa = torch.sigmoid(F.conv2d(torch.cat([u.mean(1, keepdim=True), u.amax(1, keepdim=True)], 1), wsa, padding=3))
    y = sa * u
    if res is not None:
        y = y + res.double()
    return F.relu(y) if relu else y


# c = 384: W48's deepest branch (48 groups of 8, 5 pixel lanes); 264: a channel count that is no multiple of 32 (288 padded)
CBAM_CASES = [(c, prec, rr) for c in (384, 264) for prec in (2, 0) for rr in (False, True)]


@pytest.mark.parametrize("case", CBAM_CASES, ids=lambda c: f"c{c[0]}-{'fp32' if c[1] == 2 else 'bf16x3'}-{'res_relu' if c[2] else 'plain'}")
def test_op_cbam_over_256_channels(env, case):
    """One CBAM (pool_partial + ca_mlp + cbam_maps + cbam_apply) against the exact result on the values the format holds:
    fp32-grade within 2e-5 of the scale, split bf16 within its storage rounding (2^-15 relative) plus the same."""
    c, precision, res_relu = case
    synth, lib, L = env["synth"], env["lib"], env["L"]
    q = (lambda t: t) if precision == 2 else qsb
    n, h, w = 2, 40, 36                             # 1440 pixels: the pooling runs over 64 slabs
    cp = (c + 31) // 32 * 32
    c0 = 8
    cy = c0 + cp + 8                                # y: a wider tensor; the CBAM writes [c0, c0 + cp), the rest stays
    x = q(torch.from_numpy(synth.normal(f"wx{c}", 1, (n, c, h, w))))
    res = q(torch.from_numpy(synth.normal(f"wr{c}", 2, (n, c, h, w)))) if res_relu else None
    w0 = torch.from_numpy(synth.normal(f"w0{c}", 3, (c // 16, c, 1, 1), float(np.sqrt(1.0 / c))))
    w2 = torch.from_numpy(synth.normal(f"w2{c}", 4, (c, c // 16, 1, 1), float(np.sqrt(16.0 / c))))
    wsa = torch.from_numpy(synth.normal(f"ws{c}", 5, (1, 2, 7, 7), 0.2))
    y0 = q(torch.from_numpy(synth.normal(f"wy{c}", 6, (n, cy, h, w))))
    exact = _cbam_exact(x, res, w0, w2, wsa, res_relu)
    yd, xd, rd = y0.cuda(), x.cuda(), res.cuda() if res_relu else None       # (kept alive across the call)
    L.check(lib.esahrnet_op_cbam(xd.data_ptr(), rd.data_ptr() if res_relu else None, n, c, h, w,
                                 w0.numpy().ctypes.data_as(C.c_void_p), w2.numpy().ctypes.data_as(C.c_void_p),
                                 wsa.numpy().ctypes.data_as(C.c_void_p), int(res_relu), yd.data_ptr(), cy, c0, 0, precision,
                                 _stream()))
    torch.cuda.synchronize()
    y = yd.cpu()
    got = y[:, c0:c0 + c].double()
    bound = 2e-5 * max(1.0, exact.abs().max().item()) + (0.0 if precision == 2 else 2.0 ** -15) * exact.abs()
    err = (got - exact).abs()
    assert not bool((err > bound).any()), (err.max().item(), int((err > bound).sum()))
    assert bool((y[:, c0 + c:c0 + cp] == 0).all())                        # the padding channels: exact zeros
    assert torch.equal(y[:, :c0], y0[:, :c0]) and torch.equal(y[:, c0 + cp:], y0[:, c0 + cp:])   # outside the slice: untouched


# ------------------------------------------------------------------------------------------------ whole network
@pytest.mark.parametrize("precision, shape", [("fp32", (2, 128, 128)), ("fp32", (1, 384, 384)), ("bf16x3", (2, 128, 128))])
def test_hrnet3_w48_matches_oracle(env, precision, shape):
    net, sd = _build(env, W48, 23, precision)
    n, hh, ww = shape
    x = env["synth"].make_crops(n, 1, hh, ww, seed=23)
    cfg = env["hrnet_ref"].default_cfg(1, 30, widths=W48, variant=1)
    with torch.no_grad():
        ref = env["hrnet_ref"].forward(sd, cfg, x)
        y = net(x.cuda()).cpu()
    assert torch.isfinite(y).all()
    err = (y - ref).abs().max().item()
    print(f"seg_hrnet3 W48 {precision} {n}x{hh}x{ww}: L_inf vs the oracle {err:.3e} (|out| max {ref.abs().max().item():.2f})")
    assert err <= (TOL_FP32 * max(1.0, ref.abs().max().item()) if precision == "fp32" else GUARD), err


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_hrnet3_w48_crop_does_not_depend_on_its_batch(env, precision):
    net, _ = _build(env, W48, 29, precision)
    x = env["synth"].make_crops(3, 1, 96, 128, seed=29).cuda()
    with torch.no_grad():
        y = net(x).clone()
        y1 = net(x[1:2]).clone()
    torch.cuda.synchronize()
    assert torch.equal(y[1:2], y1)


def test_unservable_cbam_is_refused_when_the_plan_is_made(env):
    """A 520-channel branch: ca_mlp takes at most 512 (padded) channels.  The forward fails with the layer and channel
    count before its first launch, and the output buffer is left as it was."""
    lib, L = env["lib"], env["L"]
    net, _ = _build(env, (16, 16, 16, 520), 31, "fp32")
    x = env["synth"].make_crops(1, 1, 64, 64, seed=31).cuda()
    msg = "CBAM channel-attention MLP of 'stage4.0.branches.3.0' at 520 channels"
    with torch.no_grad(), pytest.raises(L.EsaHrnetError, match=msg):
        net(x)
    h = net._rt._handle_for(net, x.device)              # committed by the call above
    heat = torch.full((1, 30, 64, 64), 7.0, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = lib.esahrnet_forward(h, x.data_ptr(), 1, 64, 64, heat.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    assert rc != 0 and msg in lib.esahrnet_last_error().decode()
    torch.cuda.synchronize()
    assert bool((heat == 7.0).all())
