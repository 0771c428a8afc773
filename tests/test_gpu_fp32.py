"""GPU parity of the fp32-grade mode (esahrnet_cfg.precision = 2, `precision="fp32"` — the DEFAULT of seg_hrnet /
seg_hrnet2 and the mode of BASELINE.json configs[1] / configs[2]: "HRNet-W32 256x256 batch=32, fp32").

Arithmetic under test (conv_x6.hip): f32 NHWC activations, every operand split EXACTLY into three bf16 terms, six
v_mfma_f32_16x16x32_bf16 per product, f32 accumulation.  The bar: the HIP path must be as close to an
fp64 evaluation of the oracle as the reference's own fp32 CPU forward is — HIP-vs-fp64 <= 2 x (fp32 reference vs fp64)
at EVERY weight gain incl. He init (g = 2.0), and <= 2e-5 x scale on the goldens of the real reference."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-3          # contractual (north_star): heat-map L_inf vs the reference CPU forward


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, inference, seg_hrnet, seg_hrnet2, seg_hrnet3, synth
    from oracle import hrnet_ref, keypoints_ref
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return dict(lib=_lib.lib(), L=_lib, config=config, inference=inference, seg_hrnet=seg_hrnet,
                seg_hrnet2=seg_hrnet2, seg_hrnet3=seg_hrnet3, synth=synth, hrnet_ref=hrnet_ref, kref=keypoints_ref)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _build(env, variant, widths, seed, gain=0.5, precision="fp32", **kw):
    net = env[variant].get_seg_model(env["config"].make_config(widths=widths), precision=precision, **kw)
    sd = env["synth"].make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=seed, gain=gain)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


def test_fp32_is_the_default_and_not_an_alias_of_bf16x3(env):
    from esa_pose_estimation_amd import hrnet
    assert hrnet.PRECISIONS["fp32"] == hrnet.PRECISIONS["bf16x6"] == 2
    assert hrnet.PRECISIONS["bf16x3"] == 0 and hrnet.PRECISIONS["bf16"] == 1
    net = env["seg_hrnet2"].get_seg_model(env["config"].make_config(widths=(8, 16, 32, 64)))
    assert net._cfg_struct.precision == 2


# ------------------------------------------------------------------------------------- operators
CONV_CASES = [
    # n, cin, cout, h, w, k, stride, relu, res
    (2, 32, 32, 32, 32, 3, 1, True, True),
    (1, 64, 64, 16, 48, 3, 1, True, False),
    (1, 32, 64, 32, 32, 3, 2, True, False),
    (2, 64, 64, 34, 30, 3, 2, False, False),      # odd-ish sizes, stride 2, partial tiles
    (1, 128, 32, 16, 16, 1, 1, False, False),
    (1, 96, 480, 8, 8, 1, 1, False, True),
    (1, 48, 11, 20, 24, 1, 1, True, False),       # channel padding on both sides
    (1, 8, 16, 18, 22, 3, 1, True, True),         # tiny widths
    (3, 256, 256, 16, 16, 3, 1, True, True),      # deepest branch shape: 128-cout slices, 8 chunks
    (1, 32, 32, 7, 5, 3, 1, False, False),        # image smaller than a tile
    (2, 128, 128, 32, 32, 3, 1, True, True),      # 4 chunks
    (1, 480, 11, 24, 40, 1, 1, True, False),      # last_layer[3]: 15 chunks
    (1, 32, 480, 24, 24, 1, 1, False, False),     # last_layer[0] slice of branch 0: 15 cout slices
    (2, 32, 128, 17, 31, 3, 2, False, False),     # fuse-down link with width change, odd size
    (1, 64, 256, 32, 32, 3, 2, True, False),
    (1, 256, 32, 16, 16, 1, 1, False, False),     # fuse-up 1x1
]


def _op_conv(env, x, wt, b, stride, relu, res, precision=2):
    lib, L = env["lib"], env["L"]
    n, cin, h, w = x.shape
    cout, _, k, _ = wt.shape
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
    xd = x.cuda()
    rd = res.cuda() if res is not None else None
    y = torch.full((n, cout, oh, ow), float("nan"), device="cuda")
    wn, bn = wt.numpy(), b.numpy()
    L.check(lib.esahrnet_op_conv_ex(xd.data_ptr(), n, cin, h, w, wn.ctypes.data_as(C.c_void_p),
                                    bn.ctypes.data_as(C.c_void_p), cout, k, stride, int(relu),
                                    rd.data_ptr() if rd is not None else None, y.data_ptr(), precision, _stream()))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_op_conv_fp32_grade(env, case):
    """HIP vs an fp64 convolution; beside it the error of torch's own fp32 CPU convolution on the same data.
    fp32-grade = no worse than twice the fp32 reference's error (plus one output ulp of slack for tiny cases)."""
    n, cin, cout, h, w, k, stride, relu, use_res = case
    synth = env["synth"]
    x = torch.from_numpy(synth.normal("opx", 1, (n, cin, h, w)))
    wt = torch.from_numpy(synth.normal("opw", 2, (cout, cin, k, k), float(np.sqrt(1.0 / (cin * k * k)))))
    b = torch.from_numpy(synth.normal("opb", 3, (cout,), 0.1))
    ref = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=(k - 1) // 2)
    ref32 = F.conv2d(x, wt, b, stride=stride, padding=(k - 1) // 2)
    res = None
    if use_res:
        res = torch.from_numpy(synth.normal("opr", 4, tuple(ref.shape)))
        ref = ref + res.double()
        ref32 = ref32 + res
    if relu:
        ref, ref32 = F.relu(ref), F.relu(ref32)
    y = _op_conv(env, x, wt, b, stride, relu, res)
    err = (y.double() - ref).abs().max().item()
    err32 = (ref32.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"HIP vs fp64 {err:.3e}   torch fp32 vs fp64 {err32:.3e}   scale {scale:.2f}")
    assert torch.isfinite(y).all()
    assert err <= 2.0 * err32 + 2.4e-7 * scale, (err, err32)


STREAM_CASES = [
    # network-scale launches: every workgroup walks several (item, chunk) steps, double-buffered tiles, weight reloads
    # n, cin, cout, h, w, stride, relu, res
    (32, 64, 64, 64, 64, 1, True, True),          # 64 couts: 16-row tiles, 2 chunks, residual
    (32, 32, 32, 128, 128, 1, True, True),        # 32 couts: single chunk, weights stay in registers
    (16, 128, 128, 32, 32, 1, True, True),        # 128 couts: 4 chunks
    (32, 256, 256, 16, 16, 1, True, False),       # 2 cout slices, 8 chunks
    (16, 64, 64, 128, 128, 2, True, False),       # stride 2
    (16, 32, 32, 128, 128, 2, False, False),
    (8, 480, 32, 128, 128, 1, True, False),       # 1x1, 15 chunks (last_layer[3] at network size)
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_op_conv_network_scale_is_fp32_grade_and_deterministic(env, case):
    n, cin, cout, h, w, stride, relu, use_res = case
    k = 1 if cin == 480 else 3
    synth = env["synth"]
    x = torch.from_numpy(synth.normal("sx", 11, (n, cin, h, w)))
    wt = torch.from_numpy(synth.normal("sw", 12, (cout, cin, k, k), float(np.sqrt(1.0 / (cin * k * k)))))
    b = torch.from_numpy(synth.normal("sb", 13, (cout,), 0.1))
    ref32 = F.conv2d(x, wt, b, stride=stride, padding=(k - 1) // 2)
    res = None
    if use_res:
        res = torch.from_numpy(synth.normal("sr", 14, tuple(ref32.shape)))
        ref32 = ref32 + res
    if relu:
        ref32 = F.relu(ref32)
    outs = [_op_conv(env, x, wt, b, stride, relu, res) for _ in range(3)]
    # fp64 on a slice of the batch (the full fp64 convolution of the big cases takes minutes on the CPU)
    m = min(n, 2)
    ref = F.conv2d(x[:m].double(), wt.double(), b.double(), stride=stride, padding=(k - 1) // 2)
    if use_res:
        ref = ref + res[:m].double()
    if relu:
        ref = F.relu(ref)
    err = (outs[0][:m].double() - ref).abs().max().item()
    err32 = (ref32[:m].double() - ref).abs().max().item()
    full = (outs[0] - ref32).abs().max().item()
    print(f"HIP vs fp64 {err:.3e}   torch fp32 vs fp64 {err32:.3e}   HIP vs torch fp32 (whole batch) {full:.3e}")
    assert err <= 2.0 * err32 + 1e-7, (err, err32)
    assert full <= 4.0 * err32 + 1e-6, full
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_op_fuse_fp32(env):
    synth, lib, L = env["synth"], env["lib"], env["L"]
    n, c, h, w = 2, 40, 24, 40
    sizes = [(24, 40), (12, 20), (6, 10), (3, 5)]
    xs = [torch.from_numpy(synth.normal(f"fx{i}", 5, (n, c, a, b))) for i, (a, b) in enumerate(sizes)]
    ref = xs[0].clone()
    for t in xs[1:]:
        ref = ref + F.interpolate(t, size=(h, w), mode="bilinear", align_corners=False)
    ref = F.relu(ref)
    xd = [t.cuda() for t in xs]
    ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in xd])
    hs = (C.c_int * 4)(*[s[0] for s in sizes])
    ws = (C.c_int * 4)(*[s[1] for s in sizes])
    y = torch.empty((n, c, h, w), device="cuda")
    L.check(lib.esahrnet_op_fuse_ex(ptrs, hs, ws, 4, n, c, h, w, 1, y.data_ptr(), 2, _stream()))
    torch.cuda.synchronize()
    assert (y.cpu() - ref).abs().max().item() <= 2e-6


# ------------------------------------------------------------------------------------- full net
GOLDEN = ["tiny_hrnet2_64", "tiny_hrnet_64", "w32_hrnet2_128", "w32_hrnet2_256", "w32_hrnet_256",
          "w32_hrnet2_128_g1", "w32_hrnet2_256_g1",
          "small_hrnet3_64", "w32_hrnet3_128"]      # seg_hrnet3 (CBAM: the network val.py:380 runs), SURVEY.md §8a row a18


@pytest.mark.parametrize("tag", GOLDEN)
def test_full_net_matches_reference_golden(env, golden_dir, tag):
    """HIP forward vs the output of the REAL reference model (tests/golden/make_golden.py): <= 2e-5 x scale."""
    g = np.load(os.path.join(golden_dir, tag + ".npz"), allow_pickle=False)
    variant = str(g["variant"])
    gain = float(g["gain"]) if "gain" in g.files else 0.5
    net, sd = _build(env, variant, tuple(int(v) for v in g["widths"]), int(g["seed"]), gain)
    cin = 3 if variant == "seg_hrnet" else 1
    x = env["synth"].make_crops(int(g["n"]), cin, int(g["hw"]), int(g["hw"]), seed=int(g["seed"]))
    with torch.no_grad():
        y = net(x.cuda()).cpu().numpy()
    s = int(g["subsample"])
    err = np.abs(y[:, :, ::s, ::s] - g["out"]).max()
    scale = max(1.0, float(g["out_absmax"]))
    print(f"{tag}: Linf vs reference {err:.3e} (absmax {float(g['out_absmax']):.3f}, reference fp32-vs-fp64 "
          f"{float(g['fp32_vs_fp64_linf']):.2e})")
    assert np.isfinite(y).all()
    assert err <= TOL
    assert err <= 2e-5 * scale, err
    # the reference's output carries its own fp32 noise: we must be as close to it as two fp32 evaluations are to each other
    assert err <= 4.0 * float(g["fp32_vs_fp64_linf"]) + 1e-6, err
    flat = y.reshape(y.shape[0], y.shape[1], -1)
    assert np.array_equal(flat.argmax(-1), g["plane_argmax"])


def test_dynamic_range_sweep_all_gains(env):
    """VERDICT r2 #1 'done' criterion: at W32 128x128, weight gains 0.5 / 1.0 / 1.5 / 2.0 (He init: |act| ~ 8.5e3), the
    HIP forward is at most 2x as far from an fp64 evaluation of the oracle as the fp32 CPU reference itself."""
    cfg = env["hrnet_ref"].default_cfg(1, 11)
    x = env["synth"].make_crops(1, 1, 128, 128, seed=3)
    rows = []
    for gain in (0.5, 1.0, 1.5, 2.0):
        net, sd = _build(env, "seg_hrnet2", (32, 64, 128, 256), 3, gain)
        taps = {}
        with torch.no_grad():
            ref64 = env["hrnet_ref"].forward(sd, cfg, x.double(), taps)
            ref32 = env["hrnet_ref"].forward(sd, cfg, x)
            y = net(x.cuda()).cpu().double()
        act = max(float(t.abs().max()) for t in taps.values())
        rows.append((gain, act, float(ref64.abs().max()), float((y - ref64).abs().max()),
                     float((ref32.double() - ref64).abs().max())))
    print("gain  max|act|  max|out|  HIP-vs-fp64  fp32ref-vs-fp64  ratio")
    for g_, act, out, e, e32 in rows:
        print(f"{g_:4.1f}  {act:8.1f}  {out:8.2f}  {e:11.3e}  {e32:15.3e}  {e / e32:5.2f}")
    for g_, act, out, e, e32 in rows:
        assert e <= 2.0 * e32, (g_, e, e32)
        if g_ <= 1.5:
            assert e <= TOL, (g_, e)


def test_intermediate_tensors_match_oracle(env):
    net, sd = _build(env, "seg_hrnet2", (32, 64, 128, 256), 4)
    x = env["synth"].make_crops(1, 1, 96, 64, seed=4)
    taps_ref = {}
    with torch.no_grad():
        out_ref = env["hrnet_ref"].forward(sd, env["hrnet_ref"].default_cfg(1, 11), x, taps_ref)
        taps = net.taps(x.cuda())
    torch.cuda.synchronize()
    worst = 0.0
    assert {"stem2", "layer1", "stage2.0", "stage3.2", "stage4.0", "stage4.3"} <= set(taps)
    for name, ref in taps_ref.items():
        if name not in taps:
            continue
        got = taps[name].cpu()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = (got - ref).abs().max().item()
        worst = max(worst, err / max(1.0, ref.abs().max().item()))
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (name, err)
    assert (taps["heatmaps"].cpu() - out_ref).abs().max().item() <= 2e-5
    print(f"worst intermediate Linf / scale {worst:.3e} over {len(taps_ref)} tensors")


@pytest.mark.parametrize("hw", [(48, 80), (40, 56), (16, 16), (18, 34), (104, 72), (128, 160)])
def test_odd_shapes_match_oracle(env, hw):
    net, sd = _build(env, "seg_hrnet2", (32, 64, 128, 256), 6)
    x = env["synth"].make_crops(2, 1, hw[0], hw[1], seed=6)
    with torch.no_grad():
        ref = env["hrnet_ref"].forward(sd, env["hrnet_ref"].default_cfg(1, 11), x)
        y = net(x.cuda()).cpu()
    assert (y - ref).abs().max().item() <= 2e-5


def test_batch32_properties_and_golden(env, golden_dir):
    """BASELINE configs[1] (W32, 256x256, batch 32, fp32): every sample equals its own batch-1 forward bit for bit,
    sample 0 matches the reference's golden output, permutation equivariance, input untouched."""
    g = np.load(os.path.join(golden_dir, "w32_hrnet2_256.npz"), allow_pickle=False)
    net, sd = _build(env, "seg_hrnet2", (32, 64, 128, 256), 0)
    synth = env["synth"]
    x0 = synth.make_crops(1, 1, 256, 256, seed=0)
    rest = synth.make_crops(31, 1, 256, 256, seed=123)
    x = torch.cat([x0, rest]).cuda()
    xc = x.clone()
    with torch.no_grad():
        y = net(x)
        y_single = [net(x[i:i + 1]) for i in (0, 7, 31)]
    torch.cuda.synchronize()
    assert torch.equal(x, xc)
    for i, ys in zip((0, 7, 31), y_single):
        assert torch.equal(y[i:i + 1], ys), i
    err = np.abs(y[0:1].cpu().numpy() - g["out"]).max()
    assert err <= 2e-5, err
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad():
        yp = net(x[perm])
    assert torch.equal(yp, y[perm])
    kp = env["inference"].heatmaps_to_keypoints(y)
    assert kp.shape == (32, 11, 3) and bool(torch.isfinite(kp).all())


def test_graph_capture_replays_and_weight_edits_are_seen(env):
    net, sd = _build(env, "seg_hrnet2", (16, 32, 64, 128), 2)
    x = env["synth"].make_crops(4, 1, 64, 64, seed=2).cuda()
    with torch.no_grad():
        y0 = net(x).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(x)
        torch.cuda.current_stream().wait_stream(s)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            yg = net(x)
        gph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, y0)
        # an in-place edit of ONE non-sentinel tensor, no invalidate_weights(): the next forward must see it
        dict(net.named_parameters())["last_layer.3.weight"].mul_(0.5)
        y1 = net(x)
        torch.cuda.synchronize()
        assert not torch.equal(y1, y0)


@pytest.mark.parametrize("unfused", [False, True])
def test_fused_head_and_its_materialised_alternative(env, golden_dir, monkeypatch, unfused):
    """head_x6.hip (W0, interpolation of the low-resolution slices, ReLU, last_layer[3] in one kernel) and the op-by-op
    alternative (slice 0 + fuse + 1x1: the 480-channel tensors materialised) must both reproduce the reference; the op
    list says which one ran.  Odd level sizes whose interpolation windows do not fit the fused kernel fall back per shape."""
    if unfused:
        monkeypatch.setenv("ESAHRNET_X6_UNFUSED_HEAD", "1")
    g = np.load(os.path.join(golden_dir, "w32_hrnet2_128.npz"), allow_pickle=False)
    net, sd = _build(env, "seg_hrnet2", tuple(int(v) for v in g["widths"]), int(g["seed"]))
    x = env["synth"].make_crops(int(g["n"]), 1, int(g["hw"]), int(g["hw"]), seed=int(g["seed"]))
    with torch.no_grad():
        y, ops = net.forward_timed(x.cuda())
        taps = net.taps(x.cuda())
    kernels = [o["kernel"] for o in ops]
    assert ("head_x6" in kernels) == (not unfused), kernels
    assert ("head0" in taps) == unfused
    err = np.abs(y.cpu().numpy() - g["out"]).max()
    print(f"{'materialised' if unfused else 'fused'} head: Linf vs reference {err:.3e}, {len(ops)} launches")
    assert err <= 2e-5, err
    if unfused:
        cfg = env["hrnet_ref"].default_cfg(1, 11)
        tr = {}
        env["hrnet_ref"].forward(sd, cfg, x, tr)
        for name in ("head0", "head3"):
            assert (taps[name].cpu() - tr[name]).abs().max().item() <= 2e-5 * max(1.0, tr[name].abs().max().item()), name


@pytest.mark.parametrize("no_jobs", [False, True])
def test_merged_branch_launches_and_their_fallback(env, golden_dir, monkeypatch, no_jobs):
    """The same-depth 3x3 convolutions of an HRModule's branches, the same-depth links of its fuse-down chains and its
    fuse-up 1x1s are independent (models/seg_hrnet.py:143-220) and run as ONE launch of conv_x6_jobs_kernel each;
    ESAHRNET_NO_JOBS=1 keeps one launch per convolution.  Same items, same order, same bits: the two plans must agree
    bit for bit, and both with the reference."""
    g = np.load(os.path.join(golden_dir, "w32_hrnet2_128.npz"), allow_pickle=False)
    x = env["synth"].make_crops(int(g["n"]), 1, int(g["hw"]), int(g["hw"]), seed=int(g["seed"]))
    outs = {}
    for nj in (no_jobs, not no_jobs):
        if nj:
            monkeypatch.setenv("ESAHRNET_NO_JOBS", "1")
        else:
            monkeypatch.delenv("ESAHRNET_NO_JOBS", raising=False)
        net, sd = _build(env, "seg_hrnet2", tuple(int(v) for v in g["widths"]), int(g["seed"]))
        with torch.no_grad():
            y, ops = net.forward_timed(x.cuda())
        kernels = [o["kernel"] for o in ops]
        merged = [o for o in ops if o["kernel"].startswith("conv_x6_jobs_kernel")]
        assert bool(merged) == (not nj), kernels
        assert all(" + " in o["label"] and o["flops"] > 0 for o in merged)
        outs[nj] = (y.cpu(), len(ops))
    print(f"launches: merged plan {outs[False][1]}, one per convolution {outs[True][1]}")
    assert outs[False][1] < outs[True][1]
    assert torch.equal(outs[False][0], outs[True][0])
    assert np.abs(outs[no_jobs][0].numpy() - g["out"]).max() <= 2e-5


def test_fused_stem_is_bit_identical_to_conv1_then_conv2(env, golden_dir, monkeypatch):
    """stem_x6_kernel forms conv1 + bn1 + ReLU inside conv2's staging (the 64-channel full-resolution tensor is never written):
    same f32 operations in the same order as stem_kernel, so the two plans agree bit for bit; seg_hrnet (3-channel crops)
    keeps the two-kernel stem."""
    g = np.load(os.path.join(golden_dir, "w32_hrnet2_128.npz"), allow_pickle=False)
    x = env["synth"].make_crops(3, 1, 96, 80, seed=9)
    outs = []
    for unfused in (False, True):
        if unfused:
            monkeypatch.setenv("ESAHRNET_X6_UNFUSED_STEM", "1")
        net, sd = _build(env, "seg_hrnet2", (32, 64, 128, 256), 9)
        with torch.no_grad():
            y, ops = net.forward_timed(x.cuda())
            taps = net.taps(x.cuda())
        kernels = [o["kernel"] for o in ops]
        assert ("stem_x6_kernel" in kernels) == (not unfused) and ("stem_kernel" in kernels) == unfused, kernels[:3]
        assert ("stem1" in taps) == unfused
        outs.append((y.cpu(), taps["stem2"].cpu()))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0])
    with torch.no_grad():
        ref = env["hrnet_ref"].forward(sd, env["hrnet_ref"].default_cfg(1, 11), x)
    assert (outs[0][0] - ref).abs().max().item() <= 2e-5
    monkeypatch.delenv("ESAHRNET_X6_UNFUSED_STEM")
    net3, _ = _build(env, "seg_hrnet", (16, 32, 64, 128), 9)
    with torch.no_grad():
        _, ops3 = net3.forward_timed(env["synth"].make_crops(1, 3, 64, 64, seed=9).cuda())
    assert ops3[0]["kernel"] == "stem_kernel"


# ------------------------------------------------------------------------------------- seg_hrnet3 (CBAM) in the fp32-grade mode
def test_hrnet3_fp32_is_the_default(env):
    net = env["seg_hrnet3"].get_seg_model(env["config"].make_config(widths=(16, 16, 32, 64)))
    assert net._cfg_struct.precision == 2 and net._cfg_struct.variant == 1


def test_hrnet3_intermediates_match_oracle(env):
    """seg_hrnet3 (models/seg_hrnet3.py): every named intermediate incl. the pre-BN stem skip, the CBAM blocks' outputs and
    the head-by-linearity tensors vs the oracle, at fp32-grade tolerance."""
    net, sd = _build(env, "seg_hrnet3", (32, 64, 128, 256), 9)
    x = env["synth"].make_crops(2, 1, 64, 96, seed=9)
    cfg = env["hrnet_ref"].default_cfg(1, 30, variant=1)
    taps_ref = {}
    with torch.no_grad():
        out_ref = env["hrnet_ref"].forward(sd, cfg, x, taps_ref)
        taps = net.taps(x.cuda())
    assert {"stem_raw", "stem2", "layer1", "stage4.3", "head0", "head3"} <= set(taps)
    for name, ref in taps_ref.items():
        if name in taps:
            err = (taps[name].cpu() - ref).abs().max().item()
            assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (name, err)
    assert (taps["heatmaps"].cpu() - out_ref).abs().max().item() <= 2e-5


def test_hrnet3_dynamic_range_sweep(env):
    """The same bar as seg_hrnet2's sweep: HIP-vs-fp64 <= 2 x (fp32 CPU reference vs fp64) at every weight gain."""
    cfg = env["hrnet_ref"].default_cfg(1, 30, variant=1)
    x = env["synth"].make_crops(1, 1, 128, 128, seed=3)
    rows = []
    for gain in (0.5, 1.0, 2.0):
        net, sd = _build(env, "seg_hrnet3", (32, 64, 128, 256), 3, gain)
        with torch.no_grad():
            ref64 = env["hrnet_ref"].forward(sd, cfg, x.double())
            ref32 = env["hrnet_ref"].forward(sd, cfg, x)
            y = net(x.cuda()).cpu().double()
        rows.append((gain, float(ref64.abs().max()), float((y - ref64).abs().max()), float((ref32.double() - ref64).abs().max())))
    print("gain  max|out|  HIP-vs-fp64  fp32ref-vs-fp64  ratio")
    for g_, out, e, e32 in rows:
        print(f"{g_:4.1f}  {out:8.2f}  {e:11.3e}  {e32:15.3e}  {e / e32:5.2f}")
    for g_, out, e, e32 in rows:
        assert e <= 2.0 * e32, (g_, e, e32)


@pytest.mark.parametrize("hw", [(70, 50), (16, 16), (18, 18), (36, 132), (128, 128)])
def test_hrnet3_odd_shapes_and_head_forms(env, monkeypatch, hw):
    """Odd crops (partial tiles, ragged interpolation windows); last_layer[0] by linearity (head_gather.hip) against the
    direct 3x3 over the materialised concat (ESAHRNET_HEAD3_DIRECT=1): both within fp32-grade distance of the oracle."""
    widths = (16, 32, 64, 128)
    monkeypatch.delenv("ESAHRNET_HEAD3_DIRECT", raising=False)
    net, sd = _build(env, "seg_hrnet3", widths, 41)
    x = env["synth"].make_crops(2, 1, hw[0], hw[1], seed=41)
    cfg = env["hrnet_ref"].default_cfg(1, 30, widths=widths, variant=1)
    with torch.no_grad():
        ref = env["hrnet_ref"].forward(sd, cfg, x)
        y, ops = net.forward_timed(x.cuda())
        y = y.cpu()
    assert "head_gather" in {o["kernel"] for o in ops}
    monkeypatch.setenv("ESAHRNET_HEAD3_DIRECT", "1")
    net_d, _ = _build(env, "seg_hrnet3", widths, 41)
    with torch.no_grad():
        yd, ops_d = net_d.forward_timed(x.cuda())
        yd = yd.cpu()
    assert "head_gather" not in {o["kernel"] for o in ops_d}
    assert torch.isfinite(y).all()
    scale = max(1.0, ref.abs().max().item())
    assert (y - ref).abs().max().item() <= 2e-5 * scale
    assert (yd - ref).abs().max().item() <= 2e-5 * scale


@pytest.mark.parametrize("stem_width, cin, unfused", [(32, 1, False), (64, 3, False), (64, 1, True)])
def test_hrnet3_stem_where_stem_x6_does_not_serve(env, monkeypatch, stem_width, cin, unfused):
    """stem_x6_kernel serves cin 1 and stem width 64 only: another stem width, another cin and ESAHRNET_X6_UNFUSED_STEM=1 take
    stem_kernel + the stride-2 convolution, within fp32-grade distance of the oracle.  At (64, 1) the unfused stem is bit-identical
    to stem_x6_kernel.  (The Python module fixes a stem width of 64: the test hands the library a configuration with another
    width, and the module takes its convolutions from the library.)"""
    from esa_pose_estimation_amd import hrnet
    make = hrnet._cfg_struct

    def cfg_struct(*a, **k):
        s = make(*a, **k)
        s.stem_width = stem_width
        return s
    monkeypatch.setattr(hrnet, "_cfg_struct", cfg_struct)
    monkeypatch.delenv("ESAHRNET_X6_UNFUSED_STEM", raising=False)
    if unfused:
        monkeypatch.setenv("ESAHRNET_X6_UNFUSED_STEM", "1")
    net, sd = _build(env, "seg_hrnet3", (32, 64, 128, 256), 19, cin=cin)
    assert sd["conv1.weight"].shape == (stem_width, cin, 3, 3)
    x = env["synth"].make_crops(2, cin, 64, 96, seed=19)
    cfg = env["hrnet_ref"].default_cfg(cin, 30, variant=1, stem_width=stem_width)
    with torch.no_grad():
        ref = env["hrnet_ref"].forward(sd, cfg, x)
        y, ops = net.forward_timed(x.cuda())
        y = y.cpu()
    kernels = [o["kernel"] for o in ops]
    assert "stem_x6_kernel" not in kernels and "stem_kernel" in kernels, kernels[:3]
    assert (y - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    if unfused:
        monkeypatch.delenv("ESAHRNET_X6_UNFUSED_STEM")
        net_f, _ = _build(env, "seg_hrnet3", (32, 64, 128, 256), 19, cin=cin)
        with torch.no_grad():
            y_f, ops_f = net_f.forward_timed(x.cuda())
        assert "stem_x6_kernel" in {o["kernel"] for o in ops_f}
        assert torch.equal(y_f.cpu(), y)


def test_hrnet3_cbam_forms_agree(env, monkeypatch):
    """Merged CBAM launches (cbam_jobs_kernel) / fused cbam_spatial against their single-tensor, unfused forms."""
    monkeypatch.delenv("ESAHRNET_NO_JOBS", raising=False)
    monkeypatch.delenv("ESAHRNET_CBAM_UNFUSED", raising=False)
    net, sd = _build(env, "seg_hrnet3", (32, 64, 128, 256), 13)
    x = env["synth"].make_crops(2, 1, 128, 128, seed=13).cuda()
    with torch.no_grad():
        y = net(x).clone()
    monkeypatch.setenv("ESAHRNET_NO_JOBS", "1")
    net1, _ = _build(env, "seg_hrnet3", (32, 64, 128, 256), 13)
    with torch.no_grad():
        y1 = net1(x).clone()
    monkeypatch.setenv("ESAHRNET_CBAM_UNFUSED", "1")
    net2, _ = _build(env, "seg_hrnet3", (32, 64, 128, 256), 13)
    with torch.no_grad():
        y2 = net2(x).clone()
    assert torch.equal(y, y1)
    assert (y - y2).abs().max().item() <= 2e-6 * max(1.0, y.abs().max().item())


def test_hrnet3_batch_properties_and_graph_replay(env):
    """seg_hrnet3 at the bench shape's topology (W32, 30 keypoints): every sample equals its own batch-1 forward bit for bit
    (no kernel choice depends on the batch), permutation equivariance, HIP-graph replay identical to the eager forward."""
    net, sd = _build(env, "seg_hrnet3", (32, 64, 128, 256), 17)
    x = env["synth"].make_crops(6, 1, 128, 128, seed=17).cuda()
    xc = x.clone()
    with torch.no_grad():
        y = net(x).clone()
        ys = [net(x[i:i + 1]).clone() for i in (0, 5)]
        perm = torch.tensor([3, 0, 5, 1, 4, 2], device="cuda")
        yp = net(x[perm]).clone()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            yg = net(x)
        gph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, xc) and torch.isfinite(y).all()
    for i, y1 in zip((0, 5), ys):
        assert torch.equal(y[i:i + 1], y1), i
    assert torch.equal(yp, y[perm])
    assert torch.equal(yg, y)
    kp = env["inference"].heatmaps_to_keypoints(y)
    assert kp.shape == (6, 30, 3) and bool(torch.isfinite(kp).all())
