"""fp16 scale exponents on the GPU: per-tensor power-of-two scales that bring a checkpoint into fp16's range,
chosen by net.calibrate_fp16 from one range-scanning forward of a bf16 twin.

The checkpoints are the golden fixtures' (tiny_hrnet2_64, w32_hrnet2_128, n = 2) moved out of fp16's range by powers of two
(tests/fp16_scale_ref.py: hot x 2^16, cold x 2^-16, mixed: three blocks' conv1 outputs x 2^16 / 2^-18 inside an unchanged
function), so the reference of each is the committed golden x s exactly.  Bounds, stated up front:
  * exactness: a hot (cold) net with every exponent at 16 (-16) stores the bits the plain net stores on the plain fixture, so
    its heat-maps and its true-scale taps are the plain net's x 2^+-16 BIT FOR BIT (torch.equal);
  * the plain fp16 net on hot, cold and mixed misses BOUND_FACTOR x EMU_LINF x s: the inputs bite (or, mixed on the narrow
    tiny net, esahrnet_commit refuses the checkpoint outright: a conv2 weight x 2^18 is not finite in fp16);
  * after calibrate_fp16: L_inf and mean-abs within BOUND_FACTOR x EMU_LINF / EMU_MEAN x s of the golden x s — §3c's own margin
    (tests/fp16_emu.py), nothing new —, no arg-max moves, no stored value and no h0 reaches 65504;
  * the calibrated exponents of hot / cold / mixed minus the plain checkpoint's are exactly +16 / -16 everywhere, resp. +16, +16
    and -18 on the three blocks' conv1 groups and 0 elsewhere (every scan of the bf16 twin scales exactly);
  * the h0 record of the fused head's range form: max_abs against head_ref.head_section's float64 head0 of the tapped stage-4
    tensors under test_gpu_head.py's rule for this kernel, |HIP - f64| <= 2 E_emu + q max|ref| (q = 2^-9 bf16, 2^-12 fp16);
    n_ge_f16max exactly, on planted last_layer.1 biases that put every h0 below 2^12 or above 2^20 (asserted on the reference).

Measured on an MI355X (27 cases in 6 s, none above 0.5 s; L_inf / mean-abs / arg-max flips in the golden's units):
  tiny_hrnet2_64   plain fp16: hot 2.08e-1 / 3.83e-2 / 4, cold 4.99e-3 / 6.55e-4 / 0, mixed refused by commit;
                   calibrated, all four checkpoints: 4.88e-4 / 6.24e-5 / 0   [bounds 1.52e-3 / 1.79e-4]
  w32_hrnet2_128   plain fp16: hot 2.90e-1 / 1.00e-1 / 3, cold 4.95e-3 / 6.48e-4 / 0, mixed refused by commit;
                   calibrated, all four checkpoints: 5.15e-4 / 8.85e-5 / 0   [bounds 1.49e-3 / 2.72e-4]
  h0 max_abs: error / bound at most 0.11 (fp16, 64 x 64), counts exact.  DESIGN.md §3e has the table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_emu  # noqa: E402
import fp16_scale_ref as R  # noqa: E402
import head_ref as HR  # noqa: E402

pytestmark = pytest.mark.gpu

TAGS = ("tiny_hrnet2_64", "w32_hrnet2_128")
CASES = ("hot", "cold", "mixed")


@pytest.fixture(scope="module")
def env(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from esa_pose_estimation_amd import _lib, config, inference, seg_hrnet2, synth
    from oracle import hrnet_ref
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    e = dict(lib=_lib.lib(), L=_lib, config=config, inference=inference, seg_hrnet2=seg_hrnet2, fixtures={}, nets={}, plain_out={})
    for tag in TAGS:
        g = np.load(os.path.join(golden_dir, tag + ".npz"), allow_pickle=False)
        _, cin, K, widths, sd, x, cfg = fp16_emu.golden_case(g, synth, hrnet_ref)
        e["fixtures"][tag] = dict(g=g, widths=widths, cases=R.checkpoints(sd, x))
    return e


def _net(env, tag, case, precision="fp16"):
    """A fresh net of the fixture's stage table with the case's checkpoint, on the device."""
    f = env["fixtures"][tag]
    net = env["seg_hrnet2"].get_seg_model(env["config"].make_config(widths=f["widths"]), precision=precision)
    net.load_state_dict(f["cases"][case][0], strict=True)
    return net.cuda().eval()


def _x(env, tag, case):
    return env["fixtures"][tag]["cases"][case][1].cuda()


def _calibrated(env, tag, case):
    """The case's net after calibrate_fp16 on its crops, once per module: (net, calibration, heat-maps on the host)."""
    key = (tag, case)
    if key not in env["nets"]:
        net = _net(env, tag, case)
        with torch.no_grad():
            cal = net.calibrate_fp16(_x(env, tag, case))
            y = net(_x(env, tag, case)).cpu()
        env["nets"][key] = (net, cal, y)
    return env["nets"][key]


def _plain_out(env, tag):
    if tag not in env["plain_out"]:
        net = _net(env, tag, "plain")
        with torch.no_grad():
            env["plain_out"][tag] = (net(_x(env, tag, "plain")).cpu(), {k: t.cpu() for k, t in net.taps(_x(env, tag, "plain")).items()})
    return env["plain_out"][tag]


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hot", "cold"])
@pytest.mark.parametrize("tag", TAGS)
def test_ideal_exponents_reproduce_the_plain_net_bit_for_bit(env, tag, case):
    y_base, taps_base = _plain_out(env, tag)
    s = R.SCALE[case]
    net = _net(env, tag, case)
    net.fp16_exponents = [16 if case == "hot" else -16] * len(net.fp16_scale_groups)
    with torch.no_grad():
        y = net(_x(env, tag, case)).cpu()
        taps = {k: t.cpu() for k, t in net.taps(_x(env, tag, case)).items()}
    assert torch.equal(y, y_base * s)
    assert set(taps) == set(taps_base) and len(taps) >= 8
    for name, t in taps.items():                                      # true-scale taps: the plain net's x s, bit for bit
        assert torch.equal(t, taps_base[name] * s), name
    net.fp16_exponents = [0] * len(net.fp16_scale_groups)              # and back: the plain fp16 net on a hot / cold checkpoint
    with torch.no_grad():
        y0 = net(_x(env, tag, case)).cpu()
    assert not torch.equal(y0, y)


# ---- 2. the inputs bite -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tag", TAGS)
def test_plain_fp16_misses_the_bound_on_checkpoints_outside_its_range(env, tag, case):
    f = env["fixtures"][tag]
    net = _net(env, tag, case)
    try:
        with torch.no_grad():
            y = net(_x(env, tag, case)).cpu().numpy()
    except env["L"].EsaHrnetError as e:
        # the mixed checkpoint's conv2 weights x 2^18 can leave fp16 altogether (tiny_hrnet2_64: narrow layers, large weights);
        # esahrnet_commit then refuses the network instead of saturating it — the hardest way to miss the bound
        assert case == "mixed" and "not finite in fp16" in str(e) and "stage4.0.branches.0.2.conv2" in str(e), e
        print(f"\n{tag} {case}: plain fp16 refused at commit: {e}")
        return
    linf, mean, flips = R.errors(y, f["g"], f["cases"][case][2])
    print(f"\n{tag} {case}: plain fp16 L_inf {linf:.3e} mean-abs {mean:.3e} arg-max flips {flips}")
    assert linf > fp16_emu.BOUND_FACTOR * fp16_emu.EMU_LINF[tag], linf


# ---- 3. calibrated ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("plain",) + CASES)
@pytest.mark.parametrize("tag", TAGS)
def test_calibrated_net_meets_the_fp16_bound(env, tag, case):
    f = env["fixtures"][tag]
    net, cal, y = _calibrated(env, tag, case)
    s = f["cases"][case][2]
    linf, mean, flips = R.errors(y.numpy(), f["g"], s)
    print(f"\n{tag} {case}: calibrated fp16 L_inf {linf:.3e} mean-abs {mean:.3e} arg-max flips {flips}   "
          f"[bounds {fp16_emu.BOUND_FACTOR * fp16_emu.EMU_LINF[tag]:.3e} / {fp16_emu.BOUND_FACTOR * fp16_emu.EMU_MEAN[tag]:.3e}]   "
          f"exponents {min(cal.exponents)} .. {max(cal.exponents)}")
    assert linf <= fp16_emu.BOUND_FACTOR * fp16_emu.EMU_LINF[tag], linf
    assert mean <= fp16_emu.BOUND_FACTOR * fp16_emu.EMU_MEAN[tag], mean
    assert flips == 0
    assert net.fp16_exponents == cal.exponents and cal.names == net.fp16_scale_groups
    with torch.no_grad():
        st = net._rt.forward_stats(net, _x(env, tag, case), with_h0=True)
    assert [r["name"] for r in st.saturated() if r["group"] >= 0] == []
    assert int(st.h0["n_ge_f16max"].sum()) == 0 and float(st.h0["max_abs"].max()) > 0
    assert torch.equal(st.heatmaps.cpu(), y)
    # the rows are the STORED values.  The twin put every group's maximum into (2^11, 2^12]; the fp16 net's own values differ
    # from the twin's by rounding noise, far below the factor 2 allowed here: one of the three bits of headroom at the most
    for r in st.scanned():
        if r["group"] >= 0:
            assert r["exponent"] == cal.exponents[r["group"]] and r["max_abs"] < 2.0 ** 13, r
    assert all(2.0 ** 10 < m < 2.0 ** 13 for m in cal.stored_max), cal.stored_max


# ---- 4. the exponents -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_calibrated_exponents_differ_from_the_plain_checkpoints_by_the_planted_powers(env, tag):
    base = _calibrated(env, tag, "plain")[1]
    net = _calibrated(env, tag, "plain")[0]
    lib, L = env["lib"], env["L"]
    convs = R.scale_convs(lib, L, net._rt._probe, net._descs)
    want = {"hot": [16] * len(base.names), "cold": [-16] * len(base.names), "mixed": [0] * len(base.names)}
    for block, k in R.MIXED_BLOCKS.items():
        want["mixed"][convs[block + ".conv1"][0]] = k
    assert sorted(v for v in want["mixed"] if v) == [-18, 16, 16]
    for case in CASES:
        cal = _calibrated(env, tag, case)[1]
        diff = [a - b for a, b in zip(cal.exponents, base.exponents)]
        assert diff == want[case], (case, {n: d for n, d, w in zip(cal.names, diff, want[case]) if d != w})
    print(f"\n{tag}: plain checkpoint's exponents {dict(zip(base.names, base.exponents))}")


# ---- 5. the h0 record -------------------------------------------------------------------------------------------------------
def _stats_h0_raw(env, net, x, with_h0=True):
    """esahrnet_forward_stats_h0 / esahrnet_forward_stats through the C ABI on a workspace of the test's own, then the tap
    "head3_fused" read from that workspace: -> (heat-maps, records [rows, n], h0 records [n] or None, head3 or None)."""
    lib, L = env["lib"], env["L"]
    n, _, hh, ww = x.shape
    h = net._rt._handle_for(net, x.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = C.c_size_t()
    L.check((lib.esahrnet_forward_stats_h0_workspace_bytes if with_h0 else lib.esahrnet_forward_stats_workspace_bytes)(
        h, n, hh, ww, C.byref(nbytes)))
    ws = torch.full((nbytes.value + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    rows = len(net._rt.stats_rows(h, n, hh, ww))
    heat = torch.full((n, net._k, hh, ww), float("nan"), device="cuda")
    rec = torch.full((rows + 1, n, 64), 0xFF, dtype=torch.uint8, device="cuda")
    L.check(lib.esahrnet_set_debug_keep(h, 0))
    if with_h0:
        L.check(lib.esahrnet_forward_stats_h0(h, x.data_ptr(), n, hh, ww, heat.data_ptr(), ws_ptr, nbytes.value, rec.data_ptr(),
                                              rec[rows].data_ptr(), stream))
    else:
        L.check(lib.esahrnet_forward_stats(h, x.data_ptr(), n, hh, ww, heat.data_ptr(), ws_ptr, nbytes.value, rec.data_ptr(), stream))
    head3 = None
    c, th, tw = C.c_int(), C.c_int(), C.c_int()
    L.check(lib.esahrnet_tap_shape(h, b"head3_fused", hh, ww, C.byref(c), C.byref(th), C.byref(tw)))
    L.check(lib.esahrnet_set_debug_keep(h, 1))
    t = torch.empty((n, c.value, th.value, tw.value), device="cuda")
    if lib.esahrnet_tap_read(h, b"head3_fused", n, hh, ww, ws_ptr, t.data_ptr(), stream) == 0:
        head3 = t.cpu()
    L.check(lib.esahrnet_set_debug_keep(h, 0))
    torch.cuda.synchronize()
    out = rec.cpu().numpy().reshape(-1).view(L.stats_dtype()).reshape(rows + 1, n)
    return heat.cpu(), out[:rows], out[rows] if with_h0 else None, head3


def _raw64(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(*a.shape, 64)


@pytest.mark.parametrize("shape", [(2, 64, 64), (2, 70, 50)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_h0_record_of_the_range_form(env, precision, shape):
    """tiny_hrnet2_64's weights at 64 x 64 (whole tiles) and 70 x 50 (odd level sizes 35 x 25: partial tiles both ways, the
    lanes outside the image must not count), both element types; then the planted biases."""
    from esa_pose_estimation_amd import synth
    tag = "tiny_hrnet2_64"
    p = 1 if precision == "bf16" else 3
    sd = env["fixtures"][tag]["cases"]["plain"][0]
    net = _net(env, tag, "plain", precision)
    n, hh, ww = shape
    x = synth.make_crops(n, 1, hh, ww, seed=5).cuda()
    with torch.no_grad():
        y = net(x).cpu()
        taps = {k: t.cpu() for k, t in net.taps(x).items()}
        heat, rec, h0, head3 = _stats_h0_raw(env, net, x)
        heat_p, rec_p, _, head3_p = _stats_h0_raw(env, net, x, with_h0=False)
    assert "head3_fused" in taps and "head0" not in taps               # the fused head ran: h0 exists in registers only
    # the range form computes what the product form computes, bit for bit, and the rows do not change
    assert torch.equal(heat, y) and torch.equal(heat_p, y)
    assert torch.equal(head3, taps["head3_fused"]) and torch.equal(head3_p, taps["head3_fused"])
    assert np.array_equal(_raw64(rec), _raw64(rec_p))
    # max_abs against the float64 head0 of the tapped stage-4 tensors
    ys = [taps[f"stage4.{b}"] for b in range(4)]
    with torch.no_grad():
        ref = HR.head_section(sd, ys)["head0"]
        emu = HR.head_emulation(sd, ys, 0, p)["head0"]
    for i in range(n):
        want = ref[i].abs().max().item()
        e_emu = (emu[i].double() - ref[i]).abs().max().item()
        bound = 2.0 * e_emu + HR.QUANTUM[p] * want
        print(f"\n{precision} {shape} crop {i}: h0 max_abs {h0['max_abs'][i]:.6g}  f64 {want:.6g}  error / bound "
              f"{abs(h0['max_abs'][i] - want) / bound:.3f}")
        assert abs(float(h0["max_abs"][i]) - want) <= bound
        assert h0["max"][i] == h0["max_abs"][i] and h0["n_ge_f16max"][i] == 0
    # a crop's record is the same alone and in a batch
    for i in range(n):
        with torch.no_grad():
            _, _, alone, _ = _stats_h0_raw(env, net, x[i:i + 1].contiguous())
        assert np.array_equal(_raw64(alone), _raw64(h0[i:i + 1])), i
    # planted: last_layer.1's bias +2^22 on some channels (h0 ~ 2^22, counted), -2^22 on others (ReLU: 0); the rest O(1)
    planted = {k: v.clone() for k, v in sd.items()}
    ct = planted["last_layer.1.bias"].numel()
    up, down = [0, 5, 17, ct // 2, ct - 1], [1, 18, ct - 2]
    planted["last_layer.1.bias"][up] += 2.0 ** 22
    planted["last_layer.1.bias"][down] -= 2.0 ** 22
    net.load_state_dict(planted, strict=True)
    with torch.no_grad():
        taps = {k: t.cpu() for k, t in net.taps(x).items()}
        _, _, h0, _ = _stats_h0_raw(env, net, x)
        ys = [taps[f"stage4.{b}"] for b in range(4)]
        ref = HR.head_section(planted, ys)["head0"]
        emu = HR.head_emulation(planted, ys, 0, p)["head0"]
    assert not bool(((ref >= 2.0 ** 12) & (ref <= 2.0 ** 20)).any())    # a condition on the inputs: nothing near the threshold
    want = (ref >= 65504.0).sum((1, 2, 3))
    assert want.tolist() == [len(up) * ref.shape[2] * ref.shape[3]] * n
    assert h0["n_ge_f16max"].tolist() == want.tolist()
    for i in range(n):              # (the emulation saturates its fp16 h0 at 65504: the planted channels are held by the count)
        low = ref[i] < 2.0 ** 12
        e_emu = ((emu[i].double() - ref[i]).abs() * low).max().item()
        assert abs(float(h0["max_abs"][i]) - ref[i].max().item()) <= 2.0 * e_emu + HR.QUANTUM[p] * ref[i].max().item()


def test_h0_record_is_the_stored_row_where_the_materialised_head_runs(env, monkeypatch):
    """ESAHRNET_BF_UNFUSED_HEAD=1: slice 0 + fuse + 1x1; h0 is the tensor "head0" and its record the row's, byte for byte."""
    monkeypatch.setenv("ESAHRNET_BF_UNFUSED_HEAD", "1")             # (read when the device's handle is created: at the forward)
    net = _net(env, "tiny_hrnet2_64", "plain")
    x = _x(env, "tiny_hrnet2_64", "plain")
    with torch.no_grad():
        st = net._rt.forward_stats(net, x, with_h0=True)
    (row,) = [i for i, r in enumerate(st.rows) if r["name"] == "head0"]
    assert st.rows[row]["scanned"] and st.rows[row]["n_finite"] > 0
    assert np.array_equal(_raw64(st.h0), _raw64(st.per_image[row]))


# ---- 6. a calibrated net is a net ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_calibrated_net_decodes_and_does_not_depend_on_the_batch(env, tag):
    inference = env["inference"]
    net, _, y = _calibrated(env, tag, "mixed")
    x = _x(env, tag, "mixed")
    with torch.no_grad():
        heat = net(x)
        assert torch.equal(heat.cpu(), y)
        assert torch.equal(net(x, output="keypoints"), inference.heatmaps_to_keypoints(heat))
        assert torch.equal(net(x, output="keypoints", refine="get_final2"), inference.heatmaps_to_keypoints(heat, refine="get_final2"))
        for i in range(x.shape[0]):
            assert torch.equal(net(x[i:i + 1].contiguous()).cpu(), y[i:i + 1]), i
        perm = torch.arange(x.shape[0] - 1, -1, -1)
        assert torch.equal(net(x[perm.cuda()].contiguous()).cpu(), y[perm])
