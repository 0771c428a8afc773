"""The activation range report on the GPU (include/esahrnet.h: esahrnet_tensor_stats, esahrnet_forward_stats;
net.activation_stats): the scan of one raw tensor against the numpy reference of tests/stats_ref.py in all five forms, the
report of a forward against net.taps, and what the report is for: a saturating fp16 forward and a non-finite input are
visible in it, row by row."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stats_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CHANNELS = (1, 11, 18, 30, 64, 94)          # partial chunks, a single chunk, C = Cp (64 in every format), two pixel strides
EXTENTS = ((1, 1), (5, 7), (16, 16), (33, 65))      # fewer pixels than a workgroup has lanes; ranges that do not divide
TINY_MAX, TINY_MIN = 2.0 ** -14 - 2.0 ** -24, 2.0 ** -24       # fp16's largest and smallest subnormal
PLANTS = (np.nan, np.inf, -np.inf, 65504.0, -65504.0, 65520.0, TINY_MAX, TINY_MIN, -0.0, 2.0 ** -14, -TINY_MIN, 0.0)
# the networks: (module, cin, K, variant, widths).  seg_hrnet3 refuses a branch narrower than 16 channels at create, so it
# takes the narrowest widths it accepts
NETS = {"hrnet2": ("seg_hrnet2", 1, 11, 0, (8, 16, 32, 64)), "hrnet3": ("seg_hrnet3", 1, 30, 1, (16, 16, 32, 64))}
NET_CASES = [("hrnet2", p) for p in ("fp32", "bf16x3", "bf16", "fp16")] + [("hrnet3", p) for p in ("fp32", "bf16x3", "bf16")]
SHAPES = ((3, 64, 64), (3, 18, 34))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, seg_hrnet2, seg_hrnet3, synth
    from oracle import hrnet_ref
    return dict(lib=_lib.lib(), L=_lib, config=config, synth=synth, seg_hrnet2=seg_hrnet2, seg_hrnet3=seg_hrnet3,
                hrnet_ref=hrnet_ref)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the operator ------------------------------------------------------------------------------------------------------------
def scan(env, form, raw, n, c, cp, h, w):
    """esahrnet_tensor_stats of a raw tensor (numpy uint8) -> records [n]; workspace and records pre-filled with 0xFF."""
    lib, L = env["lib"], env["L"]
    fmt = R.FORMS[form]
    t = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
    need = C.c_size_t()
    L.check(lib.esahrnet_tensor_stats_workspace_bytes(fmt, n, c, cp, h, w, C.byref(need)))
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((n * L.STATS_RECORD_BYTES,), 0xFF, dtype=torch.uint8, device="cuda")
    L.check(lib.esahrnet_tensor_stats(t.data_ptr(), fmt, n, c, cp, h, w, ws.data_ptr(), need.value, out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    b = out.cpu().numpy()
    assert not b.reshape(n, 64)[:, 44:].any(), "the reserved bytes of a record are zero"
    return b.view(L.stats_dtype())


def raw64(rec):
    """The records' bytes [..., 64], padding included (indexing a structured array copies its named fields only)."""
    return rec.view(np.uint8).reshape(*rec.shape, 64)


def values(seed, n, c, h, w, scale=3.0, plants=PLANTS):
    """f32 [n, c, h, w] ~ N(0, scale) with the plants spread over the images (as many as there are elements for)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, c, h, w)) * scale).astype(np.float32)
    per = c * h * w
    flat = x.reshape(n, per)
    for k, p in enumerate(plants):
        flat[(k + seed) % n, (k * 7919 + 3 + seed) % per] = p
    return x


def with_padding(form, x, fill):
    """x [n, c, h, w] -> [n, Cp, h, w]; the padding channels hold `fill` (a sequence, cycled over them)."""
    n, c, h, w = x.shape
    cp = R.padded(form, c)
    full = np.zeros((n, cp, h, w), dtype=np.float32)
    full[:, :c] = x
    for j in range(c, cp):
        full[:, j] = fill[(j - c) % len(fill)]
    return full


def check_tensor(env, form, x, what):
    """Every property of the operator on one tensor of real values x [n, c, h, w]."""
    n, c, h, w = x.shape
    cp = R.padded(form, c)
    raw, held = R.pack(form, with_padding(form, x, (0.0,)))
    got = scan(env, form, raw, n, c, cp, h, w)
    R.assert_records(got, R.records(held[:, :c]), what)
    if cp > c:          # poisoned padding changes no bit of any record
        raw_p, _ = R.pack(form, with_padding(form, x, (np.nan, 1e30, -np.inf, -1e30)))
        assert np.array_equal(raw64(scan(env, form, raw_p, n, c, cp, h, w)), raw64(got)), what
    if n > 1:           # an image's record alone and in a permuted batch: the same bits
        per = raw.size // n
        for i in range(n):
            alone = scan(env, form, raw[i * per:(i + 1) * per], 1, c, cp, h, w)
            assert np.array_equal(raw64(alone), raw64(got)[i:i + 1]), (what, i)
        perm = [(i + 1) % n for i in range(n)]
        raw_q = np.concatenate([raw[i * per:(i + 1) * per] for i in perm])
        assert np.array_equal(raw64(scan(env, form, raw_q, n, c, cp, h, w)), raw64(got)[perm]), what


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("form", list(R.FORMS))
def test_operator_against_reference(env, form, c):
    for hi, (h, w) in enumerate(EXTENTS):
        for n in (1, 3):
            check_tensor(env, form, values(100 * c + 10 * hi + n, n, c, h, w), (form, c, h, w, n))


@pytest.mark.parametrize("form", list(R.FORMS))
def test_operator_several_partials_per_image(env, form):
    n, c, h, w = 3, 32, 64, 96
    need = C.c_size_t()
    env["L"].check(env["lib"].esahrnet_tensor_stats_workspace_bytes(R.FORMS[form], n, c, R.padded(form, c), h, w, C.byref(need)))
    assert need.value >= n * 6 * 64
    check_tensor(env, form, values(7, n, c, h, w, scale=100.0), (form, "64x96x32"))


@pytest.mark.parametrize("form", list(R.FORMS))
def test_operator_zero_image_and_image_without_a_finite_value(env, form):
    n, c, h, w = 3, 11, 16, 16
    x = values(11, n, c, h, w)
    x[1] = 0.0
    x[1, 3] = -0.0
    x[2] = np.nan
    x[2, ::2] = np.inf
    x[2, 1, ::2] = -np.inf
    cp = R.padded(form, c)
    raw, held = R.pack(form, with_padding(form, x, (0.0,)))
    got = scan(env, form, raw, n, c, cp, h, w)
    R.assert_records(got, R.records(held[:, :c]), form)
    per = c * h * w
    assert got["n_zero"][1] == per and got["n_finite"][1] == per and got["max_abs"][1] == 0 and got["sum_abs"][1] == 0
    assert got["min"][1] == 0 and got["max"][1] == 0
    assert got["n_finite"][2] == 0 and got["n_nan"][2] + got["n_inf"][2] == per and got["n_zero"][2] == 0
    assert got["max_abs"][2] == 0 and got["min"][2] == np.inf and got["max"][2] == -np.inf and got["sum_abs"][2] == 0
    assert got["n_ge_f16max"][2] == 0 and got["n_f16_tiny"][2] == 0


# ---- the network -------------------------------------------------------------------------------------------------------------
def _build(env, key, precision):
    module, cin, k, variant, widths = NETS[key]
    net = env[module].get_seg_model(env["config"].make_config(widths=widths), precision=precision)
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=53, gain=0.5)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval(), sd


@pytest.fixture(scope="module", params=NET_CASES, ids=lambda c: "-".join(c))
def case(request, env):
    saved = {k: os.environ.pop(k) for k in [k for k in os.environ if k.startswith("ESAHRNET_")]}
    try:
        key, precision = request.param
        net, sd = _build(env, key, precision)
    finally:
        os.environ.update(saved)
    yield dict(key=key, precision=precision, net=net, sd=sd)
    del net
    torch.cuda.empty_cache()


def _crops(env, key, shape, seed=5):
    n, h, w = shape
    return env["synth"].make_crops(n, NETS[key][1], h, w, seed=seed).cuda()


def _raw_forward_stats(env, net, x, ws_fill, short=0, ws_shift=0, stats_shift=0):
    """esahrnet_forward_stats at the ctypes level inside buffers this test owns -> (rc, heat, stats bytes [rows, n, 64])."""
    lib, L = env["lib"], env["L"]
    n, _, hh, ww = x.shape
    h = net._rt._handle_for(net, x.device)
    L.check(lib.esahrnet_set_debug_keep(h, 0))
    rows, need = C.c_int(), C.c_size_t()
    L.check(lib.esahrnet_stats_rows(h, C.byref(rows)))
    L.check(lib.esahrnet_forward_stats_workspace_bytes(h, n, hh, ww, C.byref(need)))
    ws = torch.empty(need.value + 512, dtype=torch.uint8, device="cuda")
    ws.view(torch.int32).fill_(ws_fill)
    ptr = ws.data_ptr() + (-ws.data_ptr()) % 256 + ws_shift
    heat = torch.full((n, net._k, hh, ww), float("nan"), dtype=torch.float32, device="cuda")
    stats = torch.full((rows.value * n * 64 + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.esahrnet_forward_stats(h, x.data_ptr(), n, hh, ww, heat.data_ptr(), ptr, need.value - short,
                                    stats.data_ptr() + stats_shift, _stream())
    torch.cuda.synchronize()
    return rc, heat, stats[:rows.value * n * 64].cpu().numpy().reshape(rows.value, n, 64), need.value


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_report_of_a_forward(env, case, shape):
    net, key, L = case["net"], case["key"], env["L"]
    x = _crops(env, key, shape)
    n = shape[0]
    with torch.no_grad():
        heat = net(x)
        st = net.activation_stats(x)
        taps = net.taps(x)
    assert torch.equal(st.heatmaps, heat), "the heat-maps of esahrnet_forward_stats are the bits of net(x)"
    names = [r["name"] for r in st.rows]
    assert names[-1] == "heatmaps" and st.per_image.shape == (len(names), n)
    assert len(taps) > 5
    for name, t in taps.items():        # every named tap and the heat-maps
        assert names.count(name) == 1, name
        i = names.index(name)
        assert st.rows[i]["scanned"] and st.rows[i]["shape"] == tuple(t.shape[1:]), name
        want = R.records(t.cpu().numpy())
        R.assert_records(st.per_image[i], want, (name, case["precision"]))
        assert st.rows[i]["max_abs"] == want["max_abs"].max() and st.rows[i]["n_finite"] == int(want["n_finite"].sum())
    raw = raw64(st.per_image)
    for i, r in enumerate(st.rows):
        if not r["scanned"]:
            assert not raw[i].any(), r["name"]
        else:
            c, h, w = r["shape"]
            assert np.all(st.per_image[i]["n_finite"].astype(np.int64) + st.per_image[i]["n_nan"] + st.per_image[i]["n_inf"] == c * h * w)
    assert st.first_nonfinite() is None and st.saturated() == [] and st.headroom_fp16() > 1.0
    assert len(st.table().splitlines()) == len(names) + 1
    # the workspace's prior contents do not matter: zeros, NaN (f32, bf16 and fp16 alike), 0xFF in every byte
    runs = [_raw_forward_stats(env, net, x, fill) for fill in (0, 0x7FC07FC0, -1)]
    for rc, heat_i, stats_i, _ in runs:
        assert rc == 0, env["lib"].esahrnet_last_error().decode()
        assert torch.equal(heat_i, heat)
        assert np.array_equal(stats_i, raw)
    # an image's records alone and in a permuted batch: the same bits
    with torch.no_grad():
        for i in range(n):
            alone = net.activation_stats(x[i:i + 1].contiguous())
            assert np.array_equal(raw64(alone.per_image), raw[:, i:i + 1]), i
        perm = [(i + 1) % n for i in range(n)]
        moved = net.activation_stats(x[perm].contiguous())
        assert np.array_equal(raw64(moved.per_image), raw[:, perm])


def test_a_nonfinite_input_is_located(env, case):
    """One +inf pixel in one crop.  Where the plan's first stored tensor is conv1's own output in a format that holds an
    infinity (seg_hrnet3's stem_raw in every precision, stem1 in bf16), first_nonfinite() names it.  The other plans store
    nothing before conv2's ReLU (the fused stems of fp32 and bf16x3) or saturate on the store (fp16), and the forward itself
    loses the value there: conv2 sums +inf and -inf terms, and the integer-maximum ReLU (csrc/sb.h relu1 / relu_opt) turns the
    sign-set NaN of that sum into 0.  net.taps(x) shows the same (measured on an MI355X: stem1 299 infinities in bf16, stem2 0
    non-finite values in all four precisions), so there the report names the first tensor that does hold one, which is the
    heat-maps: the output layer reads the crop itself.  In every case the report agrees with the taps count for count, and
    only the records of the crop with the infinity carry non-finite counts."""
    net, n, who = case["net"], 3, 2
    x = _crops(env, case["key"], (n, 64, 64), seed=3)
    x[who, 0, 40, 11] = float("inf")
    with torch.no_grad():
        st = net.activation_stats(x)
        taps = net.taps(x)
    names = [r["name"] for r in st.rows]
    bad = st.per_image["n_nan"].astype(np.int64) + st.per_image["n_inf"]
    for name, t in taps.items():
        want = (~torch.isfinite(t)).reshape(n, -1).sum(1).cpu().numpy()
        assert np.array_equal(bad[names.index(name)], want), name
    assert bad[:, who].any() and not bad[:, [i for i in range(n) if i != who]].any()
    first = next(r for r in st.rows if r["scanned"])
    assert first["def_op"] == 0
    if first["name"] in ("stem_raw", "stem1") and case["precision"] != "fp16":
        assert st.first_nonfinite() == first["name"]
    else:
        assert first["name"] == ("stem1" if case["precision"] == "fp16" else "stem2")
        assert st.first_nonfinite() == "heatmaps"
        assert not bad[:-1].any()


def test_refusals_of_a_committed_handle(env, case):
    net, key, lib = case["net"], case["key"], env["lib"]
    x = _crops(env, key, (2, 64, 64))

    def err():
        return lib.esahrnet_last_error().decode()
    rc, _, _, need = _raw_forward_stats(env, net, x, 0, short=1)
    assert rc == 1 and err() == f"forward_stats: workspace too small ({need - 1} < {need})"
    rc, _, _, _ = _raw_forward_stats(env, net, x, 0, ws_shift=16)
    assert rc == 1 and err() == "forward_stats: workspace must be 256-byte aligned"
    rc, _, _, _ = _raw_forward_stats(env, net, x, 0, stats_shift=4)
    assert rc == 1 and err() == "forward_stats: stats_dev must be 8-byte aligned"
    rc, _, _, _ = _raw_forward_stats(env, net, x, 0, short=1, ws_shift=16, stats_shift=4)     # the order: size, alignment, stats_dev
    assert rc == 1 and err().startswith("forward_stats: workspace too small")
    h = net._rt._handle_for(net, x.device)
    assert lib.esahrnet_forward_stats(h, x.data_ptr(), 2, 63, 64, x.data_ptr(), x.data_ptr(), 0, x.data_ptr(), None) == 1
    assert err().startswith("crop 63x64: height and width must be even")
    assert lib.esahrnet_forward_stats(h, x.data_ptr(), 0, 64, 64, x.data_ptr(), x.data_ptr(), 0, x.data_ptr(), None) == 1
    assert err() == "batch must be positive (got 0)"
    with pytest.raises(RuntimeError, match="runs only on a GPU tensor"):
        net.activation_stats(x.cpu())


# ---- what the report is for --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hot(env):
    """seg_hrnet2 in fp16 and in the fp32-grade mode with the same weights, crops times 1e6, and the CPU oracle's word that the
    stem output passes 65504 there while the fp32 heat-maps stay finite."""
    key = "hrnet2"
    f16, sd = _build(env, key, "fp16")
    f32, _ = _build(env, key, "fp32")
    x = _crops(env, key, (2, 64, 64), seed=9)
    ref_taps = {}
    with torch.no_grad():
        ref = env["hrnet_ref"].forward(sd, env["hrnet_ref"].default_cfg(1, 11, widths=NETS[key][4]), x.cpu() * 1e6, ref_taps)
    assert float(ref_taps["stem1"].max()) > 65504 and float(ref_taps["stem2"].max()) > 65504
    assert bool(torch.isfinite(ref).all())
    return dict(f16=f16, f32=f32, x=x)


def test_saturation_is_visible(env, hot):
    x = hot["x"]
    with torch.no_grad():
        cold16, cold32 = hot["f16"].activation_stats(x), hot["f32"].activation_stats(x)
        s16, s32 = hot["f16"].activation_stats(x * 1e6), hot["f32"].activation_stats(x * 1e6)
    assert cold16.saturated() == [] and cold32.saturated() == []
    assert cold16.headroom_fp16() > 1.0 and cold32.headroom_fp16() > 1.0
    rows16 = {r["name"]: r for r in s16.rows}
    rows32 = {r["name"]: r for r in s32.rows}
    for stem in ("stem1", "stem2"):         # fp16 stores conv1's output; the fp32-grade stem kernel keeps it on chip
        r = rows16[stem]
        assert r["n_ge_f16max"] > 0 and r["max_abs"] == 65504.0 and r["n_nan"] + r["n_inf"] == 0, r
    assert "stem1" not in rows32
    r = rows32["stem2"]
    assert r["max_abs"] > 65504.0 and r["n_ge_f16max"] > 0, r
    assert [r["name"] for r in s16.saturated()][:2] == ["stem1", "stem2"] and s16.headroom_fp16() == 1.0
    assert "stem2" in [r["name"] for r in s32.saturated()] and s32.headroom_fp16() < 1.0
    assert bool(torch.isfinite(s16.heatmaps).all()) and bool(torch.isfinite(s32.heatmaps).all())
