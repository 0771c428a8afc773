"""The precision report on the GPU (include/esahrnet.h: esahrnet_tensor_diff, esahrnet_forward_diff; net.precision_report):
the two-operand scan of raw tensors against the numpy restatement of tests/diff_ref.py for the five format pairs, and the
report of two forwards against net.taps of the two nets.

Bounds, stated up front: the three maxima, `at` and the four counters are exact; the three sums agree to 1e-9 relative (the
bound tests/test_gpu_stats.py holds sum_abs to: float64 rounding of at most ~1e6 additions in another order)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diff_ref as D  # noqa: E402
import fp16_scale_ref as FS  # noqa: E402
import stats_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS_A = ("SB", "BF", "F32", "HF", "NCHW")     # A's format; B is F32 (NCHW against NCHW)
# 16-bit formats pad to 64 channels: 3 -> one part-real group and seven of padding, 11 -> a real and a part-real group,
# 40 -> five real groups and three of padding; 64 at 24 x 24: 576 pixels of 8 groups, five workgroups per image
SHAPES = ((3, 5, 7), (11, 5, 7), (40, 5, 7), (64, 24, 24))
EXPONENTS = (-14, 0, 16)
TIE = 1000.0                                    # the planted largest error: b = TIE against a = 0, exact in every format
NONFINITE = ((np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, np.inf), (np.inf, -np.inf), (-np.inf, np.nan),
             (np.inf, 1.0), (1.0, -np.inf), (-np.inf, -np.inf))


@pytest.fixture(scope="module")
def env(golden_dir):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, inference, seg_hrnet2, seg_hrnet3, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, synth=synth, inference=inference, seg_hrnet2=seg_hrnet2,
                seg_hrnet3=seg_hrnet3, golden_dir=golden_dir, nets={})


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw64(rec):
    return rec.view(np.uint8).reshape(*rec.shape, 64)


# ---- the operator ------------------------------------------------------------------------------------------------------------
def _form_b(form):
    return "NCHW" if form == "NCHW" else "F32"


class Pair:
    """Two raw tensors on the device and the buffers of one esahrnet_tensor_diff call (pre-filled with 0xFF)."""

    def __init__(self, env, form, raw_a, raw_b, n, c, h, w, e):
        self.lib, self.L = env["lib"], env["L"]
        self.a = torch.from_numpy(np.ascontiguousarray(raw_a)).cuda()
        self.b = torch.from_numpy(np.ascontiguousarray(raw_b)).cuda()
        fb = _form_b(form)
        self.args = (R.FORMS[form], R.padded(form, c), R.FORMS[fb], R.padded(fb, c))
        self.n, self.c, self.h, self.w, self.e = n, c, h, w, e
        need = C.c_size_t()
        self.L.check(self.lib.esahrnet_tensor_diff_workspace_bytes(*self.args, n, c, h, w, C.byref(need)))
        self.need = need.value
        self.ws = torch.full((self.need,), 0xFF, dtype=torch.uint8, device="cuda")
        self.out = torch.full((n * 64,), 0xFF, dtype=torch.uint8, device="cuda")

    def launch(self):
        fa, cpa, fb, cpb = self.args
        self.L.check(self.lib.esahrnet_tensor_diff(self.a.data_ptr(), fa, cpa, self.b.data_ptr(), fb, cpb, self.e, self.n, self.c,
                                                   self.h, self.w, self.ws.data_ptr(), self.need, self.out.data_ptr(), _stream()))

    def records(self):
        torch.cuda.synchronize()
        b = self.out.cpu().numpy()
        assert not b.reshape(self.n, 64)[:, 56:].any(), "the reserved bytes of a record are zero"
        return b.view(self.L.diff_dtype())


def scan(env, form, raw_a, raw_b, n, c, h, w, e):
    p = Pair(env, form, raw_a, raw_b, n, c, h, w, e)
    p.launch()
    return p.records()


def with_padding(form, x, fill):
    n, c, h, w = x.shape
    full = np.full((n, R.padded(form, c), h, w), fill, dtype=np.float32)
    full[:, :c] = x
    return full


def operands(seed, form, n, c, h, w, e):
    """(a, b) f32 [n, c, h, w]: b ~ N(0, 3), a = the value that ENTERS (b + noise), with the plants.  Image 0: three ties of the
    largest error, the first of them not first in NCHW order; image 1: two ties in the last pixel and the one before it; the
    last image: none.  Non-finite pairs are spread over all images."""
    rng = np.random.default_rng(seed)
    b = (rng.standard_normal((n, c, h, w)) * 3).astype(np.float32)
    a = (b + rng.standard_normal((n, c, h, w)).astype(np.float32) * 0.01).astype(np.float32)

    def plant(i, ch, y, x, va, vb):
        a[i, ch, y, x], b[i, ch, y, x] = va, vb
    for ch, y, x in ((c - 1, 1, 2), (0, 1, 3), (c // 2, h - 1, 0)):      # NHWC order: (1,2) first; NCHW order: channel 0 first
        plant(0, ch, y, x, 0.0, TIE)
    if n > 1:
        plant(1, c - 1, h - 1, w - 1, 0.0, -TIE)
        plant(1, 0, h - 1, w - 2, 0.0, TIE)
    assert n == 3 and h >= 5 and w >= 7
    for k, (va, vb) in enumerate(NONFINITE):        # image k % 3, in a row of its own clear of the ties, three distinct columns
        plant(k % 3, (k * 5 + 1) % c, (0, 2, 3)[k % 3], (k // 3 * 2 + seed) % w, va, vb)
    return a, b


def pack_pair(form, a, b, e, pad_fill=np.nan):
    """-> (raw A, raw B, held A [n, c, h, w] as STORED, held B): A is stored as a * 2^-e in its format."""
    c = a.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        stored = np.ldexp(a, np.int32(-e)).astype(np.float32)
    raw_a, held_a = R.pack(form, with_padding(form, stored, pad_fill))
    fb = _form_b(form)
    raw_b, held_b = R.pack(fb, with_padding(fb, b, pad_fill))
    return raw_a, raw_b, held_a[:, :c], held_b[:, :c]


def reference(form, held_a, held_b, e):
    return (D.records_nchw if form == "NCHW" else D.records_nhwc)(held_a, held_b, e)


@pytest.mark.parametrize("e", EXPONENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", FORMS_A)
def test_operator_against_reference(env, form, shape, e):
    c, h, w = shape
    n = 3
    a, b = operands(100 * c + e, form, n, c, h, w, e)
    raw_a, raw_b, held_a, held_b = pack_pair(form, a, b, e)
    got = scan(env, form, raw_a, raw_b, n, c, h, w, e)
    want = reference(form, held_a, held_b, e)
    D.assert_records(got, want, (form, shape, e))
    # the plants did what they are there for
    assert got["max_abs_err"][0] == TIE and got["max_abs_err"][1] == TIE and got["max_abs_err"][2] < TIE
    first = (0 * h * w + 1 * w + 3) if form == "NCHW" else (1 * w + 2) * c + c - 1
    assert got["at"][0] == first
    assert got["at"][1] == ((h * w - 2) if form == "NCHW" else (h * w - 2) * c)
    assert got["n_class_differs"].sum() == 6 and got["n_nonfinite_test"].sum() == 7 and got["n_nonfinite_ref"].sum() == 7
    assert got["n_compared"].sum() == n * c * h * w - 9
    if form != "NCHW":      # what the padding channels hold changes no bit of any record
        for fill in (0.0, 1e30, -np.inf):
            raw_p, raw_q, _, _ = pack_pair(form, a, b, e, pad_fill=fill)
            assert np.array_equal(raw64(scan(env, form, raw_p, raw_q, n, c, h, w, e)), raw64(got)), fill
    # an image's record alone and in a permuted batch: the same bits
    pa, pb = raw_a.size // n, raw_b.size // n
    for i in range(n):
        alone = scan(env, form, raw_a[i * pa:(i + 1) * pa], raw_b[i * pb:(i + 1) * pb], 1, c, h, w, e)
        assert np.array_equal(raw64(alone), raw64(got)[i:i + 1]), i
    perm = [(i + 1) % n for i in range(n)]
    raw_ap = np.concatenate([raw_a[i * pa:(i + 1) * pa] for i in perm])
    raw_bp = np.concatenate([raw_b[i * pb:(i + 1) * pb] for i in perm])
    assert np.array_equal(raw64(scan(env, form, raw_ap, raw_bp, n, c, h, w, e)), raw64(got)[perm])


@pytest.mark.parametrize("form", FORMS_A)
def test_operator_images_without_a_compared_element_and_equal_tensors(env, form):
    n, c, h, w = 3, 11, 5, 7
    rng = np.random.default_rng(3)
    b = (rng.standard_normal((n, c, h, w)) * 3).astype(np.float32)
    a = b.copy()
    a[1] = np.nan                   # image 1: nothing compared
    b[1, ::2] = np.inf
    raw_a, raw_b, held_a, held_b = pack_pair(form, a, b, 0)
    if form in ("F32", "NCHW"):     # image 0 and 2: the same bits on both sides
        assert np.array_equal(held_a[0], held_b[0])
    got = scan(env, form, raw_a, raw_b, n, c, h, w, 0)
    D.assert_records(got, reference(form, held_a, held_b, 0), form)
    per = c * h * w
    assert got["n_compared"][1] == 0 and got["at"][1] == 0xFFFFFFFF and got["n_nonfinite_test"][1] == per
    for name in ("sum_abs_err", "sum_sq_err", "sum_sq_ref", "max_abs_err", "max_abs_ref", "max_abs_test"):
        assert got[name][1] == 0, name
    assert got["n_class_differs"][1] == per
    if form in ("F32", "NCHW"):
        assert got["max_abs_err"][0] == 0 and got["sum_abs_err"][0] == 0 and got["at"][0] == 0 and got["n_compared"][0] == per


@pytest.mark.parametrize("form", FORMS_A)
def test_operator_in_a_hip_graph(env, form):
    c, h, w, n, e = 40, 5, 7, 3, 0
    a, b = operands(17, form, n, c, h, w, e)
    raw_a, raw_b, _, _ = pack_pair(form, a, b, e)
    eager = scan(env, form, raw_a, raw_b, n, c, h, w, e)
    p = Pair(env, form, raw_a, raw_b, n, c, h, w, e)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p.launch()
    for _ in range(2):
        p.out.fill_(0xFF)
        p.ws.fill_(0xFF)
        g.replay()
        assert np.array_equal(raw64(p.records()), raw64(eager))


# ---- the network -------------------------------------------------------------------------------------------------------------
GOLDEN = {"hrnet2": ("tiny_hrnet2_64", "seg_hrnet2", 1), "hrnet3": ("small_hrnet3_64", "seg_hrnet3", 1)}
VALUE_CASES = [("hrnet2", "fp16"), ("hrnet2", "bf16"), ("hrnet2", "bf16x3"), ("hrnet3", "bf16")]


def _fixture(env, key):
    tag, module, cin = GOLDEN[key]
    g = np.load(os.path.join(env["golden_dir"], tag + ".npz"), allow_pickle=False)
    widths = tuple(int(v) for v in g["widths"])
    shapes = {str(k): tuple(int(v) for v in s.split(",")) if s else () for k, s in zip(g["state_keys"], g["state_shapes"])}
    sd = env["synth"].make_state_dict(shapes, seed=int(g["seed"]), gain=float(g["gain"]) if "gain" in g.files else 0.5)
    x = env["synth"].make_crops(2, cin, int(g["hw"]), int(g["hw"]), seed=int(g["seed"]))
    return module, widths, sd, x


def _net(env, key, precision, switches=(), sd=None):
    """A net of the golden's stage table and weights on the device, built (and run once: the device handle reads the plan
    switches when it is created) under `switches`; cached per module."""
    ck = (key, precision, tuple(switches), sd is None)
    if ck in env["nets"] and sd is None:
        return env["nets"][ck]
    module, widths, sd0, x = _fixture(env, key)
    for s in switches:
        os.environ[s] = "1"
    try:
        net = env[module].get_seg_model(env["config"].make_config(widths=widths), precision=precision)
        net.load_state_dict(sd if sd is not None else sd0, strict=True)
        net = net.cuda().eval()
        with torch.no_grad():
            net(x.cuda())
    finally:
        for s in switches:
            del os.environ[s]
    if sd is None:
        env["nets"][ck] = net
    return net


def _x(env, key):
    return _fixture(env, key)[3].cuda()


@pytest.mark.parametrize("key", ["hrnet2", "hrnet3"])
def test_pairing_is_exact_between_two_plans_of_the_same_arithmetic(env, key):
    """fp32 against an fp32 net built under ESAHRNET_NO_JOBS=1: other launches and labels, bit-identical tensors
    (tests/test_gpu_fp32.py: test_merged_branch_launches_and_their_fallback).  And a net against itself."""
    net, plain = _net(env, key, "fp32"), _net(env, key, "fp32", ("ESAHRNET_NO_JOBS",))
    x = _x(env, key)
    n, _, hh, ww = x.shape
    labels = [[d.name for d in m._rt.stats_rows(m._rt._probe, n, hh, ww)] for m in (net, plain)]
    assert labels[0] != labels[1] and any(b" + " in v for v in labels[0]) and not any(b" + " in v for v in labels[1])
    with torch.no_grad():
        heat = net(x)
        for ref in (plain, net):
            rep = net.precision_report(x, reference=ref)
            assert rep.keys[-1] == "heatmaps" and rep.compared[-1] and rep.per_image.shape == (len(rep.keys), n)
            scanned = sum(d.scanned for d in net._rt.stats_rows(net._rt._probe, n, hh, ww))
            assert rep.compared.sum() == scanned >= 99, "every scanned row pairs"
            assert torch.equal(rep.heatmaps, heat) and torch.equal(rep.heatmaps_ref, heat)
            for r, d in enumerate(rep.descs):
                rec = rep.per_image[r]
                if not rep.compared[r]:
                    assert not raw64(rec).any(), rep.keys[r]
                    continue
                assert np.all(rec["max_abs_err"] == 0) and np.all(rec["n_class_differs"] == 0), rep.keys[r]
                assert np.all(rec["n_compared"] == d.c * d.h * d.w) and np.all(rec["sum_abs_err"] == 0), rep.keys[r]
                assert np.all(rec["at"] == 0) and np.all(rec["max_abs_ref"] == rec["max_abs_test"]), rep.keys[r]
            assert len(rep.table().splitlines()) == len(rep.keys) + 1
            assert np.all(rep.rel_max() == 0) and np.all(rep.rel_rms() == 0)


@pytest.fixture(scope="module", params=VALUE_CASES, ids=lambda c: "-".join(c))
def case(request, env):
    key, precision = request.param
    net, ref = _net(env, key, precision), _net(env, key, "fp32")
    x = _x(env, key)
    with torch.no_grad():
        rep = net.precision_report(x, reference=ref)
        taps_a = {k: t.cpu().numpy() for k, t in net.taps(x).items()}
        taps_b = {k: t.cpu().numpy() for k, t in ref.taps(x).items()}
    return dict(key=key, precision=precision, net=net, ref=ref, x=x, rep=rep, taps_a=taps_a, taps_b=taps_b)


def test_report_against_the_taps_of_both_nets(env, case):
    rep, ta, tb = case["rep"], case["taps_a"], case["taps_b"]
    n = case["x"].shape[0]
    assert torch.equal(rep.heatmaps.cpu(), torch.from_numpy(ta["heatmaps"])) and torch.equal(rep.heatmaps_ref.cpu(), torch.from_numpy(tb["heatmaps"]))
    checked = 0
    for name in ta:
        if name not in tb or name not in rep.keys:
            continue
        r = rep.keys.index(name)
        if not rep.compared[r]:
            continue
        d = rep.descs[r]
        assert (d.c, d.h, d.w) == ta[name].shape[1:] == tb[name].shape[1:], name
        nchw = name == "heatmaps"
        want = (D.records_nchw if nchw else D.records_nhwc)(ta[name], tb[name])
        D.assert_records(rep.per_image[r], want, (name, case["precision"]))
        err = np.abs(ta[name] - tb[name])
        for i in range(n):      # `at` through where(): the first element, in the tensor's own storage order, that reaches the maximum
            c, y, x = rep.where(r, i)
            assert err[i, c, y, x] == rep.per_image["max_abs_err"][r, i] == err[i].max(), (name, i)
        checked += 1
    assert checked >= (8 if case["key"] == "hrnet2" else 9), sorted(ta)
    hm = (rep.heatmaps - rep.heatmaps_ref).abs().max()
    assert float(hm) == float(rep.max_abs_err()[-1]) and float(hm) > 0
    # an error model is not asserted; the figures, for the record
    worst = rep.worst(3)
    assert len(worst) == 3 and worst[0]["rel_max"] >= worst[1]["rel_max"] >= worst[2]["rel_max"] > 0
    print(f"\n{case['key']} {case['precision']}: {int(rep.compared.sum())} rows compared; heat-maps max_abs_err {float(hm):.3e} "
          f"rel_max {rep.rel_max()[-1]:.3e} rel_rms {rep.rel_rms()[-1]:.3e}; worst row {worst[0]['key']} rel_max {worst[0]['rel_max']:.3e}")
    # every row: compared rows count every element once, rows not compared are all zero
    for r, d in enumerate(rep.descs):
        rec = rep.per_image[r]
        if rep.compared[r]:
            assert np.all(rec["n_compared"].astype(np.int64) + np.maximum(rec["n_nonfinite_test"], rec["n_nonfinite_ref"]) <= d.c * d.h * d.w)
            assert np.all(rec["n_compared"] == d.c * d.h * d.w), rep.keys[r]         # (finite weights and crops: nothing non-finite)
        else:
            assert not raw64(rec).any(), rep.keys[r]
    assert "stem1" not in [k for k, c in zip(rep.keys, rep.compared) if c]


def test_the_twin_is_the_explicit_reference_and_the_batch_does_not_matter(env, case):
    net, x, rep = case["net"], case["x"], case["rep"]
    with torch.no_grad():
        twin = net.precision_report(x)              # reference=None: an fp32-grade twin from the net's own state dict
        assert np.array_equal(raw64(twin.per_image), raw64(rep.per_image)) and twin.keys == rep.keys
        assert torch.equal(twin.heatmaps_ref, rep.heatmaps_ref)
        moved = net.precision_report(x[[1, 0]].contiguous(), reference=case["ref"])
        assert np.array_equal(raw64(moved.per_image), raw64(rep.per_image)[:, [1, 0]])
        alone = net.precision_report(x[1:2].contiguous(), reference=case["ref"])
        assert np.array_equal(raw64(alone.per_image), raw64(rep.per_image)[:, 1:2])


def test_keypoints_of_the_report_against_the_host_decoders(env, case):
    rep, inf = case["rep"], env["inference"]
    for refine, host in (("get_final", inf.get_final), ("get_final2", inf.get_final2)):
        k = rep.keypoints(refine=refine)
        n = rep.heatmaps.shape[0]
        a = np.stack([host(rep.heatmaps[i:i + 1]) for i in range(n)])
        b = np.stack([host(rep.heatmaps_ref[i:i + 1]) for i in range(n)])
        assert np.array_equal(k["kp"][..., :2].cpu().numpy(), a) and np.array_equal(k["kp_ref"][..., :2].cpu().numpy(), b)
        shift = np.linalg.norm(a.astype(np.float64) - b.astype(np.float64), axis=-1)
        assert np.allclose(k["max_shift"], shift.max(axis=1), rtol=1e-12, atol=0)
        assert np.allclose(k["mean_shift"], shift.mean(axis=1), rtol=1e-12, atol=0)
        pa, _ = inf.get_max_preds(rep.heatmaps)
        pb, _ = inf.get_max_preds(rep.heatmaps_ref)
        assert k["argmax_differs"] == int((pa != pb).any(axis=-1).sum())


def _raw_forward_diff(env, net, ref, x, short=0, ws_shift=0, diff_shift=0, fill=0xFF):
    lib, L = env["lib"], env["L"]
    n, _, hh, ww = x.shape
    h, hr = net._rt._handle_for(net, x.device), ref._rt._handle_for(ref, x.device)
    need = C.c_size_t()
    L.check(lib.esahrnet_forward_diff_workspace_bytes(h, hr, n, hh, ww, C.byref(need)))
    rows = len(net._rt.stats_rows(h, n, hh, ww))
    ws = torch.full((need.value + 512,), fill, dtype=torch.uint8, device="cuda")
    ptr = ws.data_ptr() + (-ws.data_ptr()) % 256 + ws_shift
    heat = torch.full((2, n, net._k, hh, ww), float("nan"), device="cuda")
    rec = torch.full((rows * n * 64 + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.esahrnet_forward_diff(h, hr, x.data_ptr(), n, hh, ww, heat[0].data_ptr(), heat[1].data_ptr(), ptr, need.value - short,
                                   rec.data_ptr() + diff_shift, _stream())
    torch.cuda.synchronize()
    return rc, heat, rec[:rows * n * 64].cpu().numpy().reshape(rows, n, 64), need.value


def test_forward_diff_in_buffers_of_the_caller_and_its_refusals(env, case):
    lib, net, ref, x, rep = env["lib"], case["net"], case["ref"], case["x"], case["rep"]

    def err():
        return lib.esahrnet_last_error().decode()
    for fill in (0xFF, 0):          # every byte of diff_dev is written; what the workspace held does not matter
        rc, heat, rec, need = _raw_forward_diff(env, net, ref, x, fill=fill)
        assert rc == 0, err()
        assert np.array_equal(rec, raw64(rep.per_image))
        assert torch.equal(heat[0], rep.heatmaps) and torch.equal(heat[1], rep.heatmaps_ref)
    keep = C.c_size_t()
    small = C.c_size_t()            # the keep states are left as found
    env["L"].check(lib.esahrnet_workspace_bytes(net._rt._handle_for(net, x.device), 2, 64, 64, C.byref(small)))
    env["L"].check(lib.esahrnet_forward_stats_workspace_bytes(net._rt._handle_for(net, x.device), 2, 64, 64, C.byref(keep)))
    assert small.value < keep.value
    rc, _, _, need = _raw_forward_diff(env, net, ref, x, short=1)
    assert rc == 1 and err() == f"forward_diff: workspace too small ({need - 1} < {need})"
    rc, _, _, _ = _raw_forward_diff(env, net, ref, x, ws_shift=16)
    assert rc == 1 and err() == "forward_diff: workspace must be 256-byte aligned"
    rc, _, _, _ = _raw_forward_diff(env, net, ref, x, diff_shift=4)
    assert rc == 1 and err() == "forward_diff: diff_dev must be 8-byte aligned"
    rc, _, _, _ = _raw_forward_diff(env, net, ref, x, short=1, ws_shift=16, diff_shift=4)
    assert rc == 1 and err().startswith("forward_diff: workspace too small")
    h, hr = net._rt._handle_for(net, x.device), ref._rt._handle_for(ref, x.device)
    p = x.data_ptr()
    assert lib.esahrnet_forward_diff(h, hr, p, 2, 63, 64, p, p, p, 0, p, None) == 1 and err().startswith("crop 63x64")
    assert lib.esahrnet_forward_diff(h, hr, p, 0, 64, 64, p, p, p, 0, p, None) == 1 and err() == "batch must be positive (got 0)"
    other = _net(env, "hrnet3" if case["key"] == "hrnet2" else "hrnet2", "fp32")
    ho = other._rt._handle_for(other, x.device)
    assert lib.esahrnet_forward_diff(h, ho, p, 0, 63, 64, p, p, p, 0, p, None) == 1
    assert err().startswith("forward_diff: the handles differ in variant (")
    with pytest.raises(env["L"].EsaHrnetError, match="differ in variant"):
        net.precision_report(x, reference=other)
    with pytest.raises(RuntimeError, match="runs only on a GPU tensor"):
        net.precision_report(x.cpu())


def test_fp16_scale_exponents_enter_the_report_exactly(env):
    """The "hot" checkpoint of tests/fp16_scale_ref.py (every activation x 2^16) after calibrate_fp16, against the golden's own
    checkpoint after calibrate_fp16: the calibrated exponents differ by 16 everywhere, both nets store the same bits,
    the fp32-grade twins differ by the factor 2^16 exactly, so every record scales exactly: maxima and sum_abs_err x 2^16,
    sum_sq_* x 2^32, `at` and the counters unchanged."""
    _, _, sd, x = _fixture(env, "hrnet2")
    cases = FS.checkpoints(sd, x)
    reports = {}
    for tag in ("plain", "hot"):
        sd_t, x_t, _ = cases[tag]
        net = _net(env, "hrnet2", "fp16", sd=sd_t)
        with torch.no_grad():
            cal = net.calibrate_fp16(x_t.cuda())
            reports[tag] = (net.precision_report(x_t.cuda()), cal.exponents)
    (plain, e_plain), (hot, e_hot) = reports["plain"], reports["hot"]
    assert [b - a for a, b in zip(e_plain, e_hot)] == [16] * len(e_plain) and any(e_hot)
    assert plain.keys == hot.keys and np.array_equal(plain.compared, hot.compared)
    for dp, dh, c in zip(plain.descs, hot.descs, plain.compared):
        if c:
            assert dh.exponent == dp.exponent + (16 if dp.fmt == 3 else 0), dp.key
    assert any(d.exponent for d in plain.descs)
    s = 2.0 ** 16
    for name, t in env["L"].DIFF_FIELDS:
        p, h = plain.per_image[name], hot.per_image[name]
        if name in ("max_abs_err", "max_abs_ref", "max_abs_test"):
            assert np.array_equal(h, p * np.float32(s)), name
        elif name == "sum_abs_err":
            assert np.array_equal(h, p * s), name
        elif name.startswith("sum_sq"):
            assert np.array_equal(h, p * s * s), name
        else:
            assert np.array_equal(h, p), name
    assert float(plain.max_abs_err()[-1]) > 0
