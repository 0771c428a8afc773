"""Results must not depend on what the workspace held on entry (include/esahrnet.h: "allocates nothing", ws_dev).

Every forward-like entry point of the C ABI is run, at the ctypes level, inside buffers this file owns: the workspace and
every output are slices of larger tensors with a 1 MiB guard band of 0xA5 on either side, the outputs are prefilled with 0xFF,
and the call is made with the workspace holding (a) zeros, (b) 0xFF in every byte — NaN in f32 / bf16 / fp16 / f64, -1 as an
int32 — and (c) the residue of the same entry point on another input.  The three results must be bit-identical, the guards
untouched, every output fully overwritten and the inputs unchanged.  Zeros, which a freshly mapped torch.empty reads as, are
the one content that hides an unwritten padding channel, an unwritten halo or a region recycled while it is still read.
No pattern that reads as a large integer is used: a latent bug must land a stray index inside a guard band, never far away.
tests/test_workspace_plan_host.py checks the planner's recycling rule itself, on the host."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1 << 20
MEAN, STD = 0.45, 0.225
THRESH, MIN_K = 0.0, 4


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, seg_hrnet, seg_hrnet2, seg_hrnet3, synth
    return dict(lib=_lib.lib(), L=_lib, config=config, synth=synth, seg_hrnet=seg_hrnet, seg_hrnet2=seg_hrnet2,
                seg_hrnet3=seg_hrnet3)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


def _build(env, key, precision):
    """(net, handle): weights from synth.make_state_dict at gain 0.5.  esahrnet_create reads the environment as it is NOW."""
    module, cin, k, variant, widths = W.NETS[key]
    net = env[module].get_seg_model(env["config"].make_config(widths=widths), precision=precision)
    sd = env["synth"].make_state_dict({k_: v.shape for k_, v in net.state_dict().items()}, seed=53, gain=0.5)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    return net, net._rt._handle_for(net, torch.device("cuda", torch.cuda.current_device()))


@pytest.fixture(scope="module", params=[(k, p) for k in W.NETS for p in W.precisions(k)], ids=lambda c: "-".join(c))
def case(request, env):
    """One network in one precision, built once for the tests below, with no plan switch set."""
    saved = {k: os.environ.pop(k) for k in [k for k in os.environ if k.startswith("ESAHRNET_")]}
    try:
        key, precision = request.param
        net, h = _build(env, key, precision)
    finally:
        os.environ.update(saved)
    yield dict(key=key, precision=precision, net=net, h=h)
    del net
    torch.cuda.empty_cache()


# ---- the harness -----------------------------------------------------------------------------------------------------------
class Guarded:
    """`nbytes` device bytes, 256-byte aligned, between two guard bands of at least 1 MiB of 0xA5."""

    def __init__(self, nbytes, fill=None):
        self.nbytes = nbytes
        self.raw = torch.full((GUARD + 256 + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        self.ptr = self.raw.data_ptr() + self.off
        self.view = self.raw[self.off:self.off + nbytes]
        if fill is not None:
            self.view.fill_(fill)

    def guards_intact(self):
        lo, hi = self.raw[:self.off], self.raw[self.off + self.nbytes:]
        return lo.numel() >= GUARD and hi.numel() >= GUARD and bool((lo == 0xA5).all()) and bool((hi == 0xA5).all())

    def typed(self, dtype, shape):
        return self.view.view(dtype).view(shape)


_ALL_ONES = {4: (torch.int32, -1), 8: (torch.int64, -1)}


def _nbytes(dtype, shape):
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= s
    return n


def run_guarded(env, call, ws_bytes, inputs, inputs_other, out_specs, may_keep_ff=()):
    """Run `call(in_ptrs, out_ptrs, ws_ptr, ws_bytes)` (-> rc) with the workspace holding zeros, 0xFF, and the residue of
    the same call on `inputs_other`; returns the typed outputs of the first run after asserting everything the module
    docstring lists.  out_specs: name -> (dtype, shape).  may_keep_ff: outputs with a documented value that reads as 0xFF
    bytes (an int32 -1), which the caller checks itself."""
    lib = env["lib"]
    assert ws_bytes % 256 == 0 and ws_bytes > 0
    ws = Guarded(ws_bytes)
    assert ws.ptr % 256 == 0

    def once(ins):
        outs = {name: Guarded(_nbytes(dt, shp), fill=0xFF) for name, (dt, shp) in out_specs.items()}
        before = {name: t.clone() for name, t in ins.items()}
        rc = call({k: t.data_ptr() for k, t in ins.items()}, {k: g.ptr for k, g in outs.items()}, ws.ptr, ws_bytes)
        assert rc == 0, lib.esahrnet_last_error().decode(errors="replace")
        torch.cuda.synchronize()
        assert ws.guards_intact(), "the call wrote outside [ws_dev, ws_dev + ws_bytes)"
        for name, g in outs.items():
            assert g.guards_intact(), f"the call wrote outside output '{name}'"
            if name not in may_keep_ff:
                it, ones = _ALL_ONES[torch.empty((), dtype=out_specs[name][0]).element_size()]
                assert not bool((g.view.view(it) == ones).any()), f"output '{name}' was not fully overwritten"
        for name, t in ins.items():
            assert torch.equal(t.view(torch.uint8), before[name].view(torch.uint8)), f"input '{name}' was modified"
        return outs

    results = []
    for content in ("zeros", "0xFF", "residue"):
        if content == "zeros":
            ws.view.zero_()
        elif content == "0xFF":
            ws.view.fill_(0xFF)
        else:
            once(inputs_other)          # its leftovers stay in the workspace
        results.append((content, once(inputs)))
    first = results[0][1]
    for content, outs in results[1:]:
        for name in out_specs:
            # (bytes compared as integers: the same NaN masks and the same NaN bits)
            assert torch.equal(outs[name].view, first[name].view), f"output '{name}' differs with the workspace holding {content}"
    return {name: first[name].typed(*out_specs[name]) for name in out_specs}


def refused_guarded(env, call, ws_bytes, inputs, out_specs):
    """A workspace one 256-byte unit too small and one misaligned by 4 bytes are refused, and nothing was enqueued:
    guards, workspace and outputs keep their fill."""
    lib = env["lib"]
    for what, dptr, dbytes, word in (("small", 0, -256, b"too small"), ("misaligned", 4, 0, b"aligned")):
        ws = Guarded(ws_bytes + 256, fill=0xFF)
        outs = {name: Guarded(_nbytes(dt, shp), fill=0xFF) for name, (dt, shp) in out_specs.items()}
        before = {name: t.clone() for name, t in inputs.items()}
        rc = call({k: t.data_ptr() for k, t in inputs.items()}, {k: g.ptr for k, g in outs.items()}, ws.ptr + dptr,
                  ws_bytes + dbytes)
        assert rc != 0 and word in lib.esahrnet_last_error(), (what, lib.esahrnet_last_error())
        torch.cuda.synchronize()
        for name, g in list(outs.items()) + [("workspace", ws)]:
            assert g.guards_intact() and bool((g.view == 0xFF).all()), (what, name)
        for name, t in inputs.items():
            assert torch.equal(t.view(torch.uint8), before[name].view(torch.uint8)), (what, name)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _query(env, fn, *args):
    need = C.c_size_t()
    env["L"].check(fn(*args, C.byref(need)))
    return need.value


F32, I32, F64 = torch.float32, torch.int32, torch.float64


def _check_kp(out, n, k, hh, ww, rows=None):
    """kp finite, idx inside the plane (`rows`: the crops that are valid)."""
    rows = slice(None) if rows is None else rows
    assert bool(torch.isfinite(out["kp"][rows]).all())
    if "idx" in out:
        idx = out["idx"][rows]
        assert bool((idx >= 0).all()) and bool((idx < hh * ww).all())


# ---- the forward forms on crops ------------------------------------------------------------------------------------------------
def forward_entries(env, case):
    """name -> (workspace query, out_specs(n, hh, ww), call) for the entry points that take crops."""
    lib, h = env["lib"], case["h"]
    k = case["net"].num_keypoints
    ent = {}

    def add(name, query, specs, fn, order):
        def call_for(n, hh, ww):
            def call(i, o, wp, wb):
                return fn(h, i["x"], n, hh, ww, *[o[a] if a else None for a in order], wp, wb, _stream())
            return call
        ent[name] = (lambda n, hh, ww: _query(env, query, h, n, hh, ww), specs, call_for)

    kp = lambda n, hh, ww: {"kp": (F32, (n, k, 3)), "idx": (I32, (n, k))}                       # noqa: E731
    kph = lambda n, hh, ww: dict(kp(n, hh, ww), hess=(F64, (n, k, 3)))                          # noqa: E731
    add("forward", lib.esahrnet_workspace_bytes, lambda n, hh, ww: {"heat": (F32, (n, k, hh, ww))}, lib.esahrnet_forward, ["heat"])
    add("forward_keypoints", lib.esahrnet_keypoints_workspace_bytes, kp, lib.esahrnet_forward_keypoints, ["kp", "idx"])
    add("forward_keypoints_final2", lib.esahrnet_keypoints_final2_forward_workspace_bytes, kp,
        lib.esahrnet_forward_keypoints_final2, ["kp", "idx"])
    add("forward_keypoints_final2_hess", lib.esahrnet_keypoints_final2_forward_workspace_bytes, kph,
        lib.esahrnet_forward_keypoints_final2_hess, ["kp", "idx", "hess"])
    return ent


def run_forward_entry(env, case, name, shape, check=run_guarded):
    n, hh, ww = shape
    cin = W.NETS[case["key"]][1]
    k = case["net"].num_keypoints
    query, specs, call_for = forward_entries(env, case)[name]
    x = env["synth"].make_crops(n, cin, hh, ww, seed=11).cuda()
    if check is refused_guarded:
        return refused_guarded(env, call_for(n, hh, ww), query(n, hh, ww), {"x": x}, specs(n, hh, ww))
    other = env["synth"].make_crops(n, cin, hh, ww, seed=12).cuda()
    out = run_guarded(env, call_for(n, hh, ww), query(n, hh, ww), {"x": x}, {"x": other}, specs(n, hh, ww))
    if "heat" in out:
        assert bool(torch.isfinite(out["heat"]).all())
    else:
        _check_kp(out, n, k, hh, ww)
    return out


def run_partials(env, case, shape):
    """esahrnet_forward_partials where the handle reports tile maxima; its heat-maps and the reduced maxima."""
    lib, h = env["lib"], case["h"]
    n, hh, ww = shape
    cin, k = W.NETS[case["key"]][1], case["net"].num_keypoints
    nt = C.c_int(0)
    env["L"].check(lib.esahrnet_partial_tiles(h, hh, ww, C.byref(nt)))
    if nt.value <= 0:
        return None
    x = env["synth"].make_crops(n, cin, hh, ww, seed=11).cuda()
    other = env["synth"].make_crops(n, cin, hh, ww, seed=12).cuda()

    def call(i, o, wp, wb):
        return lib.esahrnet_forward_partials(h, i["x"], n, hh, ww, o["heat"], o["part"], wp, wb, _stream())
    out = run_guarded(env, call, _query(env, lib.esahrnet_workspace_bytes, h, n, hh, ww), {"x": x}, {"x": other},
                      {"heat": (F32, (n, k, hh, ww)), "part": (I32, (n * k, nt.value, 2))})
    assert bool(torch.isfinite(out["heat"]).all())
    part_idx = out["part"][..., 1]
    assert bool((part_idx >= 0).all()) and bool((part_idx < hh * ww).all())
    assert bool(torch.isfinite(out["part"][..., 0].contiguous().view(F32)).all())
    return out


def run_standalone_final2(env, heat, hess):
    """esahrnet_keypoints_final2(_hess) on heat-maps: its workspace holds tile maxima."""
    lib = env["lib"]
    n, k, hh, ww = heat.shape
    specs = {"kp": (F32, (n, k, 3)), "idx": (I32, (n, k))}
    if hess:
        specs["hess"] = (F64, (n, k, 3))

    def call(i, o, wp, wb):
        if hess:
            return lib.esahrnet_keypoints_final2_hess(i["heat"], n, k, hh, ww, o["kp"], o["idx"], o["hess"], wp, wb, _stream())
        return lib.esahrnet_keypoints_final2(i["heat"], n, k, hh, ww, o["kp"], o["idx"], wp, wb, _stream())
    other = torch.flip(heat, dims=(2, 3)).contiguous() * 0.5
    out = run_guarded(env, call, _query(env, lib.esahrnet_keypoints_final2_workspace_bytes, n, k, hh, ww), {"heat": heat},
                      {"heat": other}, specs)
    _check_kp(out, n, k, hh, ww)
    return out


# ---- the loader forms on frames ------------------------------------------------------------------------------------------------
def _scene(m, seed):
    """m gray frames of 96 x 128 and one detector box on each; the LAST box of m > 1 is empty: an invalid crop."""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (m, 96, 128), dtype=torch.uint8, generator=g)
    det = torch.tensor([[20 + 7 * i, 10 + 5 * i, 90 + 3 * i, 80 + 2 * i] for i in range(m)], dtype=torch.int32)
    if m > 1:
        det[m - 1] = torch.tensor([300, 300, 200, 200], dtype=torch.int32)
    return {"frames": frames.cuda(), "det": det.cuda()}


def run_frames(env, case, m, scale, decoder, mode=None, check=run_guarded):
    """esahrnet_frames_keypoints (mode None) / esahrnet_frames_correspondences: m boxes to crops of scale x scale."""
    lib, h = env["lib"], case["h"]
    k = case["net"].num_keypoints
    specs = {"kp": (F32, (m, k, 3)), "idx": (I32, (m, k)), "boxes": (I32, (m, 4)), "rates": (F64, (m,)), "valid": (I32, (m,))}
    if mode is None:
        need = _query(env, lib.esahrnet_frames_keypoints_workspace_bytes, h, m, scale, decoder)

        def call(i, o, wp, wb):
            return lib.esahrnet_frames_keypoints(h, i["frames"], m, 96, 128, 0, i["det"], None, m, scale, 0, MEAN, STD, decoder,
                                                 o["kp"], o["idx"], o["boxes"], o["rates"], o["valid"], wp, wb, _stream())
    else:
        specs.update(count=(I32, (m,)), order=(I32, (m, k)), pts=(F64, (m, k, 2)), w=(F64, (m, k, 3)))
        need = _query(env, lib.esahrnet_frames_correspondences_workspace_bytes, h, m, scale, decoder, mode)

        def call(i, o, wp, wb):
            return lib.esahrnet_frames_correspondences(h, i["frames"], m, 96, 128, 0, i["det"], None, m, scale, 0, MEAN, STD,
                                                       decoder, THRESH, MIN_K, mode, o["kp"], o["idx"], o["boxes"], o["rates"],
                                                       o["valid"], o["count"], o["order"], o["pts"], o["w"], wp, wb, _stream())
    if check is refused_guarded:
        return refused_guarded(env, call, need, _scene(m, 21), specs)
    # documented values that read as 0xFF bytes: idx -1 of an invalid crop, order -1 beyond count — checked below
    out = run_guarded(env, call, need, _scene(m, 21), _scene(m, 22), specs, may_keep_ff=("idx", "order"))
    valid = out["valid"].bool()
    assert valid.tolist() == [True] * (m - 1) + [m == 1]
    _check_kp(out, m, k, scale, scale, rows=valid)
    if not bool(valid.all()):      # the documented record of an invalid crop: NaN keypoints, index -1
        assert bool(torch.isnan(out["kp"][~valid]).all()) and bool((out["idx"][~valid] == -1).all())
    if mode is not None:
        count, order = out["count"], out["order"]
        assert bool((count[valid] >= MIN_K).all()) and bool((count <= k).all()) and bool((count[~valid] == 0).all())
        beyond = torch.arange(k, device=count.device)[None, :] >= count[:, None]
        assert bool((order[beyond] == -1).all()) and bool((order[~beyond] >= 0).all()) and bool((order[~beyond] < k).all())
        assert bool((out["pts"][beyond] == 0).all()) and bool((out["w"][beyond] == 0).all())
        assert bool(torch.isfinite(out["pts"]).all()) and bool(torch.isfinite(out["w"]).all())
    return out


# ---- 1. every entry point, network, precision and shape --------------------------------------------------------------------
def test_results_do_not_depend_on_the_workspace_contents(env, case):
    key = case["key"]
    agreed = []
    for shape in W.shapes(key):
        heat = run_forward_entry(env, case, "forward", shape)["heat"]
        agreed.append(("forward", shape))
        if run_partials(env, case, shape) is not None:
            agreed.append(("forward_partials", shape))
        for name in ("forward_keypoints", "forward_keypoints_final2", "forward_keypoints_final2_hess"):
            run_forward_entry(env, case, name, shape)
            agreed.append((name, shape))
        for hess in (False, True):
            run_standalone_final2(env, heat.clone(), hess)
        agreed.append(("keypoints_final2(+hess)", shape))
    if W.NETS[key][1] == 1:         # the loader makes 1-channel crops
        for m, scale in ((2, 64), (3, 48), (1, 18)):
            for decoder in (0, 1):
                run_frames(env, case, m, scale, decoder)
            for decoder, mode in ((0, 0), (1, 0), (1, 1)):
                run_frames(env, case, m, scale, decoder, mode)
            agreed.append(("frames_keypoints d0 d1, frames_correspondences d0m0 d1m0 d1m1", (m, scale, scale)))
    print(f"{key} {case['precision']}: zeros / 0xFF / residue agreed bit for bit:", "; ".join(f"{a} {s}" for a, s in agreed))


# ---- 2. recycling changes no bit -------------------------------------------------------------------------------------------
def _heat_ff(env, pair, x, keep):
    """esahrnet_forward (keep: esahrnet_set_debug_keep) in a guarded workspace of its own queried size, filled with 0xFF."""
    lib = env["lib"]
    net, h = pair
    n, _, hh, ww = x.shape
    k = net.num_keypoints
    env["L"].check(lib.esahrnet_set_debug_keep(h, keep))
    try:
        need = _query(env, lib.esahrnet_workspace_bytes, h, n, hh, ww)
        ws = Guarded(need, fill=0xFF)
        heat = Guarded(n * k * hh * ww * 4, fill=0xFF)
        env["L"].check(lib.esahrnet_forward(h, x.data_ptr(), n, hh, ww, heat.ptr, ws.ptr, need, _stream()))
        torch.cuda.synchronize()
        assert ws.guards_intact() and heat.guards_intact()
        return need, heat.view.clone()
    finally:
        env["L"].check(lib.esahrnet_set_debug_keep(h, 0))


def test_recycled_plan_equals_the_unrecycled_one(env, case):
    """esahrnet_set_debug_keep(h, 1) gives every tensor a region of its own; the recycled plan must give the same bits."""
    n, hh, ww = 2, 48, 80
    x = env["synth"].make_crops(n, W.NETS[case["key"]][1], hh, ww, seed=11).cuda()
    need0, heat0 = _heat_ff(env, (case["net"], case["h"]), x, 0)
    need1, heat1 = _heat_ff(env, (case["net"], case["h"]), x, 1)
    print(f"{case['key']} {case['precision']}: workspace {need0} B recycled, {need1} B kept")
    assert need1 > need0
    assert torch.equal(heat0, heat1)
    assert bool(torch.isfinite(heat0.view(F32)).all())


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,precision", [("hrnet2_w32", "fp32"), ("hrnet2_w32", "bf16"), ("hrnet3_w16", "fp32")])
def test_refusals_enqueue_nothing(env, key, precision):
    net, h = _build(env, key, precision)
    case = dict(key=key, precision=precision, net=net, h=h)
    for name in ("forward", "forward_keypoints", "forward_keypoints_final2", "forward_keypoints_final2_hess"):
        run_forward_entry(env, case, name, (2, 64, 64), check=refused_guarded)
    run_frames(env, case, 2, 64, 0, check=refused_guarded)
    run_frames(env, case, 2, 64, 1, 1, check=refused_guarded)
    lib = env["lib"]
    heat = env["synth"].make_gaussian_heatmaps(2, 5, 48, 80, seed=3).cuda()

    def call(i, o, wp, wb):
        return lib.esahrnet_keypoints_final2_hess(i["heat"], 2, 5, 48, 80, o["kp"], o["idx"], o["hess"], wp, wb, _stream())
    refused_guarded(env, call, _query(env, lib.esahrnet_keypoints_final2_workspace_bytes, 2, 5, 48, 80), {"heat": heat},
                    {"kp": (F32, (2, 5, 3)), "idx": (I32, (2, 5)), "hess": (F64, (2, 5, 3))})


# ---- 4. the plan switches, each on its own ---------------------------------------------------------------------------------
SWITCH_ENTRIES = ("forward", "forward_keypoints", "forward_keypoints_final2_hess")


@pytest.mark.parametrize("switch,key,precision", W.switch_cases())
def test_plan_switches(env, monkeypatch, switch, key, precision):
    monkeypatch.setenv("ESAHRNET_" + switch, "1")
    net, h = _build(env, key, precision)            # a fresh net: esahrnet_create reads the environment
    case = dict(key=key, precision=precision, net=net, h=h)
    for shape in (W.shapes(key)[0], W.shapes(key)[2]):
        for name in SWITCH_ENTRIES:
            run_forward_entry(env, case, name, shape)
        run_partials(env, case, shape)
    print(f"ESAHRNET_{switch}=1 {key} {precision}: zeros / 0xFF / residue agreed bit for bit ({', '.join(SWITCH_ENTRIES)})")


@pytest.mark.parametrize("key,precision", [(k, p) for k in ("hrnet2_w32", "hrnet3_w48") for p in W.precisions(k)])
def test_two_lanes(env, monkeypatch, key, precision):
    """ESAHRNET_STREAMS=2 (the wave executor, eager): the same independence, and the bits of the one-lane handle.  On the
    W32 / W48 nets, as for the other plan switches; tests/test_workspace_plan_host.py checks the two-lane plan of every net."""
    x = env["synth"].make_crops(2, W.NETS[key][1], 48, 80, seed=11).cuda()
    one = _build(env, key, precision)
    _, heat1 = _heat_ff(env, one, x, 0)
    monkeypatch.setenv("ESAHRNET_STREAMS", "2")
    net, h = _build(env, key, precision)
    case = dict(key=key, precision=precision, net=net, h=h)
    for shape in (W.shapes(key)[0], W.shapes(key)[2]):
        for name in SWITCH_ENTRIES:
            run_forward_entry(env, case, name, shape)
    _, heat2 = _heat_ff(env, (net, h), x, 0)
    _, heat2k = _heat_ff(env, (net, h), x, 1)
    assert torch.equal(heat2, heat1) and torch.equal(heat2k, heat1)
    print(f"ESAHRNET_STREAMS=2 {key} {precision}: zeros / 0xFF / residue agreed; lanes and keep change no bit")
