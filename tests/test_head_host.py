"""What the CPU can say about the head and the output layer (tests/head_ref.py; the GPU half is tests/test_gpu_head.py):

  * the two float64 sections, fed oracle.hrnet_ref.forward's own stage-4 tensors, reproduce its head3 and heat-maps for all
    three variants: the section reference IS the reference model's head;
  * the per-format emulations reproduce oracle.emulate_bf16.forward and fp16_emu.forward_plan bit for bit from those forwards'
    own stage-4 tensors, and stay within a few storage quanta of the float64 sections in every format;
  * the open-ReLU condition of the GPU cases (>= 90 % of head0's pre-activations positive) holds on the float64 reference in
    every regime, at every configuration and crop of the GPU table;
  * the selection sweep: for every configuration of the GPU table and every legal crop with sides 16..512, read from
    esahrnet_op_desc_get, exactly one head alternative is listed, it is one the channel rules of plan_options allow, and it is
    the form the GPU cases claim.  The table it prints (run with -s) is copied into DESIGN.md.
"""
import concurrent.futures
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp16_emu  # noqa: E402
import head_ref as HR  # noqa: E402
import resample_ref as R  # noqa: E402
from oracle import emulate_bf16 as EB  # noqa: E402
from oracle import hrnet_ref  # noqa: E402

SMALL = (16, 32, 64, 128)         # seg_hrnet3's ChannelAttention needs C // 16 >= 1
SMALL_HW = (34, 50, 2)


def _stage4(taps):
    return [taps[f"stage4.{b}"] for b in range(4)]


@pytest.fixture(scope="module")
def small():
    """variant -> (Config, sd, crops, the oracle's float64 taps and heat-maps)."""
    out = {}
    for variant, K in (("seg_hrnet", 32), ("seg_hrnet2", 11), ("seg_hrnet3", 30)):
        c = HR.Config(variant, SMALL, K, 0, ())
        _, sd = HR.build_net(c)
        x = HR.crops(c, SMALL_HW)
        taps = {}
        with torch.no_grad():
            y = hrnet_ref.forward(sd, HR.oracle_cfg(c), x.double(), taps)
        out[variant] = (c, sd, x, taps, y)
    return out


@pytest.mark.parametrize("variant", ["seg_hrnet", "seg_hrnet2", "seg_hrnet3"])
def test_sections_are_the_reference_models_head(small, variant):
    """Both run in float64, so they agree to the float64 rounding of two different orders (BatchNorm folded or applied):
    far below one f32 ulp, which is what the issue asks for."""
    c, sd, x, taps, y = small[variant]
    v = HR.VARIANT[variant]
    with torch.no_grad():
        r = HR.head_section(sd, _stage4(taps), v)
        x0 = hrnet_ref._cbam(sd, "", taps["stem_raw"]) if v else x.double()
        out = HR.output_section(sd, taps["head3"], x0)
    for name, got, ref in (("head0", r["head0"], taps["head0"]), ("head3", r["head3"], taps["head3"]), ("heatmaps", out, y),
                           ("head3 from head0", HR.head3_section(sd, taps["head0"]), taps["head3"])):
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"{variant} {name}: section vs oracle (both f64) {err:.2e} of the scale")
        assert got.dtype == torch.float64 and ref.dtype == torch.float64
        assert err <= 2.0 ** -40, (name, err)


@pytest.mark.parametrize("precision", [1, 3])
def test_emulations_are_the_emulators_head(small, precision):
    """oracle.emulate_bf16.forward (bf16) / fp16_emu.forward_plan (fp16) keep their stage-4 tensors: from those, the section
    emulations return the same bits as the forwards themselves, head3 and heat-maps."""
    c, sd, x, _, _ = small["seg_hrnet2"]
    taps = {}
    if precision == 1:
        with torch.no_grad():
            y = EB.forward(sd, HR.oracle_cfg(c), x, taps)
            e = HR.head_emulation(sd, _stage4(taps), 0, 1)
            out = HR.output_emulation(sd, taps["head3"], x, 0, 1, "valu")
    else:
        y = fp16_emu.forward_plan(sd, HR.oracle_cfg(c), x, taps)
        with fp16_emu._threads(fp16_emu.EMU_THREADS):
            e = HR.head_emulation(sd, _stage4(taps), 0, 3)
            out = HR.output_emulation(sd, taps["head3"], x, 0, 3, "valu")
    assert torch.equal(e["head0"], taps["head0"])
    assert torch.equal(e["head3"], taps["head3"])
    assert torch.equal(out, y)


@pytest.mark.parametrize("variant,precision", [("seg_hrnet2", p) for p in (0, 1, 2, 3)] + [("seg_hrnet3", p) for p in (0, 1, 2)])
def test_emulations_stay_near_the_sections(small, variant, precision):
    """Each emulation rounds a handful of times: its distance to the float64 section, on inputs that are data of the format,
    is a few storage quanta of the scale (64 allows for the 1x1 over 240 channels amplifying head0's roundings).  seg_hrnet3
    has no fp16 mode."""
    c, sd, x, taps, _ = small[variant]
    v = HR.VARIANT[variant]
    q = HR.QSTORE[precision]
    ys = [q(t.float()) for t in _stage4(taps)]
    with torch.no_grad():
        ref = HR.head_section(sd, ys, v)
        emu = HR.head_emulation(sd, ys, v, precision)
        h3 = emu["head3"]
        x0 = q(hrnet_ref._cbam(sd, "", taps["stem_raw"]).float()) if v else x
        oref = HR.output_section(sd, h3, x0)
    for name in ("head0", "head3"):
        err = (emu[name].double() - ref[name]).abs().max().item() / ref[name].abs().max().item()
        print(f"{variant} p{precision} {name}: emulation vs f64 {err:.2e} of the scale (quantum {HR.QUANTUM[precision]:.2e})")
        assert err <= 64 * HR.QUANTUM[precision], (name, err)
        if precision != 2:
            assert torch.equal(q(emu[name]), emu[name])
    for form in (("conv",) if v else ("valu", "mfma")):
        o = HR.output_emulation(sd, h3, x0, v, precision, form)
        err = (o.double() - oref).abs().max().item() / oref.abs().max().item()
        print(f"{variant} p{precision} output {form}: emulation vs f64 {err:.2e} of the scale")
        assert err <= 64 * (HR.QUANTUM[precision] if form == "conv" else HR.QUANTUM[0] if form == "mfma" else HR.Q_F32), err


# ------------------------------------------------------------------------------------------------ the open-ReLU condition
def _open_cases():
    seen, out = set(), []
    for c, shapes, _, _ in HR.GPU_CASES:
        for s in shapes:
            key = (c.variant, c.widths, c.K, s)
            if key not in seen:
                seen.add(key)
                out.append((c, s))
    return out


@pytest.mark.parametrize("case", _open_cases(), ids=lambda cs: f"{HR.cfg_id(cs[0]._replace(precision=2, switches=()))}-{cs[1][0]}x{cs[1][1]}")
def test_relu_is_open_on_the_reference(case):
    """Every regime of every GPU case: the float64 reference's head0 pre-activation is positive at >= 90 % of its elements
    (stage-4 tensors from the oracle's forward here; the GPU test asserts the same on the tapped ones)."""
    c, shape = case
    _, sd = HR.build_net(c._replace(precision=2, switches=()))
    x = HR.crops(c, shape)
    taps = {}
    with torch.no_grad():
        hrnet_ref.forward(sd, HR.oracle_cfg(c), x, taps)
        for regime in HR.REGIMES:
            r = HR.head_section(HR.regime_sd(sd, c.widths, regime), _stage4(taps), HR.VARIANT[c.variant])
            frac = HR.open_fraction(r["pre"])
            live = float((r["head3"] > 0).double().mean())
            print(f"{HR.cfg_id(c)} {shape} {regime}: pre-activation > 0 at {100 * frac:.1f} %, std {r['pre'].std().item():.3f}; "
                  f"head3 > 0 at {100 * live:.1f} %")
            assert frac >= 0.90, (regime, frac)
            assert live >= 0.25, (regime, live)            # the second ReLU leaves enough of the map to look at


# ------------------------------------------------------------------------------------------------ the selection sweep
SIDES = list(range(16, 514, 2))


def _net_with_switches(c):
    """The configuration's net (CPU only: its probe handle plans without a GPU), created with exactly its switches set."""
    env = {k: os.environ.pop(k) for k in [k for k in os.environ if k.startswith("ESAHRNET_")]}
    try:
        for s in c.switches:
            os.environ["ESAHRNET_" + s] = "1"
        net, _ = HR.build_net(c)
    finally:
        for s in c.switches:
            del os.environ["ESAHRNET_" + s]
        os.environ.update(env)
    return net


def _sweep_forms(net, c):
    """{form: [number of crops, smallest crop]} over every legal crop with sides 16..512.  An op list is classified
    (head_ref.head_form, which asserts "exactly one alternative") once per distinct list."""
    import ctypes as C
    from esa_pose_estimation_amd import _lib
    rt = net._rt
    nops = rt.launch_count()
    get, probe, d = rt.lib.esahrnet_op_desc_get, rt._probe, _lib.OpDesc()
    ref = C.byref(d)
    idx = range(HR.first_head_op(rt.lib, probe, nops), nops)
    known, forms = {}, {}
    for h in SIDES:
        for w in SIDES:
            rows = []
            for i in idx:
                assert get(probe, i, 2, h, w, ref) == 0
                if d.kernel:
                    rows.append((i, d.kernel, d.label))
            rows = tuple(rows)
            f = known.get(rows)
            if f is None:
                f = known[rows] = HR.head_form([(i, k.decode(), lab.decode()) for i, k, lab in rows], HR.VARIANT[c.variant])
            ent = forms.setdefault(f, [0, (h, w)])
            ent[0] += 1
            if h * w < ent[1][0] * ent[1][1]:
                ent[1] = (h, w)
    return forms


@pytest.fixture(scope="module")
def sweep():
    """Config -> {form: [crops, smallest crop]}.  The nets are created one after the other (the switches are process
    environment).  The split-bf16 configurations that carry head_fused2 spend their time inside the library (its predicate
    scans the interpolation weights of a crop for the lo part of U, ~40 us a call): those sweeps run side by side on separate
    handles; the others, a few us a call, gain nothing from threads and run one after the other."""
    cfgs = [c for c, _, _, _ in HR.GPU_CASES]
    nets = {c: _net_with_switches(c) for c in cfgs}
    heavy = [c for c, _, form, _ in HR.GPU_CASES if form == "head_fused2"]
    with concurrent.futures.ThreadPoolExecutor(max(1, min(len(heavy), os.cpu_count() or 1))) as ex:
        res = dict(zip(heavy, ex.map(lambda c: _sweep_forms(nets[c], c), heavy)))
    for c in cfgs:
        if c not in res:
            res[c] = _sweep_forms(nets[c], c)
    print("\nconfiguration: crops with sides 16..512 (even) -> head form / output layer")
    for c in cfgs:
        print(f"  {HR.cfg_id(c):40s} " + ", ".join(f"{n} -> {f}" for f, (n, _) in res[c].items()) + f" / {HR.expect_final(c)}")
    return res


@pytest.mark.parametrize("case", HR.GPU_CASES, ids=lambda cs: HR.cfg_id(cs[0]))
def test_selection_sweep(sweep, case):
    c, shapes, form, final = case
    forms = sweep[c]
    assert sum(n for n, _ in forms.values()) == len(SIDES) ** 2           # (head_form asserted "exactly one" at each)
    allowed = HR.expect_fused_possible(c) | ({"unfused"} if HR.VARIANT[c.variant] == 0 else set())
    assert set(forms) <= allowed, (set(forms), allowed)
    # No window predicate rejects a legal crop up to 512 today, so one form serves every crop of a configuration and the GPU
    # table has no boundary crops.  If this fails, a predicate has started to reject: add the smallest rejected crop and its
    # accepted neighbours to head_ref.GPU_CASES (forms[...][1] is the smallest crop of each form).
    assert set(forms) == {form}, {f: v for f, v in forms.items()}
    assert HR.expect_final(c) == final
    for h, w, n in shapes:
        assert h in SIDES and w in SIDES


def test_first_generation_windows_fit_every_crop():
    """head_fused is launched without asking its predicate at plan time (a crop it cannot serve fails the forward): its
    window rule — per 16-pixel tile at most 11 / 7 / 5 source rows or columns of branches 1 / 2 / 3 — restated with the tap
    rule of resample_ref, holds for every side 16..512."""
    for s in SIDES:
        chain = R.level_chain((s + 1) // 2)
        out = chain[0]
        for b, inn in enumerate(chain[1:]):
            i0, i1, _, _ = R.taps(inn, out, 0, fused=False)
            for o in range(0, out, 16):
                span = i1[min(o + 15, out - 1)] - i0[o] + 1
                assert span <= (11, 7, 5)[b], (s, b, o, span)


def test_ulo_claims():
    """The crops at which head_fused2 needs the lo part of U (weights that are no bf16 numbers), by its own rule."""
    for (h, w), ulo in HR.ULO.items():
        assert HR.needs_ulo(h, w) == ulo, (h, w)
