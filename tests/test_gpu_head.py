"""The head (last_layer[0..5]) and the output layer held to a float64 reference of their own, form by form.

Every case builds a net (cached per configuration: variant, widths, K, precision, plan switches), runs taps() on seeded
crops and cuts the network behind stage 4: head3 is compared with head_ref.head_section of the TAPPED stage4.* tensors, the
heat-maps with head_ref.output_section of the TAPPED head3 and the crop (seg_hrnet3: head0 and head3 separately, the output
layer from the tapped head3 and the CBAM'd skip the library keeps in head_cat2).  taps() returns exact f32 copies of what the
device holds, so the reference reads the very numbers the kernel read, and the bound has to leave room for one section only.
Which form ran is asserted by kernel name (esahrnet_op_desc_get on the handle that ran; the matrix-core output layer by its
per-tile maxima, esahrnet_partial_tiles).  op_desc_get does not tell head_fused_bf's matrix-core interpolation from its VALU one
(ESAHRNET_BF_HEAD_VALU) nor head_fused2 with the lo part of U from without: the first is the configuration's switch, the second
follows from the crop (head_ref.needs_ulo, tests/test_head_host.py::test_ulo_claims).

Configurations, crops and claimed forms: head_ref.GPU_CASES; tests/test_head_host.py sweeps the plan over every legal crop
with sides 16..512 for each configuration and finds every claimed form chosen — and no crop at which a window predicate
rejects, so the fallback forms are reached through the switches and channel rules only (no boundary crops to add).

What each crop is there to catch:
  16x16    branch grids 8 / 4 / 2 / 1: a one-pixel source, i1 = i0 in every branch; the image is smaller than a head tile
  18x34    grids 9x17 / 5x9 / 3x5 / 2x3: weights that are no bf16 numbers (head_fused2's lo part of U), ry != rx
  70x50    odd level sizes 35x25 / 18x13 / 9x7 / 5x4: the last row and column of every window
  36x132   n = 3: several tiles along x, one along y; the per-image base of every branch and the pitch of the T layout
  48x80, 104x72   several tiles both ways, a partial last tile
Weight regimes (head_ref.regime_sd), both on seeded synth weights: "b0".."b3" keep one branch's slice of last_layer.0 (an
error in that branch's interpolation reaches the output undiluted), "open" keeps all; every regime shifts last_layer.1's folded
bias by head_ref.OPEN_SHIFT, and the case asserts on the float64 reference that head0's pre-activation is positive at >= 90 %
of its elements, so no clamp hides a wrong sum.

Bound, one rule in every precision and on both sections, taken against the reference only:
    |HIP - f64|_max <= 2 x E_emu + q x max|ref|,        E_emu = max |emulation of the format - f64| on the same inputs
(head_ref.head_emulation / output_emulation: the format's roundings where it stores).  q = 2.4e-7 with the torch float32
emulation in the fp32-grade mode (test_op_conv_fp32_grade's rule and slack); otherwise one storage quantum of the result: 2^-17
split-bf16, 2^-9 bf16, 2^-12 fp16; the output layer's result is f32, q = 2.4e-7.  In the 16-bit modes head3 must be data of
its format.  Every case prints the HIP error, E_emu and error / bound (run with -s).

Measured on an MI355X (393 cases in 27 s, none above 0.9 s; worst error / bound per form and precision, with the HIP
error and E_emu of that case):
  head   head_fused2             split-bf16  0.50  (1.40e-5, 9.4e-6; b3, 16x16)
         head_fused              split-bf16  0.47  (3.5e-5, 2.8e-5; W18, open, 18x34)
         slices + fuse + 1x1     split-bf16 0.54 (3.2e-5, 2.4e-5)   bf16 0.46 (1.59e-2, 1.59e-2)   fp16 0.50 (2.3e-3, 2.1e-3)
                                 fp32-grade 0.26 (1.1e-6, 1.7e-6)
         head_fused_bf           bf16 0.61 (9.4e-3, 6.5e-3; b3, 16x16)   fp16 0.88 (1.45e-3, 6.8e-4; b3, 16x16)
         head_x6                 fp32-grade 0.23 (8.5e-7, 1.55e-6)
         seg_hrnet3 gather       split-bf16 0.43   fp32-grade 0.36;   direct  split-bf16 0.46   bf16 0.45   fp32-grade 0.49
  output final_mfma_kernel       split-bf16 0.52 (1.17e-5, 1.11e-5)   bf16 0.51   fp16 0.54
         final_kernel (VALU)     split-bf16 0.44   bf16 0.45   fp32-grade 0.68 (8.7e-7, 4.5e-7)
         seg_hrnet3              split-bf16 0.53   bf16 0.50   fp32-grade 0.38
A ratio near 0.5 means kernel and emulation round to the same value at the worst element.  No emulation needed a rounding point
added after the measurement (final_mfma_kernel's split-bf16 arithmetic was read from head.hip beforehand), and no defect was found.

Teeth, checked once on two scratch builds with a one-line mutation each:
  * head_fused2 without the lo part of U (`if (ULO)` off): 22 of the 45 split-bf16 second-generation cases fail — "open" and
    every single-branch regime whose branch has non-dyadic weights at the crop (18x34, 70x50: b1, b2, b3; 36x132: b2, b3;
    104x72: b3; W32, W48, every K), head3 error 8.3e-4 .. 4.8e-3, 12 .. 66 times the bound; 16x16, 48x80, b0 and the
    branches at an exact 2x / 4x ratio pass, as they must.  The whole-network tests at these
    crops notice it barely: test_odd_geometry_head_carries_lo_weights and test_odd_shapes_match_oracle (40x56, 18x34, 104x72)
    measure 4.3e-4 .. 4.9e-4 against GUARD = 2e-4.
  * head_fused taking column i0 for i1 in branch 3: the b3 and open cases of ESAHRNET_HEAD_V1 and of W18 fail at every crop
    but 16x16 (a one-pixel source), 12 cases, head3 error 0.20 .. 0.50, 2500 .. 7400 times the bound.  Of the whole-network
    tests only test_both_head_generations_match_reference_golden[True] (128x128) runs head_fused at all: 0.089 against 2e-4.
"""
import ctypes as C
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as HR  # noqa: E402

pytestmark = pytest.mark.gpu

ONLY_OPEN = ("open",)


def _regimes(c):
    """Every regime per head form; the rows that vary K or the output layer reuse a form that has them all and run "open"."""
    return ONLY_OPEN if (c.K not in (11, 30) or c.variant == "seg_hrnet" or "FINAL_VALU" in c.switches) else HR.REGIMES


CASES = [(c, regime, shape, form, final) for c, shapes, form, final in HR.GPU_CASES for regime in _regimes(c) for shape in shapes]


def _case_id(case):
    c, regime, (h, w, n), _, _ = case
    return f"{HR.cfg_id(c)}-{regime}-{h}x{w}"


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, fold
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return dict(lib=_lib.lib(), L=_lib, fold=fold, nets={})


def _net(env, monkeypatch, c):
    """The configuration's net, its state dict and handle; one configuration is kept at a time (the cases come grouped)."""
    ent = env["nets"].get(c)
    if ent is None:
        env["nets"].clear()
        for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
            monkeypatch.delenv(k)
        for s in c.switches:
            monkeypatch.setenv("ESAHRNET_" + s, "1")
        net, sd = HR.build_net(c)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval()
        handle = net._rt._handle_for(net, torch.device("cuda", torch.cuda.current_device()))    # created under the switches
        nops = net._rt.launch_count()
        first = HR.first_head_op(env["lib"], handle, nops)
        ent = env["nets"][c] = dict(net=net, sd=sd, handle=handle, nops=nops, first=first, regime=None, sdr=None)
    return ent


def _set_regime(env, ent, c, regime):
    """The regime's last_layer.0 / last_layer.1 into the handle (one convolution of the plan: fold, set, commit)."""
    if ent["regime"] != regime:
        sdr = HR.regime_sd(ent["sd"], c.widths, regime)
        net, lib, L = ent["net"], env["lib"], env["L"]
        (i, d), = [(i, d) for i, d in enumerate(net._descs) if d["name"] == "last_layer.0"]
        w, b = env["fold"].fold_conv(sdr, d["name"], d["bn"], d["has_bias"])
        L.check(lib.esahrnet_set_conv(ent["handle"], i, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
        torch.cuda.synchronize()
        with torch.cuda.device(torch.cuda.current_device()):
            L.check(lib.esahrnet_commit(ent["handle"]))
        ent["regime"], ent["sdr"] = regime, sdr
    return ent["sdr"]


def _hold(tag, y, ref, emu, q):
    """|HIP - f64| <= 2 E_emu + q max|ref|, printed before it is asserted."""
    assert y.shape == ref.shape, (tag, y.shape, ref.shape)
    assert bool(torch.isfinite(y).all()), tag
    scale = ref.abs().max().item()
    err = (y.double() - ref).abs().max().item()
    e_emu = (emu.double() - ref).abs().max().item()
    bound = 2.0 * e_emu + q * scale
    print(f"  {tag}: HIP vs f64 {err:.3e}   E_emu {e_emu:.3e}   scale {scale:.2f}   error / bound {err / bound:.3f}")
    assert err <= bound, (tag, err, e_emu, scale, bound)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_head_and_output_layer(env, monkeypatch, case):
    c, regime, shape, form, final = case
    h, w, n = shape
    v, p = HR.VARIANT[c.variant], c.precision
    t0 = time.time()
    ent = _net(env, monkeypatch, c)
    sdr = _set_regime(env, ent, c, regime)
    x = HR.crops(c, shape)
    with torch.no_grad():
        taps = {k: t.cpu() for k, t in ent["net"].taps(x.cuda()).items()}
    torch.cuda.synchronize()

    # ---- the form that ran
    rows = HR.head_ops(env["lib"], ent["handle"], ent["nops"], n, h, w, ent["first"])
    assert HR.head_form(rows, v) == form, [k for _, k, _ in rows]
    assert HR.final_form(env["lib"], ent["handle"], v, p, h, w) == final
    ulo = f", lo part of U: {HR.needs_ulo(h, w)}" if form == "head_fused2" else ""
    print(f"\n{_case_id(case)}: {form} / {final}{ulo}")

    # ---- the head
    q = HR.QSTORE[p]
    ys = [taps[f"stage4.{b}"] for b in range(4)]
    with torch.no_grad():
        ref = HR.head_section(sdr, ys, v)
        emu = HR.head_emulation(sdr, ys, v, p)
    frac = HR.open_fraction(ref["pre"])
    assert frac >= 0.90, frac                                          # a condition on the inputs: the ReLU is open
    h3 = taps["head3_fused"] if "head3_fused" in taps else taps["head3"]
    if p in (1, 3):
        assert torch.equal(q(h3), h3)                                   # data of its format
        assert all(torch.equal(q(t), t) for t in ys)
    if "head0" in taps:                                                 # the materialised forms
        _hold("head0", taps["head0"], ref["head0"], emu["head0"], HR.QUANTUM[p])
    _hold("head3", h3, ref["head3"], emu["head3"], HR.QUANTUM[p])
    if v == 1:                                                          # head0 -> head3 on its own
        with torch.no_grad():
            _hold("head3 of head0", h3, HR.head3_section(sdr, taps["head0"]), HR.head3_emulation(sdr, taps["head0"], p),
                  HR.QUANTUM[p])

    # ---- the output layer, from the tapped head3
    x0 = taps["head_cat2"][:, :HR.STEM] if v == 1 else x
    with torch.no_grad():
        oref = HR.output_section(sdr, h3, x0)
        oemu = HR.output_emulation(sdr, h3, x0, v, p, final)
    _hold("heatmaps", taps["heatmaps"], oref, oemu, HR.Q_F32)
    print(f"  pre-activation > 0 at {100 * frac:.1f} %; {time.time() - t0:.2f} s")
