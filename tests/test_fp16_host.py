"""The single-pass fp16 mode (esahrnet_cfg.precision = 3, precision="fp16") without a GPU: the Python mapping, the header,
what esahrnet_create takes and refuses, the host packer's rounding, the commit-time refusal of weights fp16 cannot hold, and
the CPU emulation's figures that the GPU bounds of tests/test_gpu_fp16.py are multiples of."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fp16_emu  # noqa: E402

W32 = (32, 64, 128, 256)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


def _lib():
    import torch  # noqa: F401  (first: the library shares torch's HIP runtime)
    from esa_pose_estimation_amd import _lib as L
    return L.lib(), L


def _cfg(variant, precision, widths=W32, cin=1, k=11):
    from esa_pose_estimation_amd import _lib as L
    s = L.Cfg()
    s.cin, s.num_keypoints, s.stem_width, s.variant, s.precision, s.final_conv_kernel = cin, k, 64, variant, precision, 1
    for i, (mods, blocks) in enumerate([(1, (2,)), (1, (2, 2)), (1, (2, 2, 2)), (1, (4, 4, 4, 4))]):
        s.modules[i] = mods
        for b, nb in enumerate(blocks):
            s.blocks[i][b] = nb
    for b, w in enumerate(widths):
        s.widths[b] = w
    return s


def test_python_mapping_carries_precision_3():
    """Fails without the feature: "fp16" is not a key of PRECISIONS and _cfg_struct raises ValueError."""
    from esa_pose_estimation_amd import config, hrnet, seg_hrnet, seg_hrnet2
    assert hrnet.PRECISIONS["fp16"] == 3 and hrnet.PRECISIONS[3] == 3
    assert hrnet._cfg_struct(config.make_config(widths=W32), 1, 11, 0, "fp16").precision == 3
    for mod, w in ((seg_hrnet2, W32), (seg_hrnet2, (48, 96, 192, 384)), (seg_hrnet, W32)):
        net = mod.get_seg_model(config.make_config(widths=w), precision="fp16")
        assert net._cfg_struct.precision == 3 and net._cfg_struct.variant == 0
    # defaults unchanged
    assert seg_hrnet2.get_seg_model(config.make_config(widths=W32))._cfg_struct.precision == 2
    assert {k: v for k, v in hrnet.PRECISIONS.items() if k not in ("fp16", 3)} == \
        {"fp32": 2, "bf16x6": 2, "bf16x3": 0, "split-bf16": 0, "bf16": 1, 0: 0, 1: 1, 2: 2}


def test_seg_hrnet3_refuses_fp16_with_the_librarys_message():
    from esa_pose_estimation_amd import _lib as L, config, seg_hrnet3
    with pytest.raises(L.EsaHrnetError, match="seg_hrnet3"):
        seg_hrnet3.get_seg_model(config.make_config(widths=W32), precision="fp16")


def test_header_documents_precision_3_and_abi_stays_6():
    lib, _ = _lib()
    text = open(os.path.join(ROOT, "include", "esahrnet.h")).read()
    assert re.search(r"#define\s+ESAHRNET_ABI_VERSION\s+6\b", text)
    assert lib.esahrnet_abi_version() == 6
    field = text[text.index("int32_t precision;"):text.index("} esahrnet_cfg;")]
    assert re.search(r'\b3: "fp16"', field) and "65504" in field and "variant 0 only" in field
    assert "3: fp16" in text[text.index("int esahrnet_op_conv_ex(") - 400:text.index("int esahrnet_op_conv_ex(")]


def test_create_takes_variant_0_and_refuses_variant_1_and_precision_4():
    lib, L = _lib()
    h = C.c_void_p()
    assert lib.esahrnet_create(C.byref(_cfg(0, 3)), 0, C.byref(h)) == 0, lib.esahrnet_last_error()
    hb = C.c_void_p()
    assert lib.esahrnet_create(C.byref(_cfg(0, 1)), 0, C.byref(hb)) == 0
    assert lib.esahrnet_launch_count(h) == lib.esahrnet_launch_count(hb)          # the bf16 mode's plan, op for op
    ws, wsb = C.c_size_t(), C.c_size_t()
    for n, hh, ww in ((1, 64, 64), (32, 256, 256), (3, 80, 112)):
        assert lib.esahrnet_workspace_bytes(h, n, hh, ww, C.byref(ws)) == 0
        assert lib.esahrnet_workspace_bytes(hb, n, hh, ww, C.byref(wsb)) == 0
        assert ws.value == wsb.value and ws.value > 0
    lib.esahrnet_destroy(h)
    lib.esahrnet_destroy(hb)
    h = C.c_void_p()
    assert lib.esahrnet_create(C.byref(_cfg(1, 3, k=30)), 0, C.byref(h)) != 0
    msg = lib.esahrnet_last_error().decode()
    assert "seg_hrnet3" in msg and "fp16" in msg, msg
    assert lib.esahrnet_create(C.byref(_cfg(0, 4)), 0, C.byref(h)) != 0
    assert "0..3" in lib.esahrnet_last_error().decode()
    assert lib.esahrnet_create(C.byref(_cfg(0, -1)), 0, C.byref(h)) != 0


def test_create_refuses_fp16_without_the_matrix_core_output_layer(monkeypatch):
    lib, _ = _lib()
    monkeypatch.setenv("ESAHRNET_FINAL_VALU", "1")
    h = C.c_void_p()
    assert lib.esahrnet_create(C.byref(_cfg(0, 3)), 0, C.byref(h)) != 0
    assert "ESAHRNET_FINAL_VALU" in lib.esahrnet_last_error().decode()
    assert lib.esahrnet_create(C.byref(_cfg(0, 1)), 0, C.byref(h)) == 0            # the bf16 mode still takes the switch
    lib.esahrnet_destroy(h)


def test_op_descs_tell_fp16_from_bf16():
    """The plan of the fp16 mode names the fp16 instantiations, launch for launch where the bf16 plan names the bf16 ones."""
    lib, L = _lib()
    rows = {}
    for prec in (1, 3):
        h = C.c_void_p()
        assert lib.esahrnet_create(C.byref(_cfg(0, prec)), 0, C.byref(h)) == 0
        out = []
        for i in range(lib.esahrnet_launch_count(h)):
            d = L.OpDesc()
            assert lib.esahrnet_op_desc_get(h, i, 2, 128, 128, C.byref(d)) == 0, lib.esahrnet_last_error()
            out.append((d.kernel.decode(), d.label.decode(), d.flops, d.bytes))
        rows[prec] = out
        lib.esahrnet_destroy(h)
    assert len(rows[1]) == len(rows[3])
    renamed = 0
    for (kb, lb, fb, bb), (kh, lh, fh, bh) in zip(rows[1], rows[3]):
        assert (lb, fb, bb) == (lh, fh, bh)                        # same op, same work, same bytes
        assert bool(kb) == bool(kh)
        if not kb:
            continue
        assert "fp16" in kh and "fp16" not in kb, (kb, kh)
        assert kh.replace("<fp16>", "").replace(", fp16>", ", true>") == kb or kh.replace("<fp16>", "<bf16>") == kb, (kb, kh)
        renamed += 1
    kernels = {r[0] for r in rows[3]}
    assert {"conv_s2c32_kernel<1, 8, 4, false, fp16>", "conv1x1_kernel<fp16>", "head_fused_bf<fp16>", "stem_kernel<fp16>",
            "fuse_kernel<fp16>", "final_kernel<fp16>"} <= kernels, sorted(kernels)
    assert renamed >= 40


# ---- the host packer (esa::pack_conv_weights_bf with half = true: an internal C++ function of the library, reached by its
# mangled name — the C ABI gains no symbol for this mode) ---------------------------------------------------------------
def _pack_hf(w, coutp, cinp):
    lib, _ = _lib()
    fn = getattr(lib, "_ZN3esa20pack_conv_weights_bfEPKfiiiiiPvb")
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_bool]
    cout, cin, k, _ = w.shape
    dst = np.full((coutp // 16) * (cinp // 64) * k * k * 1024, 0xFFFF, dtype=np.uint16)
    w = np.ascontiguousarray(w, dtype=np.float32)
    fn(w.ctypes.data, cout, cin, k, coutp, cinp, dst.ctypes.data, True)
    return dst.reshape(coutp // 16, cinp // 64, k * k, 2, 64, 8)


def test_host_packer_rounds_to_nearest_even_keeps_subnormals_and_fragment_order():
    rng = np.random.default_rng(5)
    cout, cin, k = 20, 70, 3
    w = (rng.standard_normal((cout, cin, k, k)) * np.exp(rng.uniform(-18, 8, (cout, cin, k, k)))).astype(np.float32)
    flat = w.reshape(-1)
    flat[0] = 1.0 + 2.0 ** -11            # tie between 1 and 1 + 2^-10: to even -> 1
    flat[1] = 1.0 + 3 * 2.0 ** -11        # tie between 1 + 2^-10 and 1 + 2^-9: to even -> 1 + 2^-9
    flat[2] = 2.0 ** -24                  # the smallest subnormal half, exactly
    flat[3] = 1.5 * 2.0 ** -24            # tie between subnormals 1 and 2 -> 2
    flat[4] = 2.0 ** -25                  # tie between 0 and the smallest subnormal -> 0
    flat[5] = -3.3e-6                     # a subnormal half after rounding
    flat[6] = 65504.0
    flat[7] = -65519.0                    # rounds to -65504 (65520 would be inf)
    flat[8] = 2.0 ** -14 - 2.0 ** -26     # rounds up into the normal range
    p = _pack_hf(w, 32, 128)
    ref = w.astype(np.float16)            # NumPy rounds to nearest even and keeps subnormals
    assert ref.reshape(-1)[0] == np.float16(1.0) and ref.reshape(-1)[1] == np.float16(1.0 + 2.0 ** -9)
    assert ref.reshape(-1)[2].view(np.uint16) == 1 and ref.reshape(-1)[3].view(np.uint16) == 2 and ref.reshape(-1)[4] == 0
    assert 0 < abs(float(ref.reshape(-1)[5])) < 2.0 ** -14
    assert np.isfinite(ref).all()
    seen = 0
    for t16 in range(2):
        for blk in range(2):
            for tap in range(9):
                for step in range(2):
                    for lane in range(64):
                        for j in range(8):
                            co, ci = t16 * 16 + (lane & 15), blk * 64 + step * 32 + 8 * (lane >> 4) + j
                            want = ref[co, ci, tap // 3, tap % 3].view(np.uint16) if co < cout and ci < cin else 0
                            assert p[t16, blk, tap, step, lane, j] == want, (co, ci, tap)
                            seen += co < cout and ci < cin
    assert seen == w.size


def test_fp16_splits_exactly_into_hi_plus_lo_bf16():
    """What the output layer relies on when a tap weight is 1: every finite half is hi + lo with hi = bf16(v), lo = bf16(v - hi)
    (11 significand bits fit in 8 + 8), subnormals included."""
    import torch
    bits = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.float16).float()
    v = v[torch.isfinite(v)]
    hi = v.to(torch.bfloat16).float()
    lo = (v - hi).to(torch.bfloat16).float()
    assert v.numel() == 2 * (31 * 1024) and torch.equal(hi + lo, v)


def _committable(precision, poison=None):
    """A handle with every weight set (He-like synthetic state dict); poison = (conv name, value) overwrites one weight."""
    lib, L = _lib()
    from esa_pose_estimation_amd import config, seg_hrnet2, synth
    from esa_pose_estimation_amd.fold import fold_conv
    net = seg_hrnet2.get_seg_model(config.make_config(widths=W32), precision=precision)
    sd = synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0)
    h = C.c_void_p()
    assert lib.esahrnet_create(C.byref(net._cfg_struct), 0, C.byref(h)) == 0
    for i, d in enumerate(net._descs):
        w, b = fold_conv(sd, d["name"], d["bn"], d["has_bias"])
        if poison and d["name"] == poison[0]:
            w = w.copy()
            w.reshape(-1)[7] = poison[1]
        assert lib.esahrnet_set_conv(h, i, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)) == 0
    return lib, h


@pytest.mark.parametrize("name,value", [("stage3.0.branches.1.0.conv2", 65520.0), ("last_layer.3", -7.0e4),
                                        ("stage2.0.fuse_layers.0.1.0", 1.0e30)])
def test_commit_refuses_a_weight_fp16_cannot_hold(name, value):
    lib, h = _committable("fp16", (name, value))
    assert lib.esahrnet_commit(h) != 0
    msg = lib.esahrnet_last_error().decode()
    assert f"'{name}'" in msg and "fp16" in msg, msg
    lib.esahrnet_destroy(h)


def test_commit_weight_check_is_fp16_only_and_spares_f32_layers():
    # 65519 still rounds to 65504: accepted (the commit then stops at the missing GPU, or succeeds where there is one)
    for prec, poison in (("fp16", ("layer1.0.conv1", 65519.0)), ("fp16", ("conv1", 1.0e6)), ("fp16", ("output_layer.0", 1.0e6)),
                         ("bf16", ("layer1.0.conv1", 1.0e6))):
        lib, h = _committable(prec, poison)
        rc = lib.esahrnet_commit(h)
        assert rc == 0 or "not finite in fp16" not in lib.esahrnet_last_error().decode(), (prec, poison)
        lib.esahrnet_destroy(h)


@pytest.mark.parametrize("tag", ["tiny_hrnet2_64", "w32_hrnet2_128"])
def test_emulation_constants(golden_dir, tag):
    """The figures the GPU bounds are 3 x of (tests/test_gpu_fp16.py) are what the emulation gives here."""
    import torch
    from esa_pose_estimation_amd import synth
    from oracle import hrnet_ref
    g = np.load(os.path.join(golden_dir, tag + ".npz"), allow_pickle=False)
    *_, sd, x, cfg = fp16_emu.golden_case(g, synth, hrnet_ref)
    y = fp16_emu.forward(sd, cfg, x).numpy()
    s = int(g["subsample"])
    d = np.abs(y[:, :, ::s, ::s] - g["out"])
    print(f"{tag}: fp16 emulation vs fp32 reference L_inf {d.max():.4e} mean-abs {d.mean():.4e}")
    assert abs(d.max() - fp16_emu.EMU_LINF[tag]) <= 0.01 * fp16_emu.EMU_LINF[tag]
    assert abs(d.mean() - fp16_emu.EMU_MEAN[tag]) <= 0.01 * fp16_emu.EMU_MEAN[tag]
    flips = (y.reshape(*y.shape[:2], -1).argmax(-1) != g["plane_argmax"]).sum()
    assert flips == 0


def test_emulation_rounding_saturates_and_keeps_subnormals():
    import torch
    t = torch.tensor([1e9, -1e9, 65519.0, 65520.0, 2.0 ** -24, 1.0 + 2.0 ** -11, float("inf")])
    assert fp16_emu.q16(t).tolist() == [65504.0, -65504.0, 65504.0, 65504.0, 2.0 ** -24, 1.0, 65504.0]
