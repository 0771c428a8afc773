"""CPU: the get_final2 decoder (include/esahrnet.h esahrnet_keypoints_final2).  The host restatement (tests/final2_ref.py)
reproduces the reference's own outputs (tests/golden/final2_*.npz, from tests/golden/make_final2_golden.py), recovers the
centre of rotated anisotropic Gaussians far better than get_final (dxy matters there), and the new entry points are
declared, bound, validated before anything touches a device, and compiled without scratch memory."""
import ctypes as C
import glob
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import final2_ref as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("esahrnet_keypoints_final2_workspace_bytes", "esahrnet_keypoints_final2")
# The reference's outputs come from NumPy 2, where its taylor runs in f32 (NEP 50) and inverts the Hessian with LAPACK; the
# restatement follows NumPy 1.x (f64 after the first product with a Python number, closed-form inverse).  Those two differ by
# the f32 rounding of a handful of intermediate values: ~1e-5 px at worst for these planes, far below 1e-3 px.
REF_TOL = 1e-3


def test_restatement_matches_the_reference_outputs(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "final2_*.npz")))
    names = {os.path.basename(p)[len("final2_"):-4] for p in files}
    assert {"sigma2", "rotated", "nonsquare", "guard", "negative", "constant", "noisy"} <= names
    for p in files:
        d = np.load(p)
        kp, idx, applied = F.decode(d["hm"])
        w = d["hm"].shape[3]
        np.testing.assert_array_equal(np.stack([idx[0] % w, idx[0] // w], -1).astype(np.float32), d["coords"])
        np.testing.assert_allclose(kp[0, :, :2], d["out"], rtol=0, atol=REF_TOL, err_msg=os.path.basename(p))
        if "guard" in p:                            # px = 2 and W-3 (and the same in y) refine, px = 1 and W-2 do not
            assert applied[0].tolist() == [True, True, True, True, False, False]
        if "negative" in p or "constant" in p:      # every blurred value clamps to 1e-10 (det = 0) / the peak is a corner
            assert not applied.any()


def test_get_final2_beats_get_final_on_rotated_gaussians():
    from oracle import keypoints_ref as K
    rng = np.random.default_rng(1)
    e1, e2 = [], []
    for th in np.linspace(0.15, 3.0, 24):
        c = (32 + rng.uniform(-0.5, 0.5), 30 + rng.uniform(-0.5, 0.5))
        hm = F.gaussian_planes(64, 64, [c], 4.0, 1.5, th)[None]
        e1.append(math.hypot(*(K.heatmaps_to_keypoints(hm)[0, 0, :2] - c)))
        e2.append(math.hypot(*(F.decode(hm)[0][0, 0, :2] - c)))
    # measured here: get_final mean 0.27 px (max 0.55), get_final2 mean 1.5e-4 px (max 3.7e-4)
    assert np.mean(e2) < 2e-3 and np.max(e2) < 5e-3
    assert np.mean(e1) > 0.1 and np.mean(e1) > 50 * np.mean(e2)


def test_gauss_weights_in_the_kernel_are_the_formula():
    src = open(os.path.join(ROOT, "esa-pose-estimation_amd", "csrc", "refine.h")).read()
    body = re.search(r"kFinal2Gauss\[11\]\s*=\s*\{(.*?)\}", src, re.S).group(1)
    hexes = [float.fromhex(v.strip()) for v in body.split(",")]
    assert hexes == F.GAUSS
    assert abs(sum(F.GAUSS) - 1) < 1e-15


def test_header_declares_and_lib_exports_the_entries():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esahrnet.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    from esa_pose_estimation_amd import _lib as L
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == L.ABI_VERSION
    assert set(ENTRIES) <= set(L.exported_symbols())
    raw = C.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name


def test_workspace_query_and_argument_checks():
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    b = C.c_size_t()
    L.check(lib.esahrnet_keypoints_final2_workspace_bytes(32, 11, 256, 256, C.byref(b)))
    tiles = 32 * 11 * math.ceil(256 / 32) * math.ceil(256 / 64)
    assert b.value >= tiles * 12 and b.value % 256 == 0 and b.value < 32 * 11 * 256 * 256 * 4 // 100
    assert lib.esahrnet_keypoints_final2_workspace_bytes(0, 11, 256, 256, C.byref(b)) != 0
    assert b"bad shape" in lib.esahrnet_last_error()
    assert lib.esahrnet_keypoints_final2_workspace_bytes(1, 1, 16, 16, None) != 0
    assert lib.esahrnet_keypoints_final2(None, 1, 1, 16, 16, None, None, None, 0, None) != 0
    assert b"null argument" in lib.esahrnet_last_error()


def test_refine_argument_validation():
    from esa_pose_estimation_amd import config, inference, parallel, seg_hrnet2
    from esa_pose_estimation_amd.inference import get_final2  # noqa: F401  (the reference's import line, val.py:20)
    assert inference.check_refine("get_final2") == "get_final2"
    for bad in ("get_final3", None, 2, "GET_FINAL2"):
        with pytest.raises(ValueError):
            inference.heatmaps_to_keypoints(torch.zeros(1, 1, 16, 16), refine=bad)
    with pytest.raises(ValueError):
        parallel.sharded_keypoints(None, torch.zeros(1, 1, 16, 16), refine="nope")
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(16, 32, 64, 128)))
    x = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError):
        net(x, output="keypoints", refine="nope")
    with pytest.raises(ValueError):
        net(x, output="heatmaps", refine="get_final2")


def test_sharded_keypoints_passes_refine_on():
    from esa_pose_estimation_amd import parallel
    seen = []

    class Net:
        num_keypoints = 2

        def __call__(self, x, **kw):
            seen.append(("net", kw))
            return torch.zeros(x.shape[0], 2, 3) if kw else torch.zeros(x.shape[0], 2, 8, 8)

    def fn(heat, **kw):
        seen.append(("fn", kw))
        return torch.zeros(heat.shape[0], 2, 3)

    crops = torch.zeros(3, 1, 8, 8)
    parallel.sharded_keypoints(Net(), crops, keypoints_fn=fn, refine="get_final2")
    parallel.sharded_keypoints(Net(), crops, keypoints_only=True, refine="get_final2")
    parallel.sharded_keypoints(Net(), crops, keypoints_fn=fn)
    assert seen == [("net", {}), ("fn", {"refine": "get_final2"}), ("net", {"output": "keypoints", "refine": "get_final2"}),
                    ("net", {}), ("fn", {})]


def test_new_kernels_use_no_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("esa_build", os.path.join(ROOT, "esa-pose-estimation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    if not os.path.exists(b.USAGE):
        b.build(force=True)
    usage = json.load(open(b.USAGE))
    mine = {k: v for k, v in usage.items() if k.startswith("keypoints_final2.hip:")}
    assert len(mine) == 2
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
