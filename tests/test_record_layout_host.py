"""The one description of the packed records (inference.record_fields / record_views / packed_layout / pack_correspondences) and
the refusals around it, against a record: tests/golden/record_layouts.json holds what the commit BEFORE the description was
made one returned — every layout dict (key order included), every field tuple, the offsets of pack_correspondences' views — and
the text every ValueError was raised with before the net is touched (tests/golden/make_record_layouts_golden.py wrote it by
running `recorded` below on that commit).  Equality with a record, not with a formula.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from esa_pose_estimation_amd import inference, pipeline

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_layouts.json")
SHAPES = [(m, k) for m in (1, 3, 32) for k in (1, 11, 30, 32)]
# every form packed_layout accepts: name -> (gaussfit, cov, candidates)
FORMS = {"plain": (False, False, None), "gaussfit": (True, False, None), "gaussfit+cov": (True, True, None),
         **{f"candidates={M}": (False, False, M) for M in (1, 2, 3, 4)}}
KINDS = {"keypoints/plain": ("keypoints", False, False), "keypoints/gaussfit": ("keypoints", True, False),
         "keypoints/gaussfit+cov": ("keypoints", True, True), "correspondences": ("correspondences", False, False)}
NAN = float("nan")


def _poses(**kw):
    """estimate_poses on nothing: the net, the frames and the boxes are None, so a case must be refused before it reads them."""
    return lambda inf, pipe: pipe.estimate_poses(None, None, None, None, None, **kw)


# name -> the call that must raise ValueError; a name with "+" makes two checks fire, so the record pins which comes first
REFUSALS = {
    "packed_layout/cov_without_gaussfit": lambda inf, pipe: inf.packed_layout(2, 11, False, True),
    "packed_layout/candidates_with_gaussfit": lambda inf, pipe: inf.packed_layout(2, 11, True, candidates=2),
    "packed_layout/candidates_0": lambda inf, pipe: inf.packed_layout(2, 11, candidates=0),
    "packed_layout/candidates_5": lambda inf, pipe: inf.packed_layout(2, 11, candidates=5),
    "packed_layout/cov_without_gaussfit+candidates_0": lambda inf, pipe: inf.packed_layout(2, 11, False, True, candidates=0),
    "packed_layout/candidates_with_gaussfit+candidates_9": lambda inf, pipe: inf.packed_layout(2, 11, True, True, candidates=9),
    "record_fields/unknown_kind": lambda inf, pipe: inf.record_fields(11, "poses"),
    "record_fields/k_0": lambda inf, pipe: inf.record_fields(0, "keypoints"),
    "record_fields/k_negative": lambda inf, pipe: inf.record_fields(-3, "correspondences"),
    "record_fields/correspondences_gaussfit": lambda inf, pipe: inf.record_fields(11, "correspondences", gaussfit=True),
    "record_fields/correspondences_cov": lambda inf, pipe: inf.record_fields(11, "correspondences", cov=True),
    "record_fields/cov_without_gaussfit": lambda inf, pipe: inf.record_fields(11, "keypoints", False, True),
    "record_fields/unknown_kind+k_0": lambda inf, pipe: inf.record_fields(0, "poses"),
    "record_fields/k_0+correspondences_gaussfit": lambda inf, pipe: inf.record_fields(0, "correspondences", True),
    "record_fields/k_0+cov_without_gaussfit": lambda inf, pipe: inf.record_fields(0, "keypoints", False, True),
    "check_weights/unknown": lambda inf, pipe: inf.check_weights("variance"),
    "check_weights/no_string": lambda inf, pipe: inf.check_weights(None),
    "check_weights/hessian_get_final": lambda inf, pipe: inf.check_weights("hessian", "get_final"),
    "check_weights/covariance_get_final2": lambda inf, pipe: inf.check_weights("covariance", "get_final2"),
    "check_weights/covariance_get_final": lambda inf, pipe: inf.check_weights("covariance", "get_final"),
    "check_weights/unknown+get_final": lambda inf, pipe: inf.check_weights("Hessian", "get_final"),
    "check_refine/unknown": lambda inf, pipe: inf.check_refine("get_final3"),
    "check_refine/none": lambda inf, pipe: inf.check_refine(None),
    "check_refine/number": lambda inf, pipe: inf.check_refine(2),
    "check_cov_floor/string": lambda inf, pipe: inf.check_cov_floor("tiny"),
    "check_cov_floor/none": lambda inf, pipe: inf.check_cov_floor(None),
    "check_cov_floor/negative": lambda inf, pipe: inf.check_cov_floor(-1e-6),
    "check_cov_floor/nan": lambda inf, pipe: inf.check_cov_floor(NAN),
    "estimate_poses/unknown_refine": _poses(refine="taylor"),
    "estimate_poses/unknown_weights": _poses(weights="variance"),
    "estimate_poses/hessian_get_final": _poses(weights="hessian", device_select=True),
    "estimate_poses/unknown_candidates_path": _poses(candidates_path="device"),
    "estimate_poses/candidates_path_without_candidates": _poses(candidates_path="fused"),
    "estimate_poses/candidates_path_loader_without_candidates": _poses(candidates_path="loader"),
    "estimate_poses/candidates+keypoints_only": _poses(candidates=3, keypoints_only=True),
    "estimate_poses/candidates+device_loader": _poses(candidates=3, device_loader=True),
    "estimate_poses/candidates+device_select": _poses(candidates=3, device_select=True),
    "estimate_poses/candidates+distributed": _poses(candidates=3, distributed=True),
    "estimate_poses/candidates+native_false": _poses(candidates=3, native=False),
    "estimate_poses/candidates+refine": _poses(candidates=3, refine="get_final2"),
    "estimate_poses/report_native_false": _poses(return_report=True, native=False),
    "estimate_poses/max_rms_px_native_false": _poses(max_rms_px=2.0, native=False),
    "estimate_poses/min_inliers_native_false": _poses(min_inliers=6, native=False),
    "estimate_poses/weights_without_device_select": _poses(weights="hessian", refine="get_final2"),
    "estimate_poses/covariance_without_device_select": _poses(weights="covariance", refine="gaussfit", device_loader=True),
    "estimate_poses/device_select_native_false": _poses(device_select=True, native=False),
    "estimate_poses/frame_idx_without_loader": _poses(frame_idx=[0, 0]),
    "estimate_poses/rule_without_loader": _poses(rule="train"),
    "estimate_poses/frame_idx_without_loader_candidates_fused": _poses(frame_idx=[0], candidates=2, candidates_path="fused"),
    # two checks fire: which one speaks
    "estimate_poses/unknown_refine+unknown_weights": _poses(refine="taylor", weights="variance"),
    "estimate_poses/unknown_weights+unknown_candidates_path": _poses(weights="variance", candidates_path="device"),
    "estimate_poses/unknown_candidates_path+candidates+keypoints_only": _poses(candidates_path="device", candidates=3, keypoints_only=True),
    "estimate_poses/candidates+keypoints_only+device_loader": _poses(candidates=3, keypoints_only=True, device_loader=True),
    "estimate_poses/candidates+native_false+report": _poses(candidates=3, native=False, return_report=True),
    "estimate_poses/report_native_false+weights_without_device_select": _poses(return_report=True, native=False, weights="hessian",
                                                                               refine="get_final2"),
    "estimate_poses/weights_without_device_select+frame_idx": _poses(weights="hessian", refine="get_final2", frame_idx=[0]),
    "estimate_poses/device_select_native_false+frame_idx": _poses(device_select=True, native=False, rule="train"),
}


def _text(inf, e):
    # record_fields names its kinds in its refusal, and the kinds are allowed to grow: the record keeps the rest of that text
    return str(e).replace(repr(tuple(inf.RECORD_KINDS)), "<RECORD_KINDS>")


def recorded(inf, pipe):
    """Everything the record holds, from the two modules given (the golden's maker passes another commit's)."""
    rec = {"packed_layout": {}, "record_fields": {}, "pack_correspondences": {}, "refusals": {}}
    for m, k in SHAPES:
        # lists of [name, [offset, bytes]], not dicts: the order of the keys is part of the record
        rec["packed_layout"][f"{m}x{k}"] = {form: [[n, list(v)] for n, v in inf.packed_layout(m, k, g, c, cand).items()]
                                            for form, (g, c, cand) in FORMS.items()}
        count, order, pts, w, packed = inf.pack_correspondences(m, k, "cpu")
        rec["pack_correspondences"][f"{m}x{k}"] = {"total": packed.numel(), **{
            n: t.data_ptr() - packed.data_ptr() for n, t in (("count", count), ("order", order), ("pts", pts), ("w", w))}}
    for k in sorted({k for _, k in SHAPES}):
        rec["record_fields"][str(k)] = {name: [list(f) for f in inf.record_fields(k, kind, g, c)] for name, (kind, g, c) in KINDS.items()}
    for name, call in REFUSALS.items():
        try:
            call(inf, pipe)
        except ValueError as e:
            rec["refusals"][name] = _text(inf, e)
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now():
    return recorded(inference, pipeline)


@pytest.mark.parametrize("part", ["packed_layout", "record_fields", "pack_correspondences"])
def test_layouts_are_the_recorded_ones(golden, now, part):
    assert set(now[part]) == set(golden[part])
    for key, want in golden[part].items():
        assert now[part][key] == want, (part, key)              # == on lists: names, order, offsets and sizes at once


def test_the_record_holds_every_shape_form_and_case(golden):
    assert set(golden["packed_layout"]) == set(golden["pack_correspondences"]) == {f"{m}x{k}" for m, k in SHAPES}
    assert all(set(v) == set(FORMS) for v in golden["packed_layout"].values())
    assert all(set(v) == set(KINDS) for v in golden["record_fields"].values())
    assert set(golden["refusals"]) == set(REFUSALS)


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_with_the_recorded_text(golden, case):
    with pytest.raises(ValueError) as e:
        REFUSALS[case](inference, pipeline)
    assert _text(inference, e.value) == golden["refusals"][case]


# ---- the candidates kind is new with the one table: held to the recorded layout (the numpy views: tests/test_records_host.py) ----
@pytest.mark.parametrize("m,k", SHAPES)
def test_candidates_kind_rebuilds_the_recorded_layout(golden, m, k):
    assert "candidates" in inference.RECORD_KINDS
    for M in (1, 2, 3, 4):
        fields = inference.record_fields(k, "candidates", candidates=M)
        off, want = 0, []
        for name, b in fields:
            want.append([name, [off, m * b]])
            off += m * b
        assert want + [["total", [0, off]]] == golden["packed_layout"][f"{m}x{k}"][f"candidates={M}"]
        v = inference.record_views(torch.zeros(off, dtype=torch.uint8), m, k, fields)
        assert v["cand"].shape == (m, k, M, 3) and v["cand"].dtype == torch.float32
        assert v["cidx"].shape == (m, k, M) and v["cidx"].dtype == torch.int32
    for bad in (None, 0, 5):
        with pytest.raises(ValueError, match="candidates"):
            inference.record_fields(k, "candidates", candidates=bad)
    with pytest.raises(ValueError, match="candidates"):
        inference.record_fields(k, "keypoints", candidates=2)


@pytest.mark.parametrize("m,k", SHAPES)
def test_unpack_correspondences_gives_the_numpy_views(golden, m, k):
    want = golden["pack_correspondences"][f"{m}x{k}"]
    host = (np.arange(want["total"]) % 251).astype(np.uint8)
    shapes = {"count": (m,), "order": (m, k), "pts": (m, k, 2), "w": (m, k, 3)}
    for n, x in zip(("count", "order", "pts", "w"), inference.unpack_correspondences(host, m, k)):
        assert x.ctypes.data - host.ctypes.data == want[n] and x.shape == shapes[n] and np.shares_memory(x, host), n
        assert x.dtype == (np.int32 if n in ("count", "order") else np.float64), n


def test_packed_layout_refuses_k_below_1():
    """New with the one table: packed_layout works from record_fields, so it refuses what record_fields refuses (before, it gave
    a dict of empty fields for k = 0)."""
    for kw in ({}, {"candidates": 2}, {"gaussfit": True}):
        with pytest.raises(ValueError, match="k = 0: a record has at least one keypoint per crop"):
            inference.packed_layout(3, 0, **kw)


def test_loader_calls_refuse_a_bad_refine_first(golden):
    """The loader's request (inference.LoaderRequest, which net._loader takes) and the public calls that build it refuse
    refine=None and an unknown refine by name, with the recorded text of check_refine, before they look at weights, cov_floor or
    the frames (all bad here: CPU frames, unknown weights, a NaN floor)."""
    from esa_pose_estimation_amd import config, seg_hrnet2
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(8, 16, 32, 64))).eval()
    frames, boxes = torch.zeros(1, 64, 64, dtype=torch.uint8), [[0, 0, 9, 9]]
    for refine, case in ((None, "check_refine/none"), ("get_final3", "check_refine/unknown")):
        rest = (frames, boxes, None, 64, "val", None, 0.229, None)
        calls = (lambda: net._loader(inference.LoaderRequest(refine, None, NAN), *rest),
                 lambda: net._loader(inference.LoaderRequest(refine, None, NAN, (0.8, 24, "variance")), *rest),
                 lambda: net.frames_to_keypoints(frames, boxes, refine=refine),
                 lambda: net.frames_to_correspondences(frames, boxes, refine=refine, weights="variance", cov_floor=NAN))
        for call in calls:
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == golden["refusals"][case]
    # and behind a good refine: the weights, then the floor, then the loader's arguments
    with pytest.raises(ValueError) as e:
        net.frames_to_correspondences(frames, boxes, refine="gaussfit", weights="variance", cov_floor=NAN)
    assert str(e.value) == golden["refusals"]["check_weights/unknown"]
    with pytest.raises(ValueError) as e:
        net.frames_to_correspondences(frames, boxes, refine="gaussfit", weights="covariance", cov_floor=NAN)
    assert str(e.value) == golden["refusals"]["check_cov_floor/nan"]
    net.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        net.frames_to_keypoints(frames, boxes, refine=None)                         # the eval check comes before everything
