"""The refusals of the entries that share a body (csrc/loader.hip frames_keypoints, csrc/abi_decode.hip keypoints_gaussfit): the
three esahrnet_frames_keypoints* entries and the two stand-alone Gaussian-fit entries, one bad argument at a time and a few
pairs.  Every call must return, byte for byte, the message recorded in tests/golden/refusal_messages.json from the library
built before the bodies were shared (tests/golden/make_refusal_golden.py wrote it): equality with a record, not with a
formula, so a slip in a `who` prefix or in the order of two checks fails.

A case is refused before anything is launched.  The cases up to the check of esahrnet_commit run on an uncommitted handle
with pointers that are only numbers, and need no GPU.  What an entry checks after that — the Gaussian fit's output alignment,
the workspace's size and alignment — is reachable only with a committed handle, which only a GPU gives: those cases are
marked gpu, and pass real device buffers, so that a refusal that went missing would launch on valid memory."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusal_messages.json")
P = 0x10000                                 # host cases: a 256-byte aligned number, never dereferenced
NAN = float("nan")
FRAMES = ("frames_keypoints", "frames_keypoints_gaussfit", "frames_keypoints_gaussfit_cov")
ALONE = ("keypoints_gaussfit", "keypoints_gaussfit_cov")
M, SCALE, FH, FW, K = 1, 64, 96, 128, 11    # the committed cases' loader shape (one crop of 64 x 64 from one 96 x 128 frame)

# name -> (overrides of the good call: value, or ("+", bytes) to misalign a pointer; entries it applies to, None: all of the kind)
GF, COV = FRAMES[1:], FRAMES[2:]
FRAMES_HOST = {
    "null_handle": (dict(h=None), None), "null_frames": (dict(frames=None), None), "null_det_boxes": (dict(det=None), None),
    "null_kp": (dict(kp=None), None), "null_status": (dict(status=None), GF), "null_crop_boxes": (dict(boxes=None), None),
    "null_rates": (dict(rates=None), None), "null_valid": (dict(valid=None), None), "null_ws": (dict(ws=None), None),
    "m_zero": (dict(m=0), None), "frame_h_zero": (dict(fh=0), None), "scale_zero": (dict(scale=0), None),
    "bad_rule": (dict(rule=3), None), "nframes_zero": (dict(nframes=0), None), "bad_pixel_format": (dict(fmt=5), None),
    "stdv_zero": (dict(std=0.0), None), "stdv_nan": (dict(std=NAN), None), "no_frame_index": (dict(m=2), None),
    "uncommitted": (dict(), None),
    "cov_misaligned": (dict(cov=("+", 4)), COV), "info_misaligned": (dict(info=("+", 4)), COV),
    "cov_floor_nan": (dict(floor=NAN), COV), "cov_floor_negative": (dict(floor=-1e-6), COV),
    # pairs: which of two refusals comes first (every host case is also a pair with the uncommitted handle)
    "rule_and_pixel_format": (dict(rule=3, fmt=5), None), "stdv_and_frame_index": (dict(std=0.0, m=2), None),
    "frame_index_and_cov_floor": (dict(m=2, floor=NAN), COV), "kp_misaligned_uncommitted": (dict(kp=("+", 2)), None),
    "null_kp_and_m_zero": (dict(kp=None, m=0), None),
}
FRAMES_COMMITTED = {
    "kp_misaligned": (dict(kp=("+", 2)), GF), "idx_misaligned": (dict(idx=("+", 2)), GF), "status_misaligned": (dict(status=("+", 2)), GF),
    "fit_misaligned": (dict(fit=("+", 4)), GF), "hess_misaligned": (dict(hess=("+", 4)), GF),
    "cov_misaligned_committed": (dict(cov=("+", 4)), COV), "cov_floor_nan_committed": (dict(floor=NAN), COV),
    "bad_decoder": (dict(decoder=7), FRAMES[:1]), "odd_scale": (dict(scale=63), None),
    "ws_too_small": (dict(wsb=0), None), "ws_one_byte_short": (dict(wsb=("need", -1)), None), "ws_misaligned": (dict(ws=("+", 16)), None),
    "ws_small_and_misaligned": (dict(wsb=0, ws=("+", 16)), None), "fit_misaligned_and_ws_small": (dict(fit=("+", 4), wsb=0), GF),
}
ALONE_HOST = {
    "null_heat": (dict(heat=None), None), "null_kp": (dict(kp=None), None), "null_status": (dict(status=None), None),
    "n_zero": (dict(n=0), None), "planes_too_many": (dict(n=65536, k=65536), None), "plane_too_large": (dict(hh=65536, ww=65536), None),
    "heat_misaligned": (dict(heat=("+", 2)), None), "kp_misaligned": (dict(kp=("+", 2)), None),
    "idx_misaligned": (dict(idx=("+", 2)), None), "status_misaligned": (dict(status=("+", 2)), None),
    "fit_misaligned": (dict(fit=("+", 4)), None), "hess_misaligned": (dict(hess=("+", 4)), None),
    "cov_misaligned": (dict(cov=("+", 4)), ALONE[1:]), "info_misaligned": (dict(info=("+", 4)), ALONE[1:]),
    "cov_floor_nan": (dict(floor=NAN), ALONE[1:]),
    "null_kp_and_n_zero": (dict(kp=None, n=0), None), "n_zero_and_kp_misaligned": (dict(n=0, kp=("+", 2)), None),
    "kp_and_fit_misaligned": (dict(kp=("+", 2), fit=("+", 4)), None), "hess_misaligned_and_cov_floor": (dict(hess=("+", 4), floor=NAN), ALONE[1:]),
}


def _cases(table, entries):
    return [(e, name) for name, (_, only) in table.items() for e in (only or entries)]


def _resolve(base, bad, need=0):
    a = dict(base)
    for key, v in bad.items():
        a[key] = a[key] + v[1] if isinstance(v, tuple) and v[0] == "+" else need + v[1] if isinstance(v, tuple) else v
    return a


def refuse_frames(lib, entry, base, bad, need=0):
    """The message `entry` refuses the good call `base` with once `bad` is applied."""
    a = _resolve(base, bad, need)
    head = (a["h"], a["frames"], a["nframes"], a["fh"], a["fw"], a["fmt"], a["det"], None, a["m"], a["scale"], a["rule"], 0.485, a["std"])
    placed = (a["boxes"], a["rates"], a["valid"])
    fitted = (a["kp"], a["idx"], a["fit"], a["status"], a["hess"])
    if entry == "frames_keypoints":
        rc = lib.esahrnet_frames_keypoints(*head, a["decoder"], a["kp"], a["idx"], *placed, a["ws"], a["wsb"], None)
    elif entry == "frames_keypoints_gaussfit":
        rc = lib.esahrnet_frames_keypoints_gaussfit(*head, *fitted, *placed, a["ws"], a["wsb"], None)
    else:
        rc = lib.esahrnet_frames_keypoints_gaussfit_cov(*head, *fitted, *placed, a["cov"], a["info"], a["floor"], a["ws"], a["wsb"], None)
    assert rc != 0, (entry, bad)
    return lib.esahrnet_last_error().decode()


def refuse_alone(lib, entry, bad):
    a = _resolve(dict(heat=P, n=2, k=3, hh=32, ww=40, kp=P, idx=P, fit=P, status=P, hess=P, cov=P, info=P, floor=1e-6), bad)
    args = (a["heat"], a["n"], a["k"], a["hh"], a["ww"], a["kp"], a["idx"], a["fit"], a["status"], a["hess"])
    if entry == "keypoints_gaussfit":
        rc = lib.esahrnet_keypoints_gaussfit(*args, None)
    else:
        rc = lib.esahrnet_keypoints_gaussfit_cov(*args, a["cov"], a["info"], a["floor"], None)
    assert rc != 0, (entry, bad)
    return lib.esahrnet_last_error().decode()


def host_base(h):
    """The good call on pointers that are only numbers (every host case is refused before any of them is read)."""
    return dict(h=h, frames=P, nframes=1, fh=1200, fw=1920, fmt=0, det=P, m=1, scale=256, rule=0, std=0.229, decoder=0, kp=P, idx=P,
                fit=P, status=P, hess=P, boxes=P, rates=P, valid=P, cov=P, info=P, floor=1e-6, ws=P, wsb=1 << 40)


def uncommitted_handle(lib, L):
    from esa_pose_estimation_amd import config, hrnet
    cfg = hrnet._cfg_struct(config.make_config(widths=(16, 32, 64, 128)), 1, K, 0, "fp32")
    h = C.c_void_p()
    L.check(lib.esahrnet_create(C.byref(cfg), 0, C.byref(h)))
    return h


def committed_setup(lib_path=None):
    """-> (lib, base, need): a committed tiny seg_hrnet2 and the good loader call on real, zeroed device buffers (each with
    slack behind it for the misaligned cases); need[entry]: what the entry's workspace query returns.  lib_path: another build
    of the library (the golden maker's)."""
    import torch
    from esa_pose_estimation_amd import _lib as L, config, seg_hrnet2, synth
    net = seg_hrnet2.get_seg_model(config.make_config(widths=(16, 32, 64, 128)), precision="fp32")
    net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0), strict=True)
    if lib_path:
        net._rt.use_library(L.load_other(lib_path))
    net = net.cuda().eval()
    lib, dev = net._rt.lib, torch.device("cuda", torch.cuda.current_device())
    h = net._rt._handle_for(net, dev)
    need, nb = {}, C.c_size_t()
    L.check(lib.esahrnet_frames_keypoints_workspace_bytes(h, M, SCALE, 0, C.byref(nb)))
    need["frames_keypoints"] = nb.value
    L.check(lib.esahrnet_frames_keypoints_gaussfit_workspace_bytes(h, M, SCALE, C.byref(nb)))
    need["frames_keypoints_gaussfit"] = need["frames_keypoints_gaussfit_cov"] = nb.value
    sizes = dict(frames=FH * FW, det=M * 16, kp=M * K * 12, idx=M * K * 4, fit=M * K * 64, status=M * K * 4, hess=M * K * 24,
                 boxes=M * 16, rates=M * 8, valid=M * 4, cov=M * K * 24, info=M * K * 24, ws=max(need.values()))
    arena = torch.zeros(sum((b + 511) // 256 * 256 for b in sizes.values()) + 256, dtype=torch.uint8, device=dev)
    base, at = dict(h=h, nframes=1, fh=FH, fw=FW, fmt=0, m=M, scale=SCALE, rule=0, std=0.229, decoder=0, floor=1e-6), \
        arena.data_ptr() + (-arena.data_ptr()) % 256
    for name, b in sizes.items():
        base[name] = at
        at += (b + 511) // 256 * 256
    torch.cuda.synchronize()
    return lib, base, need, (net, arena)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def host():
    from esa_pose_estimation_amd import _lib as L
    lib = L.lib()
    h = uncommitted_handle(lib, L)
    yield lib, host_base(h)
    lib.esahrnet_destroy(h)


@pytest.fixture(scope="module")
def committed():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    return committed_setup()


@pytest.mark.parametrize("entry,case", _cases(FRAMES_HOST, FRAMES))
def test_frames_entries_refuse_with_the_recorded_message(host, golden, entry, case):
    lib, base = host
    assert refuse_frames(lib, entry, base, FRAMES_HOST[case][0]) == golden[f"{entry}/{case}"]


@pytest.mark.parametrize("entry,case", _cases(ALONE_HOST, ALONE))
def test_stand_alone_gaussfit_entries_refuse_with_the_recorded_message(golden, entry, case):
    from esa_pose_estimation_amd import _lib as L
    assert refuse_alone(L.lib(), entry, ALONE_HOST[case][0]) == golden[f"{entry}/{case}"]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,case", _cases(FRAMES_COMMITTED, FRAMES))
def test_frames_entries_refuse_behind_the_commit_with_the_recorded_message(committed, golden, entry, case):
    lib, base, need, _ = committed
    base = dict(base, wsb=need[entry])
    assert refuse_frames(lib, entry, base, FRAMES_COMMITTED[case][0], need[entry]) == golden[f"{entry}/{case}"]


def test_the_record_holds_exactly_these_cases(golden):
    want = {f"{e}/{c}" for table, ents in ((FRAMES_HOST, FRAMES), (FRAMES_COMMITTED, FRAMES), (ALONE_HOST, ALONE))
            for e, c in _cases(table, ents)}
    assert set(golden) == want
