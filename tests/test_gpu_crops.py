"""The crop kernels held to an independent float64 reference, class by class: crop_kernel (csrc/crops.hip, through
esahrnet_crops) and crop_ex_kernel<0|1> (csrc/frontend.hip, through esahrnet_crops_ex).  References, the bound and the case
tables: tests/crops_ref.py; what holds those, and the derivation of the bound: tests/test_crops_ref_host.py.

Every served crop, through both entries, into outputs prefilled with NaN:
  1. |recover_u8(out) - exact| <= B.  exact() is the loader's rule in float64 (slice, the reference's swapped edge pad, bilinear
     interpolation with half-pixel centres), written from the loader and not from the kernel; B = 1.19458 gray levels is derived
     from the 8-bit fixed-point arithmetic alone.  The independent rule.
  2. the output's bits equal normalise(oracle/crops_ref.resize_u8_linear): the existing rule, at the new classes.
  3. no NaN is left: every element was written.
and crop_kernel and crop_ex_kernel<0> agree bit for bit.  Classes (crops_ref.CASES): ratio (source side 1, 2, 3, S-1, S, S+1, 2S,
a 4.3x and a 270x downscale), blocks (S = 8 .. 513: blockIdx.y 0, 1, 2 of crop_ex_kernel), nonsquare (both ways, 1-pixel boxes),
position (edges, corners, whole frame, interior of two odd frames with FH != FW), workload (1920x1200 at 256), normalisation
(three (mean, std) on all 256 levels).  Launches of several crops (crops_ref.BATCHES): the same box alone, first, middle and last
of 7 has the same bits; a permuted and repeated frame index; crop_ex_kernel<1> on RGB frames equals crop_ex_kernel<0> on
luma(rgb) bit for bit.  Crops esahrnet_crops_ex must not serve (crops_ref.NOT_SERVED: valid == 0, a frame index of -1 or nframes,
empty, reversed and off-frame boxes, INT32_MIN / INT32_MAX corners) are +0.0 in every bit, the other crops of the launch keep
the bits they have alone, and the call returns 0.  esahrnet_frames_keypoints at scale 258, the smallest above 256 the network
serves (even sides), is bit-identical to crop_batch followed by the forward.
Every case prints its figures (run with -s); the module prints the case count, its time and the worst |u8 - exact| per class.

Measured on an MI355X: 201 served crops in 160 launches (87 tests), 0.7 s of case time, 3.2 s for the module.  The derived bound
is B = 1.19458; the worst |u8 - exact| per class, the same figure from both kernels in every row: blocks 0.802 (a 40-pixel
source at S = 513), nonsquare 0.791 (40x25 at S = 257), batching 0.772, the served crops of the not-served launches 0.757,
workload 0.747, position 0.746, ratio 0.742 (0.56 and 0.74 on the wide frame's rows, whose source coordinates pass 2048), normalisation 0 (the
identity).  Every bit-equality held at the first run: the restatement at every class, crop_kernel against crop_ex_kernel<0>,
RGB against luma, a crop against its batch, the one call at 258 against its parts.  No defect found in either kernel.

Teeth, each mutation checked once on a scratch build (none widens an index range), this module and the rest of the GPU suite
(2816 tests) run against it:
  1. crop_ex_kernel's column without the `blockIdx.y * 256` term: the 6 single rows with S > 256 and test_batch[rgb-S257] fail
     on leftover NaN (257, 49152 and 131841 elements at S = 257, 384, 513: the columns from 256 on), and the one call at 258 no
     longer equals its parts; every row with S <= 256 passes.  No existing test noticed: none had a scale above 256.
  2. `min(c, xs - 1)` as `min(c, ys - 1)` in px of both kernels: the rows with xs > ys fail, at assertion 1 (the single rows
     40x25, 30x1, 41x40, the two wide-frame rows, the whole landscape frame and the workload row, and the batches that hold such a
     box; test_not_served...[valid0-first] is where the launches' served crops are first held), 17 tests.  Every square row and
     every row with xs < ys passes, as it must: there a column is never past ys - 1.  Of the existing tests one noticed,
     test_crops_pipeline.py::test_gpu_crops_bit_exact_vs_oracle (its full-frame box).
  3. The `- 0.5` dropped from coef in both kernels AND in a scratch copy of oracle/crops_ref.py: 66 tests fail, every one at
     assertion 1 (|u8 - exact| 71 .. 176 levels) with the restatement's bits still equal; what passes is the 1x1 sources, the
     not-served rows' zeros and the tests that compare the kernels with each other.  test_gpu_crops_bit_exact_vs_oracle and all of
     test_gpu_frontend.py pass: this is the misreading the restatement shares.  Two existing tests noticed, both through the
     poses of rendered scenes (test_gpu_refine_at.py::test_candidate_poses_with_get_final_and_peak_weights_is_estimate_poses,
     test_gpu_candidates_forward.py::test_estimate_poses_on_the_fused_path_and_behind_the_loader).
  4. `rintf` as truncation in coef of both kernels: assertion 2 catches it (14 tests: every row at S = 24, 255, 257, 384, 513),
     assertion 1 does not (the worst |u8 - exact| grows to 0.960, inside B).  At a power-of-two S the coefficients are exact
     multiples of 2^-11 and nothing moves, which is why no existing test noticed: their scales are 256, 128 and 64, and the one
     at 90 compares the two kernels with each other.
  5. `+ 0x8000` dropped from the luma: the three RGB batches fail (crop_ex_kernel<1> against crop_ex_kernel<0> on luma(rgb));
     of the existing tests test_gpu_frontend.py::test_rgb_equals_pil_luma_plane noticed.
"""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crops_ref as R  # noqa: E402
from oracle import crops_ref as O  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from esa_pose_estimation_amd import _lib, config, crops, seg_hrnet3, synth
    e = dict(lib=_lib.lib(), L=_lib, config=config, crops=crops, seg_hrnet3=seg_hrnet3, synth=synth, worst={}, t0=time.time(),
             cases=0, launches=0, memo={})
    yield e
    print(f"\n{e['cases']} served crops in {e['launches']} launches, {time.time() - e['t0']:.1f} s; worst |u8 - exact| per class "
          f"(bound {R.B:.5f}):")
    for cls in sorted(e["worst"]):
        print(f"  {cls:<14} {e['worst'][cls][0]:.3f}  {e['worst'][cls][1]}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                     # a copy: the tables' frames are read-only


def _i32(seq):
    return torch.tensor(np.asarray(seq, dtype=np.int64).astype(np.int32)).cuda()


def _finish(env, rc, out):
    """The call returned 0 and the device is well: a refused call of a valid case or a failed launch ends the session, nothing
    more is started on the device after an error."""
    if rc != 0:
        pytest.exit("library call failed: " + env["lib"].esahrnet_last_error().decode(errors="replace"), returncode=3)
    try:
        host = out.cpu().numpy()
    except RuntimeError as e:
        pytest.exit(f"device error after a crop launch: {e}", returncode=3)
    env["launches"] += 1
    return host[:, 0]


def _crops(env, frames, boxes, S, mean=R.MEAN, std=R.STD):
    """esahrnet_crops: crop i of frames [n, FH, FW] (numpy u8) -> [n, S, S] f32."""
    n, fh, fw = frames.shape
    assert n == len(boxes)
    f, b = _dev(frames), _i32(boxes)
    out = torch.full((n, 1, S, S), NAN, device="cuda")
    rc = env["lib"].esahrnet_crops(f.data_ptr(), n, fh, fw, b.data_ptr(), S, mean, std, out.data_ptr(), _stream())
    return _finish(env, rc, out)


def _crops_ex(env, frames, boxes, S, fidx=None, valid=None, mean=R.MEAN, std=R.STD):
    """esahrnet_crops_ex on frames [nframes, FH, FW] (gray) or [nframes, FH, FW, 3] (RGB) -> [m, S, S] f32."""
    nframes, fh, fw = frames.shape[:3]
    m = len(boxes)
    f, b = _dev(frames), _i32(boxes)
    fi = None if fidx is None else _i32(fidx)
    va = None if valid is None else _i32(valid)
    out = torch.full((m, 1, S, S), NAN, device="cuda")
    rc = env["lib"].esahrnet_crops_ex(f.data_ptr(), nframes, fh, fw, int(frames.ndim == 4), None if fi is None else fi.data_ptr(),
                                      b.data_ptr(), None if va is None else va.data_ptr(), m, S, mean, std, out.data_ptr(),
                                      _stream())
    return _finish(env, rc, out)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


@functools.lru_cache(maxsize=None)
def _refs(fname, fi, box, S):
    """(exact, the restatement's u8) of one crop, computed once."""
    g = R.gray(fname)
    g = g if fi is None else g[fi]
    ex, u8 = R.exact(g, box, S), O.resize_u8_linear(R.padded(g, box), S, S)
    ex.setflags(write=False)
    u8.setflags(write=False)
    return ex, u8


def _hold(env, cls, name, out, refs, mean=R.MEAN, std=R.STD):
    """The three assertions on one served crop [S, S]."""
    ex, u8 = refs
    left = int(np.isnan(out).sum())
    err = float(np.abs(R.recover_u8(np.nan_to_num(out, nan=0.0), mean, std) - ex).max())
    bits = _same_bits(out, R.normalise(u8, mean, std))
    print(f"{name}: |u8 - exact| {err:.3f} (bound {R.B:.3f}), bits of the restatement {bits}, NaN left {left}")
    assert left == 0, (name, left)                                  # 3. every element written
    assert err <= R.B, (name, err)                                  # 1. the independent rule
    assert bits, name                                               # 2. the restatement, bit for bit
    env["cases"] += 1
    if err >= env["worst"].get(cls, (-1.0, ""))[0]:
        env["worst"][cls] = (err, name)


# ---- single crops: every class, both kernels ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_served_row(env, case):
    frame = R.frame(case.frame)
    refs = _refs(case.frame, None, case.box, case.S)
    a = _crops(env, frame[None], [case.box], case.S, case.mean, case.std)[0]
    b = _crops_ex(env, frame[None], [case.box], case.S, mean=case.mean, std=case.std)[0]
    _hold(env, case.cls, case.name + " crop_kernel", a, refs, case.mean, case.std)
    _hold(env, case.cls, case.name + " crop_ex_kernel<0>", b, refs, case.mean, case.std)
    assert _same_bits(a, b), case.name
    if R.source_shape(case.box) == (case.S, case.S):                # identity: the source pixels themselves
        x0, y0, x1, y1 = case.box
        assert np.array_equal(R.recover_u8(a, case.mean, case.std), frame[y0:y1, x0:x1]), case.name
    if R.source_shape(case.box) == (2 * case.S, 2 * case.S):        # exact 2x: (a + b + c + d + 2) >> 2
        x0, y0, x1, y1 = case.box
        p = frame[y0:y1, x0:x1].astype(np.int64)
        four = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        assert np.array_equal(R.recover_u8(a, case.mean, case.std), (four + 2) >> 2), case.name


# ---- launches of several crops ------------------------------------------------------------------------------------------------
def _batch_out(env, b):
    """(crop_kernel on the gathered gray frames, crop_ex_kernel<0> on the gray frames with the index), launched once."""
    if b.name not in env["memo"]:
        g = R.gray(b.frame)
        ident = tuple(b.fidx) == tuple(range(g.shape[0]))
        env["memo"][b.name] = (_crops(env, g[list(b.fidx)], b.boxes, b.S),
                               _crops_ex(env, g, b.boxes, b.S, fidx=None if ident else b.fidx))
    return env["memo"][b.name]


@pytest.mark.parametrize("batch", R.BATCHES, ids=[b.name for b in R.BATCHES])
def test_batch(env, batch):
    a, b = _batch_out(env, batch)
    for i, (box, fi) in enumerate(zip(batch.boxes, batch.fidx)):
        refs = _refs(batch.frame, fi, box, batch.S)
        _hold(env, "batching", f"batching-{batch.name}-{i} crop_kernel", a[i], refs)
        _hold(env, "batching", f"batching-{batch.name}-{i} crop_ex_kernel<0>", b[i], refs)
    assert _same_bits(a, b), batch.name
    if batch.rgb:                                                   # crop_ex_kernel<1> == crop_ex_kernel<0> on luma(rgb)
        rgb = R.frame(batch.frame)
        assert rgb.ndim == 4 and rgb.shape[3] == 3
        c = _crops_ex(env, rgb, batch.boxes, batch.S, fidx=batch.fidx)
        assert not np.isnan(c).any() and _same_bits(c, b), batch.name


def test_a_crop_does_not_depend_on_its_batch(env):
    by = {b.name: b for b in R.BATCHES}
    alone = _batch_out(env, by["alone"])
    for name, at in R.TARGET_AT.items():
        got = _batch_out(env, by[name])
        for k in (0, 1):                                            # crop_kernel, crop_ex_kernel<0>
            assert _same_bits(got[k][at], alone[k][0]), (name, k)


# ---- crops esahrnet_crops_ex must not serve -----------------------------------------------------------------------------------
def _alone(env):
    if "ns_alone" not in env["memo"]:
        g = R.frame("A3")
        env["memo"]["ns_alone"] = [_crops_ex(env, g, [box], R.NS_S, fidx=[fi])[0] for box, fi in zip(R.NS_BOXES, R.NS_FIDX)]
        for i, (box, fi) in enumerate(zip(R.NS_BOXES, R.NS_FIDX)):
            _hold(env, "not-served", f"not-served-base-{i} crop_ex_kernel<0>", env["memo"]["ns_alone"][i], _refs("A3", fi, box, R.NS_S))
    return env["memo"]["ns_alone"]


@pytest.mark.parametrize("row", R.NOT_SERVED, ids=[r[0] for r in R.NOT_SERVED])
def test_not_served_crop_is_zeros_and_leaves_the_others_alone(env, row):
    name, pos, box, fidx, valid = row
    alone = _alone(env)
    boxes, fi, va = list(R.NS_BOXES), list(R.NS_FIDX), [1] * len(R.NS_BOXES)
    if box is not None:
        boxes[pos] = box
    if fidx is not None:
        fi[pos] = fidx
    va[pos] = valid
    # the valid array is NULL for the rows that do not need it: both forms of the argument run
    out = _crops_ex(env, R.frame("A3"), boxes, R.NS_S, fidx=fi, valid=va if (valid == 0 or fidx is not None) else None)
    assert not np.isnan(out).any(), name
    assert not out[pos].view(np.int32).any(), name                  # +0.0 in every bit
    for i in range(len(boxes)):
        if i != pos:
            assert _same_bits(out[i], alone[i]), (name, i)


def test_several_not_served_crops_in_one_launch(env):
    alone = _alone(env)
    boxes, fi, va = list(R.NS_BOXES), list(R.NS_FIDX), [1] * len(R.NS_BOXES)
    boxes[0], fi[2], va[4] = (R.INT32_MIN, R.INT32_MIN, R.INT32_MAX, R.INT32_MAX), 3, 0
    out = _crops_ex(env, R.frame("A3"), boxes, R.NS_S, fidx=fi, valid=va)
    assert not np.isnan(out).any() and not out[[0, 2, 4]].view(np.int32).any()
    assert _same_bits(out[1], alone[1]) and _same_bits(out[3], alone[3])


# ---- the one call at a scale above 256 ----------------------------------------------------------------------------------------
def test_one_call_equals_crop_batch_then_keypoints_above_256(env):
    scale = 258                                                     # even sides: the smallest scale above 256 the network serves
    net = env["seg_hrnet3"].get_seg_model(env["config"].make_config(widths=(16, 16, 32, 64)), precision="fp32")
    net.load_state_dict(env["synth"].make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=53), strict=True)
    need = C.c_size_t()
    assert env["lib"].esahrnet_workspace_bytes(net._rt._probe, 2, 257, 257, C.byref(need)) != 0     # 257 is refused by the shape rule
    assert env["lib"].esahrnet_workspace_bytes(net._rt._probe, 2, scale, scale, C.byref(need)) == 0
    net = net.cuda().eval()
    frames = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=(2, 300, 400), dtype=np.uint8)).cuda()
    boxes = [(50, 40, 250, 260), (-20, 100, 180, 330)]              # the second is clamped to a non-square crop box
    x, rboxes, rrates = env["crops"].crop_batch(frames, boxes, scale)
    assert rboxes[1][2] - rboxes[1][0] != rboxes[1][3] - rboxes[1][1]
    with torch.no_grad():
        rkp, ridx = net(x, output="keypoints+index", refine="get_final")
        from esa_pose_estimation_amd.inference import LoaderRequest
        r = net._loader(LoaderRequest("get_final"), frames, boxes, None, scale, "val", None, 0.229, None)
        kp, cboxes, rates, valid, idx = (r[n] for n in ("kp", "boxes", "rates", "valid", "idx"))
        kp2, cboxes2, rates2, valid2 = net.frames_to_keypoints(frames, boxes, scale=scale, refine="get_final")
    torch.cuda.synchronize()
    assert kp.shape == (2, net.num_keypoints, 3) and bool(torch.isfinite(rkp).all())
    for got in (kp, kp2):
        assert torch.equal(got.contiguous().view(torch.int32), rkp.contiguous().view(torch.int32))
    assert torch.equal(idx, ridx)
    assert cboxes.tolist() == rboxes == cboxes2.tolist() and rates.tolist() == rrates == rates2.tolist()
    assert valid.tolist() == [1, 1] == valid2.tolist()
