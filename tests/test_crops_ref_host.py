"""What holds the references of the crop stage (tests/crops_ref.py), on the CPU: the fixed-point restatement oracle/crops_ref.py
against the independent float64 rule exact(), the properties of exact() the case classes lean on, and the table's coverage.

The bound B on |resize_u8_linear - exact| in gray levels, from the restatement's arithmetic alone.  Let H0, H1 be the exact
horizontal interpolants of the two source rows and E = (1 - v) H0 + v H1 the exact value, all in [0, 255].
  horizontal pass   r = p0 * a0 + p1 * a1 with a1 = rint(f * 2048), a0 = rint((1 - f) * 2048), f the fraction of the float32
                    source coordinate.  The float32 rounding moves the coordinate by at most half an ulp, 2^-13 for coordinates in
                    [2048, 4096) (the widest padded source here is 2640), and the interpolant is piecewise linear with slope at
                    most 255 a pixel, continuous across the floor and both clamps: 255 x 2^-13.  The rounding to 11 bits moves a1
                    by at most 2^-12 of the weight, and with a0 + a1 == 2048 (asserted below for every axis of the table) the
                    value moves by |e1 (p1 - p0)|: 255 x 2^-12.  So |r / 2048 - H| <= 255 x (2^-12 + 2^-13) = 0.0934.
  `>> 4`            r >> 4 is r / 16 minus less than 1, in units of 1/128 level; the two rows enter with weights that sum to 1:
                    less than 2^-7 = 0.0078.
  vertical pass     the same two terms for (b0, b1) on values in [0, 255]: 0.0934; the horizontal errors pass through weights
                    that sum to 1.
  two `>> 16`       (b * (r >> 4)) >> 16 is in quarter levels; each truncation loses less than one: 2 x 0.25.
  `(+ 2) >> 2`      rounding of the quarter-level sum to a level: 0.5.  The clip to [0, 255] only moves towards E.
  B = 0.5 + 0.5 + 2^-7 + 2 x 255 x (2^-12 + 2^-13) = 1.19458 (crops_ref.B).  exact() itself is float64: its own error is below 1e-9.
Measured worst over the table (printed by the test, run with -s): 0.802 (blocks, a 40-pixel source at S = 513), 0.74 .. 0.79 in
the other classes, with 12.2 % of the table's 1 064 328 pixels above 0.5.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crops_ref as R  # noqa: E402
from oracle import crops_ref as O  # noqa: E402


def _oracle(frame, box, S):
    return O.resize_u8_linear(R.padded(frame, box), S, S)


def test_bound_is_the_sum_of_its_terms():
    assert R.B == 0.5 + 0.25 + 0.25 + 1 / 128 + 2 * 255 * (1 / 4096 + 1 / 8192)
    assert 1.19 < R.B < 1.20


def test_restatement_is_within_the_bound_of_exact_on_every_row():
    worst, above, total = {}, 0, 0
    for cls, name, frame, box, S in R.rows():
        rows, cols = R.source_shape(box)
        assert max(rows, cols) < 4096                                          # the derivation's coordinate range
        for src in (rows, cols):                                               # the derivation's a0 + a1 == 2048
            _, _, a0, a1 = O._coef(S, src)
            assert np.all(a0 + a1 == 2048), (name, src)
        d = np.abs(_oracle(frame, box, S).astype(np.float64) - R.exact(frame, box, S))
        above += int((d > 0.5).sum())
        total += d.size
        if d.max() > worst.get(cls, (0.0, ""))[0]:
            worst[cls] = (float(d.max()), name)
        assert d.max() <= R.B, (name, d.max())
    print("\nworst |restatement - exact| per class (bound %.5f), %.1f %% of %d pixels above 0.5:" % (R.B, 100.0 * above / total, total))
    for cls in sorted(worst):
        print(f"  {cls:<14} {worst[cls][0]:.3f}  {worst[cls][1]}")
    assert max(w[0] for w in worst.values()) > 0.5                            # the table reaches past plain rounding


def test_numpy_bilinear_equals_the_interpolate_rule():
    for cls, name, frame, box, S in R.rows():
        assert np.abs(R.bilinear(R.padded(frame, box), S, S) - R.exact(frame, box, S)).max() < 1e-9, name


def test_exact_identity_rows_equal_the_source():
    seen = 0
    for cls, name, frame, box, S in R.rows():
        if R.source_shape(box) == (S, S):
            x0, y0, x1, y1 = box
            assert np.array_equal(R.exact(frame, box, S), frame[y0:y1, x0:x1].astype(np.float64)), name
            assert np.array_equal(_oracle(frame, box, S), frame[y0:y1, x0:x1]), name
            seen += 1
    assert seen >= 3


def test_exact_2x_rows_are_the_four_pixel_mean():
    seen = 0
    for cls, name, frame, box, S in R.rows():
        if R.source_shape(box) == (2 * S, 2 * S):
            x0, y0, x1, y1 = box
            p = frame[y0:y1, x0:x1].astype(np.int64)
            four = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
            assert np.abs(R.exact(frame, box, S) - four / 4.0).max() < 1e-9, name
            assert np.abs(R.exact(frame, box, S) - ((four + 2) >> 2)).max() <= 0.5, name
            assert np.array_equal(_oracle(frame, box, S), (four + 2) >> 2), name
            seen += 1
    assert seen >= 2


def test_exact_keeps_a_constant_frame_constant():
    for c in R.CASES:
        fh, fw = R.frame_hw(c.frame)
        flat = np.full((fh, fw), 201, np.uint8)
        assert np.abs(R.exact(flat, c.box, c.S) - 201.0).max() < 1e-9, c.name      # (1 - u) * 201 + u * 201 rounds in float64


def test_replicated_line_is_distinguishable_and_the_swap_is_visible():
    ways = set()
    for c in (c for c in R.CASES if c.cls == "nonsquare"):
        frame = R.frame(c.frame)
        xs, ys = c.box[2] - c.box[0], c.box[3] - c.box[1]
        ways.add(xs > ys)
        edge, inner, outer = R.replicated_edge(frame, c.box)
        assert outer is not None                                               # the box does not end at the frame's edge
        for other in (inner, outer):
            if other is not None and edge.size >= 20:
                assert np.mean(edge != other) > 0.9, c.name
            elif other is not None:
                assert np.any(edge != other), c.name
        d = np.abs(R.exact(frame, c.box, c.S) - R.exact(frame, c.box, c.S, swapped=False))
        assert d.max() > 10 * R.B, (c.name, d.max())
    assert ways == {True, False}


def test_half_a_source_pixel_is_visible_on_every_row():
    """Every row but a 1 x 1 source, which is one constant under any geometry."""
    checked = 0
    for cls, name, frame, box, S in R.rows():
        if R.source_shape(box) == (1, 1):
            continue
        src = R.padded(frame, box)
        d = np.abs(R.bilinear(src, S, S, shift=0.5) - R.exact(frame, box, S))
        assert d.max() > 10 * R.B, (name, d.max())
        checked += 1
    assert checked >= len(R.CASES) - 2


def test_round_trip_of_the_normalisation_is_exact():
    levels = np.arange(256, dtype=np.uint8)
    for mean, std in R.NORMALISATIONS:
        out = R.normalise(levels, mean, std)
        assert out.dtype == np.float32 and np.array_equal(R.recover_u8(out, mean, std), levels)
        assert np.all(np.diff(out) > 0)
    rgb = R.frame("C3")[0]
    lum = R.luma(rgb)
    ref = (rgb[..., 0] * 0.299 + rgb[..., 1] * 0.587 + rgb[..., 2] * 0.114)
    assert lum.dtype == np.uint8 and np.abs(lum - ref).max() <= 0.5 + 1e-2     # ITU-R 601-2 in 16-bit fixed point, rounded
    assert np.array_equal(R.luma(np.full((1, 1, 3), 255, np.uint8)), [[255]]) and (rgb != rgb[..., :1]).any()


def test_table_coverage():
    by = {}
    for c in R.CASES:
        by.setdefault(c.cls, []).append(c)
        fh, fw = R.frame_hw(c.frame)
        x0, y0, x1, y1 = c.box
        assert 0 <= x0 < x1 <= fw and 0 <= y0 < y1 <= fh, c.name                # served rows stay inside the frame
    assert set(by) == set(R.CLASSES) and len({c.name for c in R.CASES}) == len(R.CASES)
    small = [R.frame_hw(f) for f in ("A", "B")]
    assert all(h % 2 and w % 2 and h != w and max(h, w) < 200 for h, w in small) and (small[0][0] < small[0][1]) != (small[1][0] < small[1][1])
    for S in {c.S for c in by["ratio"] if c.frame != "W"}:
        sides = {c.box[2] - c.box[0] for c in by["ratio"] if c.S == S and c.frame != "W"}
        assert {1, 2, 3, S - 1, S, S + 1, 2 * S} <= sides and any(k >= 4 * S and k % S for k in sides), S
    assert any(R.source_shape(c.box)[1] > 2048 and R.source_shape(c.box)[1] >= 100 * c.S for c in by["ratio"])
    assert {8, 64, 255, 256, 257, 384, 513} <= {c.S for c in by["blocks"]}
    assert all(c.box[2] - c.box[0] <= 41 for c in by["blocks"] if c.S > 256)
    assert {(c.S - 1) // 256 for c in R.CASES} >= {0, 1, 2}                    # blockIdx.y of the last column
    ns = by["nonsquare"]
    assert any(c.box[2] - c.box[0] == 1 for c in ns) and any(c.S > 256 for c in ns)
    assert any(c.box[2] - c.box[0] > c.box[3] - c.box[1] for c in ns) and any(c.box[2] - c.box[0] < c.box[3] - c.box[1] for c in ns)
    for frm in ("A", "B"):
        fh, fw = R.frame_hw(frm)
        touch = {(c.box[0] == 0, c.box[1] == 0, c.box[2] == fw, c.box[3] == fh) for c in by["position"] if c.frame == frm}
        assert len(touch) == 10, (frm, touch)       # four edges, four corners, the whole frame, the interior
    assert [c.box for c in by["workload"]] == [(0, 0, 1920, 1200)] and by["workload"][0].S == 256
    assert {(c.mean, c.std) for c in by["normalisation"]} == set(R.NORMALISATIONS)
    assert all(np.array_equal(np.sort(R.frame(c.frame), axis=None), np.arange(256)) for c in by["normalisation"])
    # batching: the target alone, first, middle, last of 7; a permuted and repeated index over three distinct frames; RGB at
    # S <= 256, S > 256 and on a non-square box
    names = {b.name: b for b in R.BATCHES}
    for n, at in R.TARGET_AT.items():
        assert names[n].boxes[at] == R.TARGET and names[n].fidx[at] == 1 and len(names[n].boxes) == (1 if n == "alone" else 7)
    p = names["permuted"]
    assert sorted(set(p.fidx)) == [0, 1, 2] and len(p.fidx) > 3 and list(p.fidx) != sorted(p.fidx)
    a3 = R.frame("A3")
    assert not any(np.array_equal(a3[i], a3[j]) for i in range(3) for j in range(i))
    rgb = [b for b in R.BATCHES if b.rgb]
    assert any(b.S <= 256 for b in rgb) and any(b.S > 256 for b in rgb)
    assert any(x[2] - x[0] != x[3] - x[1] for b in rgb for x in b.boxes)
    assert any(b.fidx == tuple(range(len(b.fidx))) == tuple(range(R.FRAMES[b.frame][0][0])) for b in R.BATCHES if not b.rgb)
    c3 = R.frame("C3")
    assert (c3[..., 0] != c3[..., 1]).mean() > 0.9 and (c3[..., 1] != c3[..., 2]).mean() > 0.9
    for b in R.BATCHES:
        fh, fw = R.frame_hw(b.frame)
        assert all(0 <= x0 < x1 <= fw and 0 <= y0 < y1 <= fh for x0, y0, x1, y1 in b.boxes) and len(b.boxes) == len(b.fidx)
        assert all(0 <= f < R.FRAMES[b.frame][0][0] for f in b.fidx)
    # not served: every kind the kernel must turn into zeros, each box really outside what the kernel serves
    fh, fw = R.frame_hw("A3")
    kinds = set()
    for name, pos, box, fidx, valid in R.NOT_SERVED:
        assert 0 <= pos < len(R.NS_BOXES) and (box is not None) + (fidx is not None) + (valid == 0) == 1, name
        if box is not None:
            x0, y0, x1, y1 = box
            assert not (0 <= x0 < x1 <= fw and 0 <= y0 < y1 <= fh), name
            assert all(R.INT32_MIN <= v <= R.INT32_MAX for v in box)
            kinds |= {k for k, hit in (("empty", x1 == x0 or y1 == y0), ("reversed", x1 < x0 or y1 < y0), ("x0<0", x0 < 0),
                                       ("x1>FW", x1 > fw), ("y1>FH", y1 > fh), ("min", R.INT32_MIN in box),
                                       ("max", R.INT32_MAX in box)) if hit}
        if fidx is not None:
            assert fidx in (-1, 3) and not 0 <= fidx < 3
            kinds.add(f"fidx{fidx}")
        if valid == 0:
            kinds.add("valid0")
    assert kinds == {"empty", "reversed", "x0<0", "x1>FW", "y1>FH", "min", "max", "fidx-1", "fidx3", "valid0"}
    assert all(0 <= x0 < x1 <= fw and 0 <= y0 < y1 <= fh for x0, y0, x1, y1 in R.NS_BOXES)


def test_crops_ref_does_not_import_the_restatement():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "crops_ref.py")).read()
    imports = [line for line in src.splitlines() if line.lstrip().startswith(("import ", "from "))]
    assert imports and not any("oracle" in line or "esa_pose" in line for line in imports)
