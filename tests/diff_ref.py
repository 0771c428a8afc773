"""numpy restatement of the precision report's record (include/esahrnet.h: esahrnet_diff_record).  Per element, in float32:
d = a - b (one rounding), err = |d|; an element is compared only if a and b are both finite.  The sums are float64 sums of
the float32 err, err^2 (exact in float64) and b^2 (exact); `at` is the smallest index among the elements that reach the
largest error.  The format packers are those of tests/stats_ref.py.

record(a, b, e) takes ONE image's real channels in the order the record indexes them: [H, W, C] flattened for the NHWC
formats (index pixel * C + c), [C, H, W] flattened for plain f32 NCHW.  A enters as ldexp(a, e) in float32."""
import numpy as np

from esa_pose_estimation_amd import _lib

AT_NONE = 0xFFFFFFFF
SUMS = ("sum_abs_err", "sum_sq_err", "sum_sq_ref")


def _kind(v):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    return np.where(np.isnan(v), 1, np.where(v == np.inf, 2, np.where(v == -np.inf, 3, 0)))


def record(a, b, e=0):
    a = np.ldexp(np.asarray(a, dtype=np.float32).reshape(-1), np.int32(e)).astype(np.float32)
    b = np.asarray(b, dtype=np.float32).reshape(-1)
    assert a.shape == b.shape
    r = np.zeros((), dtype=_lib.diff_dtype())
    ka, kb = _kind(a), _kind(b)
    both = (ka == 0) & (kb == 0)
    with np.errstate(over="ignore", invalid="ignore"):
        err = np.abs((a - b).astype(np.float32))[both]
    bb, aa = b[both], a[both]
    e64, b64 = err.astype(np.float64), bb.astype(np.float64)
    with np.errstate(over="ignore"):
        r["sum_abs_err"] = e64.sum()
        r["sum_sq_err"] = (e64 * e64).sum()
        r["sum_sq_ref"] = (b64 * b64).sum()
    r["max_abs_err"] = err.max() if err.size else 0.0
    r["max_abs_ref"] = np.abs(bb).max() if err.size else 0.0
    r["max_abs_test"] = np.abs(aa).max() if err.size else 0.0
    r["at"] = np.flatnonzero(both)[np.argmax(err)] if err.size else AT_NONE       # (argmax: the first of equal maxima)
    r["n_compared"] = both.sum()
    r["n_nonfinite_test"] = (ka != 0).sum()
    r["n_nonfinite_ref"] = (kb != 0).sum()
    r["n_class_differs"] = (ka != kb).sum()
    return r


def records_nchw(a, b, e=0):
    """a, b [N, C, H, W], compared as plain f32 NCHW tensors (`at` = the flat index inside the image) -> records [N]."""
    return np.stack([record(x, y, e) for x, y in zip(np.asarray(a), np.asarray(b))])


def records_nhwc(a, b, e=0):
    """a, b [N, C, H, W] (real channels), compared where they lie in NHWC storage (`at` = pixel * C + c) -> records [N]."""
    t = lambda v: np.transpose(np.asarray(v, dtype=np.float32), (0, 2, 3, 1))      # noqa: E731
    return np.stack([record(x, y, e) for x, y in zip(t(a), t(b))])


def assert_records(got, want, what=""):
    """The three maxima, `at` and the four counters exactly; the three sums within 1e-9 relative (the bound
    tests/test_gpu_stats.py holds sum_abs to: f64 rounding of at most ~1e6 additions)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name, _ in _lib.DIFF_FIELDS:
        if name in SUMS:
            g, w = got[name], want[name]
            ok = (np.abs(g - w) <= 1e-9 * np.abs(w)) | ((g == w) & np.isinf(w))     # (an overflowed difference: +inf on both sides)
            assert np.all(ok), (what, name, g, w)
        else:
            assert np.array_equal(got[name], want[name]), (what, name, got[name], want[name])
