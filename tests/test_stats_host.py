"""The activation range report without a GPU (include/esahrnet.h: esahrnet_stats_*, esahrnet_forward_stats,
esahrnet_tensor_stats): the declarations, the one description of the 64-byte record, the row table of the three networks on
uncommitted handles, the refusals that come before a committed handle is needed, and the kernels' resource usage.
tests/test_gpu_stats.py runs the scan."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_cases as W  # noqa: E402

from esa_pose_estimation_amd import _lib, build, config, hrnet  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "esahrnet.h")).read()
ENTRIES = ("esahrnet_stats_rows", "esahrnet_stats_row_get", "esahrnet_forward_stats_workspace_bytes", "esahrnet_forward_stats",
           "esahrnet_tensor_stats_workspace_bytes", "esahrnet_tensor_stats")
NETS = ("hrnet2_w32", "hrnet_w16", "hrnet3_w16")        # seg_hrnet2, seg_hrnet, seg_hrnet3 (tests/workspace_cases.py)
P = 0x10000                                             # a 256-byte aligned number, never dereferenced
C_TYPES = {"double": "f8", "float": "f4", "uint32_t": "u4"}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)


class Handle:
    def __init__(self, key, precision):
        _, cin, k, variant, widths = W.NETS[key]
        self.lib = _lib.lib()
        self.h = C.c_void_p()
        s = hrnet._cfg_struct(config.make_config(widths=widths), cin, k, variant, precision)
        _lib.check(self.lib.esahrnet_create(C.byref(s), 0, C.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.esahrnet_destroy(self.h)

    def rows(self, n, hh, ww):
        count = C.c_int()
        _lib.check(self.lib.esahrnet_stats_rows(self.h, C.byref(count)))
        out = []
        for i in range(count.value):
            d = _lib.StatsRowDesc()
            _lib.check(self.lib.esahrnet_stats_row_get(self.h, i, n, hh, ww, C.byref(d)))
            out.append(d)
        return out

    def op_descs(self, n, hh, ww):
        out = []
        for i in range(self.lib.esahrnet_launch_count(self.h)):
            d = _lib.OpDesc()
            _lib.check(self.lib.esahrnet_op_desc_get(self.h, i, n, hh, ww, C.byref(d)))
            out.append((d.kernel, d.label, d.flops, d.bytes))
        return out

    def taps(self):
        buf = C.create_string_buffer(96)
        names = []
        for i in range(self.lib.esahrnet_tap_count(self.h)):
            _lib.check(self.lib.esahrnet_tap_name(self.h, i, buf, 96))
            names.append(buf.value.decode())
        return names


def err(lib):
    return lib.esahrnet_last_error().decode()


def test_declared_in_header_and_binding_with_abi_6():
    assert re.search(r"#define\s+ESAHRNET_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    assert _lib.lib().esahrnet_abi_version() == 6
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", HEADER), name
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name), name


def test_one_description_of_the_record():
    """ESAHRNET_STATS_FIELDS in the header = _lib.STATS_FIELDS, name for name and type for type; no holes; 64 bytes."""
    body = re.search(r"#define ESAHRNET_STATS_FIELDS\(X\)(.*?)\ntypedef struct esahrnet_stats_record", HEADER, re.S).group(1)
    header_fields = tuple((name, C_TYPES[ctype]) for ctype, name in re.findall(r"X\((\w+),\s*(\w+)\)", body))
    assert header_fields == _lib.STATS_FIELDS
    assert re.search(r"#define\s+ESAHRNET_STATS_RECORD_BYTES\s+64\b", HEADER) and _lib.STATS_RECORD_BYTES == 64
    assert C.sizeof(_lib.StatsRecord) == 64
    dt = _lib.stats_dtype()
    assert dt.itemsize == 64 and dt.names == tuple(n for n, _ in _lib.STATS_FIELDS)
    off = 0
    for name, t in _lib.STATS_FIELDS:
        assert getattr(_lib.StatsRecord, name).offset == off == dt.fields[name][1], name
        assert dt.fields[name][0] == np.dtype(t)
        off += np.dtype(t).itemsize
    assert _lib.StatsRecord.reserved.offset == off == 44


# (seg_hrnet3 refuses fp16 at create)
@pytest.mark.parametrize("key,precision", [(k, p) for k in NETS for p in (0, 1, 2, 3) if not (p == 3 and W.NETS[k][3] == 1)])
def test_rows_of_an_uncommitted_handle(key, precision):
    n, hh, ww = 3, 64, 48
    with Handle(key, precision) as H:
        lib, h = H.lib, H.h
        launches, descs = lib.esahrnet_launch_count(h), H.op_descs(n, hh, ww)
        rows = H.rows(n, hh, ww)
        names = [r.name.decode() for r in rows]
        # one row per tensor of the plan (esahrnet_debug_op_regions names them) + "heatmaps"
        count = C.c_int()
        _lib.check(lib.esahrnet_set_debug_keep(h, 1))
        _lib.check(lib.esahrnet_debug_op_count(h, n, hh, ww, C.byref(count)))
        seen, written = set(), set()
        for k in range(count.value):
            d = _lib.DebugOp()
            _lib.check(lib.esahrnet_debug_op_regions(h, n, hh, ww, k, C.byref(d)))
            seen |= {r.tensor for r in d.regions[:d.nregions]}
            written |= {r.tensor for r in d.regions[:d.nregions] if r.write}      # by an op that runs at this shape
        _lib.check(lib.esahrnet_set_debug_keep(h, 0))
        assert max(seen) < len(rows) - 1
        assert names[-1] == "heatmaps" and rows[-1].scanned == 1 and rows[-1].fmt == -1
        assert (rows[-1].c, rows[-1].h, rows[-1].w) == (W.NETS[key][2], hh, ww) and rows[-1].def_op == launches - 1
        for tap in H.taps():
            assert names.count(tap) == 1, tap
            c, th, tw = C.c_int(), C.c_int(), C.c_int()
            _lib.check(lib.esahrnet_tap_shape(h, tap.encode(), hh, ww, C.byref(c), C.byref(th), C.byref(tw)))
            r = rows[names.index(tap)]
            assert (r.c, r.h, r.w) == (c.value, th.value, tw.value), tap
        plan_fmt = {0: 0, 1: 1, 2: 2, 3: 3}[precision]
        for i, r in enumerate(rows[:-1]):
            assert r.name and -1 <= r.def_op < launches
            assert r.fmt in (plan_fmt, 2)                  # the plan's format, or a plain f32 tensor inside it
            label = descs[r.def_op][1] if r.def_op >= 0 else b""
            flat = (r.c, r.h, r.w) == (0, 0, 0)
            t_layout = b"(T layout)" in label
            unused = i not in written                       # the head alternative that does not run
            two_plane = r.c == 2 and r.fmt == 2 and W.NETS[key][3] == 1           # CBAM's maps: f32 [N][H][W][2]
            assert r.scanned == (0 if flat or t_layout or unused or two_plane or r.def_op < 0 else 1), (r.name, label)
        assert any(r.scanned for r in rows[:-1])
        # the queries change nothing
        assert lib.esahrnet_launch_count(h) == launches and H.op_descs(n, hh, ww) == descs
        need = C.c_size_t()
        assert lib.esahrnet_forward_stats_workspace_bytes(h, n, hh, ww, C.byref(need)) == 0, err(lib)
        plain = C.c_size_t()
        _lib.check(lib.esahrnet_set_debug_keep(h, 1))
        _lib.check(lib.esahrnet_workspace_bytes(h, n, hh, ww, C.byref(plain)))
        _lib.check(lib.esahrnet_set_debug_keep(h, 0))
        assert need.value > plain.value and need.value % 256 == 0           # the keep-mode plan + the partials
        small = C.c_size_t()
        _lib.check(lib.esahrnet_workspace_bytes(h, n, hh, ww, C.byref(small)))
        assert small.value < plain.value                                     # ... and the keep state was left as found
        assert lib.esahrnet_launch_count(h) == launches and H.op_descs(n, hh, ww) == descs


def test_refusals_of_the_handle_entries():
    lib = _lib.lib()
    d, rows, need = _lib.StatsRowDesc(), C.c_int(), C.c_size_t()
    with Handle("hrnet2_w32", 0) as H:
        h = H.h
        assert lib.esahrnet_stats_rows(None, C.byref(rows)) == 1 and err(lib) == "stats_rows: null argument"
        assert lib.esahrnet_stats_rows(h, None) == 1 and err(lib) == "stats_rows: null argument"
        assert lib.esahrnet_stats_row_get(None, 0, 1, 64, 64, C.byref(d)) == 1 and err(lib) == "stats_row_get: null argument"
        assert lib.esahrnet_stats_row_get(h, 0, 1, 64, 64, None) == 1 and err(lib) == "stats_row_get: null argument"
        _lib.check(lib.esahrnet_stats_rows(h, C.byref(rows)))
        assert lib.esahrnet_stats_row_get(h, rows.value, 1, 64, 64, C.byref(d)) == 1
        assert err(lib) == f"stats_row_get: row {rows.value} out of range (0..{rows.value - 1})"
        assert lib.esahrnet_stats_row_get(h, -1, 1, 64, 64, C.byref(d)) == 1 and "out of range" in err(lib)
        assert lib.esahrnet_stats_row_get(h, 0, 0, 64, 64, C.byref(d)) == 1 and err(lib) == "batch must be positive (got 0)"
        assert lib.esahrnet_stats_row_get(h, 0, 1, 63, 64, C.byref(d)) == 1 and err(lib).startswith("crop 63x64: height and width")
        assert lib.esahrnet_forward_stats_workspace_bytes(None, 1, 64, 64, C.byref(need)) == 1
        assert err(lib) == "forward_stats_workspace_bytes: null argument"
        assert lib.esahrnet_forward_stats_workspace_bytes(h, 1, 64, 64, None) == 1
        assert lib.esahrnet_forward_stats_workspace_bytes(h, 1, 64, 62 + 1, C.byref(need)) == 1 and err(lib).startswith("crop 64x63")
        good = dict(h=h, x=P, n=1, hh=64, ww=64, heat=P, ws=P, wsb=1 << 30, stats=P, stream=None)

        def call(**kw):
            a = {**good, **kw}
            return lib.esahrnet_forward_stats(a["h"], a["x"], a["n"], a["hh"], a["ww"], a["heat"], a["ws"], a["wsb"], a["stats"],
                                              a["stream"])
        for name in ("h", "x", "heat", "ws", "stats"):
            assert call(**{name: None}) == 1 and err(lib) == "forward_stats: null argument", name
        # null arguments come first, then the commit; everything behind it needs a committed handle (tests/test_gpu_stats.py)
        assert call() == 1 and err(lib) == "forward_stats: esahrnet_commit has not been called"
        assert call(n=0, wsb=0, ws=P + 16, stats=P + 4) == 1 and err(lib) == "forward_stats: esahrnet_commit has not been called"


def test_refusals_of_the_tensor_entries():
    lib = _lib.lib()
    need = C.c_size_t()
    good = dict(t=P, fmt=2, n=2, c=11, cp=32, h=5, w=7, ws=P, wsb=1 << 20, stats=P, stream=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.esahrnet_tensor_stats(a["t"], a["fmt"], a["n"], a["c"], a["cp"], a["h"], a["w"], a["ws"], a["wsb"], a["stats"],
                                         a["stream"])

    def size(**kw):
        a = {**good, **kw}
        return lib.esahrnet_tensor_stats_workspace_bytes(a["fmt"], a["n"], a["c"], a["cp"], a["h"], a["w"], C.byref(need))
    assert lib.esahrnet_tensor_stats_workspace_bytes(2, 2, 11, 32, 5, 7, None) == 1
    assert err(lib) == "tensor_stats_workspace_bytes: null argument"
    for name in ("t", "ws", "stats"):
        assert call(**{name: None}) == 1 and err(lib) == "tensor_stats: null argument", name
    assert call(n=0) == 1 and err(lib) == "tensor_stats: batch must be positive (got 0)"
    assert size(n=0) == 1 and err(lib) == "tensor_stats_workspace_bytes: batch must be positive (got 0)"
    for bad in (dict(fmt=4), dict(fmt=-2), dict(c=0), dict(c=33), dict(cp=30), dict(fmt=0, cp=12), dict(fmt=1, cp=12), dict(h=0),
                dict(w=0), dict(h=1 << 15, w=1 << 15, cp=4096, c=4096), dict(fmt=-1, c=1 << 10, h=1 << 15, w=1 << 15)):
        a = {**good, **bad}
        msg = f"no scan for format {a['fmt']}, {a['c']} channels ({a['cp']} padded), {a['h']}x{a['w']}"
        assert call(**bad) == 1 and err(lib).startswith("tensor_stats: " + msg), bad
        assert size(**bad) == 1 and err(lib).startswith("tensor_stats_workspace_bytes: " + msg), bad
    # the partials: a function of the shape alone, times n
    assert size() == 0 and need.value == 2 * 64
    one = need.value
    assert size(n=6) == 0 and need.value == 3 * one
    assert size(h=64, w=96) == 0 and need.value == 2 * 24 * 64          # 6144 pixels of 128 bytes, 32 KiB per workgroup
    assert size(fmt=-1, c=11, h=33, w=65) == 0 and need.value == 2 * 3 * 64     # 23595 elements, 8192 per workgroup
    assert call(wsb=2 * 64 - 1) == 1 and err(lib) == "tensor_stats: workspace too small (127 < 128)"
    assert call(t=P + 8) == 1 and err(lib) == "tensor_stats: t_dev must be 16-byte aligned"
    assert call(ws=P + 4) == 1 and err(lib) == "tensor_stats: workspace must be 8-byte aligned"
    assert call(stats=P + 4) == 1 and err(lib) == "tensor_stats: stats_dev must be 8-byte aligned"
    assert call(wsb=0, ws=P + 4, stats=P + 4) == 1 and err(lib).startswith("tensor_stats: workspace too small")


def test_the_scan_kernels_use_no_scratch():
    assert "stats.hip" in build.SOURCES
    usage = json.load(open(build.USAGE))
    mine = {k: v for k, v in usage.items() if k.startswith("stats.hip:")}
    assert len(mine) == 6, sorted(mine)                 # the scan in four formats, the NCHW scan, the finish
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["waves_per_simd"] == 8, (k, v)         # read-bound: full occupancy
