"""The precision report without a GPU (include/esahrnet.h: esahrnet_diff_*, esahrnet_forward_diff, esahrnet_tensor_diff): the
declarations, the one description of the 64-byte record, the pairing of two plans' rows on uncommitted handles, the workspace
query, the refusals that come before a committed handle is needed, and the kernels' resource usage.  tests/test_gpu_diff.py
runs the scan."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from esa_pose_estimation_amd import _lib, build, config, hrnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "esahrnet.h")).read()
ENTRIES = ("esahrnet_tensor_diff_workspace_bytes", "esahrnet_tensor_diff", "esahrnet_diff_row_get",
           "esahrnet_forward_diff_workspace_bytes", "esahrnet_forward_diff")
P = 0x10000                                             # a 256-byte aligned number, never dereferenced
C_TYPES = {"double": "f8", "float": "f4", "uint32_t": "u4"}
NETS = {"hrnet2": (1, 11, 0), "hrnet3": (1, 30, 1), "hrnet": (3, 32, 0)}       # cin, K, variant
W8, W16, W32 = (8, 16, 32, 64), (16, 32, 64, 128), (32, 64, 128, 256)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)


def err(lib):
    return lib.esahrnet_last_error().decode()


class Handle:
    """An uncommitted handle: the plan of a configuration, no device."""

    def __init__(self, net, widths, precision, k=None, env=()):
        cin, k0, variant = NETS[net]
        self.lib = _lib.lib()
        self.h = C.c_void_p()
        s = hrnet._cfg_struct(config.make_config(widths=widths), cin, k or k0, variant, precision)
        for name in env:                    # the plan switches are read once, at create
            os.environ[name] = "1"
        try:
            _lib.check(self.lib.esahrnet_create(C.byref(s), 0, C.byref(self.h)))
        finally:
            for name in env:
                del os.environ[name]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.esahrnet_destroy(self.h)

    def stats_rows(self, n, hh, ww):
        count = C.c_int()
        _lib.check(self.lib.esahrnet_stats_rows(self.h, C.byref(count)))
        out = []
        for i in range(count.value):
            d = _lib.StatsRowDesc()
            _lib.check(self.lib.esahrnet_stats_row_get(self.h, i, n, hh, ww, C.byref(d)))
            out.append(d)
        return out

    def diff_rows(self, ref, n, hh, ww):
        out = []
        for i in range(len(self.stats_rows(n, hh, ww))):
            d = _lib.DiffRowDesc()
            _lib.check(self.lib.esahrnet_diff_row_get(self.h, ref.h, i, n, hh, ww, C.byref(d)))
            out.append(d)
        return out


def test_declared_in_header_and_binding_with_abi_6():
    assert re.search(r"#define\s+ESAHRNET_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    assert _lib.lib().esahrnet_abi_version() == 6
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", HEADER), name
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name), name


def test_one_description_of_the_record():
    """ESAHRNET_DIFF_FIELDS in the header = _lib.DIFF_FIELDS, name for name and type for type; no holes; 64 bytes."""
    body = re.search(r"#define ESAHRNET_DIFF_FIELDS\(X\)(.*?)\ntypedef struct esahrnet_diff_record", HEADER, re.S).group(1)
    header_fields = tuple((name, C_TYPES[ctype]) for ctype, name in re.findall(r"X\((\w+),\s*(\w+)\)", body))
    assert header_fields == _lib.DIFF_FIELDS
    assert re.search(r"#define\s+ESAHRNET_DIFF_RECORD_BYTES\s+64\b", HEADER) and _lib.DIFF_RECORD_BYTES == 64
    assert C.sizeof(_lib.DiffRecord) == 64
    dt = _lib.diff_dtype()
    assert dt.itemsize == 64 and dt.names == tuple(n for n, _ in _lib.DIFF_FIELDS)
    off = 0
    for name, t in _lib.DIFF_FIELDS:
        assert getattr(_lib.DiffRecord, name).offset == off == dt.fields[name][1], name
        assert dt.fields[name][0] == np.dtype(t)
        off += np.dtype(t).itemsize
    assert _lib.DiffRecord.reserved.offset == off == 56
    # the row description: the header's struct, field for field
    body = re.search(r"typedef struct esahrnet_diff_row_desc \{(.*?)\} esahrnet_diff_row_desc;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"(?:char|int)\s+([^;]+);", body) for n in re.findall(r"(\w+)(?:\[\d+\])?", decl) if not n.isdigit()]
    assert names == [f[0] for f in _lib.DiffRowDesc._fields_]
    assert C.sizeof(_lib.DiffRowDesc) == 96 + 8 * 4


# The pairing an earlier label-parsing experiment reached (tested handle against precision "fp32"): (net, widths, precision of
# the tested handle, its plan switches, crop) -> (paired rows at least, keys that must stay unpaired).  The counts are floors.
PAIRING = [
    ("hrnet2", W32, "fp16", (), 64, 100, ("stem1",)),
    ("hrnet2", W32, "bf16", (), 64, 100, ("stem1",)),
    ("hrnet2", W32, "bf16x3", (), 64, 93, ()),
    ("hrnet2", W8, "fp16", (), 64, 100, ("stem1",)),
    ("hrnet2", W8, "fp16", (), 18, 100, ("stem1",)),
    ("hrnet2", W8, "bf16x3", (), 64, 96, ()),
    ("hrnet2", W8, "bf16x3", (), 18, 96, ()),
    ("hrnet3", W32, "bf16", (), 64, 102, ("stem1",)),
    ("hrnet3", W32, "bf16x3", (), 64, 104, ()),
    ("hrnet2", W16, "fp32", ("ESAHRNET_NO_JOBS",), 64, 100, ()),
    ("hrnet3", W16, "fp32", ("ESAHRNET_NO_JOBS",), 64, 106, ()),
]


@pytest.mark.parametrize("net,widths,precision,env,size,floor,unpaired", PAIRING,
                         ids=[f"{c[0]}-w{c[1][0]}-{c[2]}-{c[4]}" + ("-nojobs" if c[3] else "") for c in PAIRING])
def test_rows_pair_by_what_the_tensor_is(net, widths, precision, env, size, floor, unpaired):
    n = 2
    with Handle(net, widths, precision, env=env) as A, Handle(net, widths, "fp32") as B:
        rows_a, rows_b = A.stats_rows(n, size, size), B.stats_rows(n, size, size)
        before = [(r.name, r.def_op, r.scanned) for r in rows_a]
        d = A.diff_rows(B, n, size, size)
        assert len(d) == len(rows_a) and d[-1].key == b"heatmaps"
        assert d[-1].compared == 1 and d[-1].ref_row == len(rows_b) - 1 and d[-1].fmt == d[-1].ref_fmt == -1
        compared = [r for r in d if r.compared]
        assert len(compared) >= floor, (len(compared), sum(r.scanned for r in rows_a))
        keys = [r.key for r in compared]
        assert len(set(keys)) == len(keys) and all(keys), "every key is unique among the compared rows"
        refs = [r.ref_row for r in compared]
        assert len(set(refs)) == len(refs), "no reference row is paired twice"
        keys_b = [r.key for r in B.diff_rows(B, n, size, size)]
        for i, r in enumerate(d):
            sa = rows_a[i]
            assert (r.c, r.h, r.w, r.fmt) == (sa.c, sa.h, sa.w, sa.fmt), r.key
            if sa.name.decode() in A_TAPS(A):
                assert r.key == sa.name, "a tensor with a tap name has it for a key"
            if r.compared:
                sb = rows_b[r.ref_row]
                assert sa.scanned and sb.scanned and (sb.c, sb.h, sb.w) == (r.c, r.h, r.w) and r.ref_fmt == sb.fmt, r.key
                assert keys_b[r.ref_row] == r.key
            if r.ref_row < 0:
                assert not r.compared
            assert r.exponent == 0
        for name in unpaired:
            assert [r.compared for r in d if r.key == name.encode()] == [0], name
        # no key is made of a label: none carries the words the merged launches' labels do
        assert not [r.key for r in d if b" + " in r.key or b"launch" in r.key]
        # every scanned convolution output pairs: what is left over is what the other plan never stores
        left = [r.key.decode() for i, r in enumerate(d) if rows_a[i].scanned and not r.compared]
        assert len(left) <= 3 or net == "hrnet3", left
        assert [(r.name, r.def_op, r.scanned) for r in A.stats_rows(n, size, size)] == before      # the query changes nothing


def A_TAPS(H):
    buf = C.create_string_buffer(96)
    names = set()
    for i in range(H.lib.esahrnet_tap_count(H.h)):
        _lib.check(H.lib.esahrnet_tap_name(H.h, i, buf, 96))
        names.add(buf.value.decode())
    return names


def test_a_handle_against_itself_and_against_another_network():
    n, size = 2, 64
    with Handle("hrnet2", W8, "fp32") as A, Handle("hrnet3", W16, "fp32") as B3, Handle("hrnet2", W8, "fp16") as F:
        d = A.diff_rows(A, n, size, size)
        rows = A.stats_rows(n, size, size)
        for i, r in enumerate(d):           # against itself: every scanned row with a unique key is compared with itself
            if r.compared:
                assert r.ref_row == i
            assert r.compared == (1 if rows[i].scanned and [x.key for x in d].count(r.key) == 1 and r.key else 0), r.key
        assert sum(r.compared for r in d) == sum(r.scanned for r in rows)
        # an fp16 handle against itself: the reference side is not f32, only f32 rows and the heat-maps are compared
        df = F.diff_rows(F, n, size, size)
        assert df[-1].compared == 1 and all(r.fmt in (2, -1) for r in df if r.compared)
        assert any(r.ref_row >= 0 and not r.compared for r in df)
        # another network: the query answers, nothing but same-shaped tensors is compared (K differs: not the heat-maps)
        d3 = A.diff_rows(B3, n, size, size)
        assert d3[-1].compared == 0
        rows3 = B3.stats_rows(n, size, size)
        for r in d3:
            if r.compared:
                assert (rows3[r.ref_row].c, rows3[r.ref_row].h, rows3[r.ref_row].w) == (r.c, r.h, r.w)


def test_exponent_follows_the_scale_exponents():
    lib = _lib.lib()
    n, size = 2, 64
    with Handle("hrnet2", W8, "fp16") as A, Handle("hrnet2", W8, "fp32") as B:
        groups = C.c_int()
        _lib.check(lib.esahrnet_scale_groups(A.h, C.byref(groups)))
        assert groups.value > 4
        exps = [(7 * g) % 23 - 11 for g in range(groups.value)]
        _lib.check(lib.esahrnet_set_scale_exponents(A.h, (C.c_int32 * groups.value)(*exps), groups.value))
        d = A.diff_rows(B, n, size, size)
        g = C.c_int()
        seen = set()
        for i, r in enumerate(d[:-1]):
            _lib.check(lib.esahrnet_scale_row_group(A.h, i, C.byref(g)))
            assert r.exponent == (exps[g.value] if g.value >= 0 else 0), r.key
            if r.compared and g.value >= 0:
                seen.add(g.value)
        assert d[-1].exponent == 0 and len(seen) > 4
        # the reference's exponents never enter (its compared tensors are f32 and belong to no group)
        assert all(r.exponent == 0 for r in B.diff_rows(A, n, size, size))


def _keep_ws(H, n, hh, ww):
    lib, need = H.lib, C.c_size_t()
    _lib.check(lib.esahrnet_set_debug_keep(H.h, 1))
    _lib.check(lib.esahrnet_workspace_bytes(H.h, n, hh, ww, C.byref(need)))
    _lib.check(lib.esahrnet_set_debug_keep(H.h, 0))
    return (need.value + 255) // 256 * 256


@pytest.mark.parametrize("precision", ["fp16", "bf16x3", "fp32"])
def test_workspace_is_two_keep_mode_forwards_and_the_partials(precision):
    lib = _lib.lib()
    n, hh, ww = 3, 64, 48
    with Handle("hrnet2", W16, precision) as A, Handle("hrnet2", W16, "fp32") as B:
        need, part = C.c_size_t(), C.c_size_t()
        assert lib.esahrnet_forward_diff_workspace_bytes(A.h, B.h, n, hh, ww, C.byref(need)) == 0, err(lib)
        rows_a, rows_b = A.stats_rows(n, hh, ww), B.stats_rows(n, hh, ww)
        partials = 0
        for i, r in enumerate(A.diff_rows(B, n, hh, ww)):
            if not r.compared:
                continue
            if r.fmt == -1:
                _lib.check(lib.esahrnet_tensor_diff_workspace_bytes(-1, 0, -1, 0, n, r.c, r.h, r.w, C.byref(part)))
            else:       # (the partials depend on the real channels and the extent, not on the padding: any valid one serves)
                cp = -(-r.c // 8) * 8
                _lib.check(lib.esahrnet_tensor_diff_workspace_bytes(r.fmt, cp, r.ref_fmt, cp, n, r.c, r.h, r.w, C.byref(part)))
            partials += part.value
        want = _keep_ws(A, n, hh, ww) + _keep_ws(B, n, hh, ww) + partials
        assert need.value == (want + 255) // 256 * 256
        # keep states are left as found: the plain workspace is still the small one
        small = C.c_size_t()
        _lib.check(lib.esahrnet_workspace_bytes(A.h, n, hh, ww, C.byref(small)))
        assert small.value < _keep_ws(A, n, hh, ww)
        assert len(rows_a) and len(rows_b)


def test_refusals_of_the_handle_entries():
    lib = _lib.lib()
    d, need = _lib.DiffRowDesc(), C.c_size_t()
    with Handle("hrnet2", W8, "fp16") as A, Handle("hrnet2", W8, "fp32") as B:
        a, b = A.h, B.h
        for args in ((None, b, 0, 1, 64, 64, C.byref(d)), (a, None, 0, 1, 64, 64, C.byref(d)), (a, b, 0, 1, 64, 64, None)):
            assert lib.esahrnet_diff_row_get(*args) == 1 and err(lib) == "diff_row_get: null argument"
        rows = len(A.stats_rows(1, 64, 64))
        assert lib.esahrnet_diff_row_get(a, b, rows, 1, 64, 64, C.byref(d)) == 1
        assert err(lib) == f"diff_row_get: row {rows} out of range (0..{rows - 1})"
        assert lib.esahrnet_diff_row_get(a, b, -1, 1, 64, 64, C.byref(d)) == 1 and "out of range" in err(lib)
        assert lib.esahrnet_diff_row_get(a, b, 0, 0, 64, 64, C.byref(d)) == 1 and err(lib) == "batch must be positive (got 0)"
        assert lib.esahrnet_diff_row_get(a, b, 0, 1, 63, 64, C.byref(d)) == 1 and err(lib).startswith("crop 63x64: height and width")
        for args in ((None, b, 1, 64, 64, C.byref(need)), (a, None, 1, 64, 64, C.byref(need)), (a, b, 1, 64, 64, None)):
            assert lib.esahrnet_forward_diff_workspace_bytes(*args) == 1
            assert err(lib) == "forward_diff_workspace_bytes: null argument"
        assert lib.esahrnet_forward_diff_workspace_bytes(a, b, 1, 64, 63, C.byref(need)) == 1 and err(lib).startswith("crop 64x63")
        assert lib.esahrnet_forward_diff_workspace_bytes(a, b, 0, 64, 64, C.byref(need)) == 1
        assert err(lib) == "batch must be positive (got 0)"
        good = dict(h=a, href=b, x=P, n=1, hh=64, ww=64, heat=P, heat_ref=P, ws=P, wsb=1 << 30, diff=P, stream=None)

        def call(**kw):
            v = {**good, **kw}
            return lib.esahrnet_forward_diff(v["h"], v["href"], v["x"], v["n"], v["hh"], v["ww"], v["heat"], v["heat_ref"], v["ws"],
                                             v["wsb"], v["diff"], v["stream"])
        for name in ("h", "href", "x", "heat", "heat_ref", "ws", "diff"):
            assert call(**{name: None}) == 1 and err(lib) == "forward_diff: null argument", name
        # null arguments come first, then the commit; everything behind it needs committed handles (tests/test_gpu_diff.py)
        assert call() == 1 and err(lib) == "forward_diff: esahrnet_commit has not been called on the tested handle"
        assert call(n=0, wsb=0, ws=P + 16, diff=P + 4) == 1 and err(lib).startswith("forward_diff: esahrnet_commit has not been called")


# configurations that differ in anything but `precision`: refused with the first differing field, by the workspace query on
# uncommitted handles and (behind the commit and the device) by esahrnet_forward_diff through the same check
@pytest.mark.parametrize("other,field", [
    (("hrnet3", W16, "fp32", None), "variant (0 against 1)"),
    (("hrnet2", W16, "fp32", 12), "num_keypoints (11 against 12)"),
    (("hrnet", W16, "fp32", 11), "cin (1 against 3)"),
    (("hrnet2", (16, 32, 64, 96), "fp32", None), "widths[3] (128 against 96)"),
    (("hrnet2", W32, "fp32", None), "widths[0] (16 against 32)"),
], ids=["hrnet3", "K12", "cin3", "width3", "widths"])
def test_configurations_must_agree(other, field):
    lib = _lib.lib()
    need = C.c_size_t(7)
    net, widths, precision, k = other
    with Handle("hrnet2", W16, "bf16") as A, Handle(net, widths, precision, k=k) as B:
        assert lib.esahrnet_forward_diff_workspace_bytes(A.h, B.h, 2, 64, 64, C.byref(need)) == 1
        assert err(lib) == f"forward_diff_workspace_bytes: the handles differ in {field}: they may differ in precision only"
        assert need.value == 7
        # the configuration comes before the shape
        assert lib.esahrnet_forward_diff_workspace_bytes(A.h, B.h, 0, 63, 64, C.byref(need)) == 1 and "differ in" in err(lib)
        d = _lib.DiffRowDesc()
        assert lib.esahrnet_diff_row_get(A.h, B.h, 0, 2, 64, 64, C.byref(d)) == 0        # the row query only describes


def test_refusals_of_the_tensor_entries():
    lib = _lib.lib()
    need = C.c_size_t()
    good = dict(a=P, fa=1, cpa=64, b=P, fb=2, cpb=32, e=0, n=2, c=11, h=5, w=7, ws=P, wsb=1 << 20, diff=P, stream=None)

    def call(**kw):
        v = {**good, **kw}
        return lib.esahrnet_tensor_diff(v["a"], v["fa"], v["cpa"], v["b"], v["fb"], v["cpb"], v["e"], v["n"], v["c"], v["h"], v["w"],
                                        v["ws"], v["wsb"], v["diff"], v["stream"])

    def size(**kw):
        v = {**good, **kw}
        return lib.esahrnet_tensor_diff_workspace_bytes(v["fa"], v["cpa"], v["fb"], v["cpb"], v["n"], v["c"], v["h"], v["w"], C.byref(need))
    assert lib.esahrnet_tensor_diff_workspace_bytes(1, 64, 2, 32, 2, 11, 5, 7, None) == 1
    assert err(lib) == "tensor_diff_workspace_bytes: null argument"
    for name in ("a", "b", "ws", "diff"):
        assert call(**{name: None}) == 1 and err(lib) == "tensor_diff: null argument", name
    assert call(n=0) == 1 and err(lib) == "tensor_diff: batch must be positive (got 0)"
    assert size(n=0) == 1 and err(lib) == "tensor_diff_workspace_bytes: batch must be positive (got 0)"
    for e in (-33, 33, 1 << 20):
        assert call(e=e) == 1 and err(lib) == f"tensor_diff: exponent {e} outside -32..32"
    assert call(e=32, wsb=0) == 1 and err(lib).startswith("tensor_diff: workspace too small")        # (32 itself is in range)
    assert call(e=-32, wsb=0) == 1 and err(lib).startswith("tensor_diff: workspace too small")
    for bad in (dict(fa=4), dict(fa=-2), dict(fb=1), dict(fb=0), dict(fb=3), dict(fa=-1), dict(fb=-1), dict(fa=2, fb=-1)):
        v = {**good, **bad}
        msg = f"no scan for format {v['fa']} against format {v['fb']} (0..3 against 2, or -1 against -1)"
        assert call(**bad) == 1 and err(lib) == "tensor_diff: " + msg, bad
        assert size(**bad) == 1 and err(lib) == "tensor_diff_workspace_bytes: " + msg, bad
    for bad in (dict(c=0), dict(c=33), dict(c=65, cpb=96), dict(cpa=60), dict(cpb=28), dict(cpa=8), dict(h=0), dict(w=0), dict(w=-3),
                dict(h=1 << 15, w=1 << 15, cpa=4096, cpb=4096, c=4096), dict(fa=-1, fb=-1, c=1 << 10, h=1 << 15, w=1 << 15),
                dict(fa=0, cpa=36)):
        v = {**good, **bad}
        msg = f"no scan for {v['c']} channels ({v['cpa']} and {v['cpb']} padded), {v['h']}x{v['w']}"
        assert call(**bad) == 1 and err(lib).startswith("tensor_diff: " + msg), bad
        assert size(**bad) == 1 and err(lib).startswith("tensor_diff_workspace_bytes: " + msg), bad
    # the partials: a function of the shape alone, times n.  A workgroup owns 32 KiB of B's real groups: 11 channels are two
    # groups of 8 (64 bytes of a pixel), so 512 pixels
    assert size() == 0 and need.value == 2 * 64
    assert size(n=6) == 0 and need.value == 6 * 64
    assert size(h=24, w=24) == 0 and need.value == 2 * 2 * 64                       # 576 pixels
    assert size(c=64, cpa=64, cpb=64, h=24, w=24) == 0 and need.value == 2 * 5 * 64   # 8 groups: 128 pixels per workgroup
    assert size(fa=-1, fb=-1, c=11, h=33, w=65) == 0 and need.value == 2 * 3 * 64     # 23595 elements, 8192 per workgroup
    assert call(wsb=2 * 64 - 1) == 1 and err(lib) == "tensor_diff: workspace too small (127 < 128)"
    assert call(a=P + 8) == 1 and err(lib) == "tensor_diff: a_dev and b_dev must be 16-byte aligned"
    assert call(b=P + 8) == 1 and err(lib) == "tensor_diff: a_dev and b_dev must be 16-byte aligned"
    assert call(fa=-1, fb=-1, a=P + 2) == 1 and err(lib) == "tensor_diff: a_dev and b_dev must be 4-byte aligned"
    assert call(ws=P + 4) == 1 and err(lib) == "tensor_diff: workspace must be 8-byte aligned"
    assert call(diff=P + 4) == 1 and err(lib) == "tensor_diff: diff_dev must be 8-byte aligned"
    assert call(wsb=0, ws=P + 4, diff=P + 4) == 1 and err(lib).startswith("tensor_diff: workspace too small")


def test_the_diff_kernels_use_no_scratch():
    assert "diff.hip" in build.SOURCES
    usage = json.load(open(build.USAGE))
    mine = {k: v for k, v in usage.items() if k.startswith("diff.hip:")}
    assert len(mine) == 6, sorted(mine)                 # the scan for four formats of A, the NCHW scan, the finish
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["waves_per_simd"] == 8, (k, v)
    # stats.hip's kernels are untouched: the same six entries
    assert len([k for k in usage if k.startswith("stats.hip:")]) == 6
