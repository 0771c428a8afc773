"""Host side of the convolution tests (no GPU): the emulations of tests/conv_ref.py against the project's oracles, the launch
geometry against hand-counted values, the conditions on the inputs, and the coverage condition — the kernel names
esahrnet_op_conv_kernel returns over the case table are exactly the committed list of reachable names, so that the table cannot
silently lose a kernel to a later change of the dispatch.  Everything here is on the float64 reference or on host arithmetic,
none of it on a kernel's output."""
import ctypes as C
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as CR  # noqa: E402
import head_ref as HR  # noqa: E402
from oracle import emulate_bf16 as EB  # noqa: E402
from oracle import emulate_split_bf16 as ES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = CR.R


@pytest.fixture(scope="module")
def lib():
    from esa_pose_estimation_amd import _lib
    return _lib.lib()


def _kernel(lib, r, p):
    buf = C.create_string_buffer(96)
    assert lib.esahrnet_op_conv_kernel(r.n, r.cin, r.cout, r.h, r.w, r.k, r.stride, int(r.res), p, buf, 96) == 0, lib.esahrnet_last_error()
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------- emulations
@pytest.mark.parametrize("stride", (1, 2))
def test_split_emulation_is_the_oracles(stride):
    """conv(0, ...) is oracle.emulate_split_bf16.Emu.conv bit for bit, stride and residual included."""
    r = R(2, 48, 40, 11, 13, stride=stride, res=True, relu=True)
    d = CR.conv_data(r, "signed", 0)
    want = ES.Emu({"c.weight": d["w"], "c.bias": d["b"]}).conv("c", None, d["x"], stride, True, d["res"])
    assert torch.equal(d["emu"], want)
    assert torch.equal(CR.Q[0](d["x"]), d["x"]) and torch.equal(CR.Q[0](d["res"]), d["res"])      # inputs are data of the format


def test_bf16_emulation_is_the_oracles():
    """conv(1, ...) is the convolution of oracle.emulate_bf16.forward (its inner `conv`): rounded weights, f32 accumulation,
    + bias, + residual, ReLU, one rounding — written here with the oracle's own q."""
    r = R(2, 48, 40, 11, 13, stride=2, res=True, relu=True)
    d = CR.conv_data(r, "signed", 1)
    want = EB.q(F.relu(F.conv2d(d["x"], EB.q(d["w"]), None, 2, 1) + d["b"][None, :, None, None] + d["res"]))
    assert torch.equal(d["emu"], want)
    assert torch.equal(EB.q(d["x"]), d["x"])


def test_head_ref_keeps_its_convolution():
    """head_ref._conv is conv_ref.conv (one definition): the head's stride-1 convolution without residual, every format."""
    x = CR._n("hx", 1, (1, 24, 9, 7))
    w = CR._n("hw", 2, (8, 24, 3, 3), 0.1)
    b = CR._n("hb", 3, (8,), 0.1)
    for p in (0, 1, 2, 3):
        xq = CR.Q[p](x)
        y = HR._conv(p, xq, w, b, True)
        assert torch.equal(y, CR.conv(p, xq, w, b, 1, None, True)) and torch.equal(CR.Q[p](y), y)
    assert torch.equal(HR._conv(0, CR.Q[0](x), w, None, False), CR.Q[0](HR._sb3(CR.Q[0](x), w) + 0.0))


def test_emulation_errors_are_of_the_formats_size():
    """E_emu of a plain row: a few storage quanta of the scale in the stored formats, f32 rounding noise in the fp32-grade
    mode — the rule's bound 2 E_emu + q max|ref| is neither vacuous nor loose."""
    r = R(2, 64, 64, 17, 33, res=True, relu=True)
    for p, (lo, hi) in {0: (0.2, 2.0), 1: (0.2, 2.0), 3: (0.2, 2.0), 2: (0.05, 8.0)}.items():
        d = CR.conv_data(r, "signed", p)
        e = (d["emu"].double() - d["ref"]).abs().max().item() / (CR.QUANTUM[p] * d["ref"].abs().max().item())
        assert lo <= e <= hi, (p, e)


# ---------------------------------------------------------------------------------------------- the edge regime
@pytest.mark.parametrize("shape", CR.BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_regime_shows_an_unmasked_mid_pixel_block32(shape):
    """For the reference alone: every mid pixel outside the image would be > 0 before masking, and a bblock32 that kept them
    would miss the rule's bound by far on every image."""
    n, h, w = shape
    d = CR.block_data(n, h, w, "edge")
    assert CR.unmasked_ring_min(d["x"], d["w1"], d["b1"]) >= 1.0
    wrong = CR.ref_block32(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], masked=False)
    bound = 2 * (d["emu"].double() - d["ref"]).abs().max().item() + CR.QUANTUM[0] * d["ref"].abs().max().item()
    per_image = (wrong - d["ref"]).abs().amax((1, 2, 3))
    print(f"unmasked - masked: {per_image.min().item():.3e} at least, bound {bound:.3e}")
    assert per_image.min().item() > 100 * bound


@pytest.mark.parametrize("case", CR.STEM2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_edge_regime_shows_an_unmasked_mid_pixel_stem(case):
    n, cin, h, w, cmid, cout, p = case
    d = CR.stem2_data(n, cin, h, w, cmid, cout, "edge", p)
    assert CR.unmasked_ring_min(d["x"], d["w1"], d["b1"]) >= 1.0
    wrong = CR.ref_stem2(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], masked=False)
    bound = 2 * (d["emu"].double() - d["ref"]).abs().max().item() + CR.QUANTUM[p] * d["ref"].abs().max().item()
    assert (wrong - d["ref"]).abs().amax((1, 2, 3)).min().item() > 100 * bound


def test_positive_regime_is_positive():
    r = R(2, 64, 64, 17, 33, res=True, relu=True)
    d = CR.conv_data(r, "positive", 0)
    assert all(bool((d[k] >= 0).all()) for k in ("x", "w", "b", "res")) and bool((d["ref"] > 0).all())


# ---------------------------------------------------------------------------------------------- geometry, hand-counted
def test_geometry_against_hand_counted_values():
    # 3 images of 20x24, 64 -> 128 split-bf16, stride 1: 3 row tiles of 8 x 2 column tiles of 16 x 2 slices of 64 couts = 36 items
    r = R(3, 64, 128, 20, 24)
    assert CR.stream_geometry(r, 0) == dict(items=36, ctiles=2, grid=36, double_buffered=True)
    assert CR.stream_geometry(r, 0, 1) == dict(items=36, ctiles=2, grid=2, double_buffered=False)          # 18 items a workgroup
    assert CR.stream_geometry(r, 0, 3) == dict(items=36, ctiles=2, grid=6, double_buffered=False)
    # 96 couts in the split format: three slices of 32; a grid of 2 stays below them (slices change inside a workgroup), 4 -> 3
    r = R(3, 64, 96, 20, 24)
    assert CR.stream_geometry(r, 0, 1)["grid"] == 2 and CR.stream_geometry(r, 0, 2)["grid"] == 3 and CR.stream_geometry(r, 0)["items"] == 54
    assert CR.stream_geometry(r, 1)["ctiles"] == 2                                                         # bf16: 128 padded couts
    # stride 2, 17x31 -> 9x16: 3 row tiles of 4 x 1 column tile; never double-buffered
    assert CR.stream_geometry(R(3, 32, 128, 17, 31, stride=2), 0, 1) == dict(items=18, ctiles=2, grid=2, double_buffered=False)
    assert not CR.stream_geometry(R(1, 32, 64, 8, 32, stride=2), 0)["double_buffered"]
    # the persistent tile kernel: 3 images x (1 x 2 tiles of 16x16) x 3 slices of 32
    assert CR.tile_geometry(R(3, 32, 96, 16, 24), 1) == dict(items=18, ctiles=3, grid=2)
    assert CR.x6_geometry(R(3, 64, 128, 20, 24), 1) == dict(items=36, ctiles=2, grid=2)
    assert CR.x6_geometry(R(2, 32, 96, 20, 24), 256, 4) == dict(items=36, ctiles=3, grid=3)                # test_gpu_x6_resident's case
    # 1x1: 2 x 17 rows x 3 tiles of 16 columns = 102 tiles; the 16-bit formats take two tiles a wave from 32 a CU on
    r = R(2, 64, 64, 17, 33, k=1)
    assert CR.conv1x1_geometry(r, 1) == dict(ntiles=102, kern2=False, nblk=26, nsplit=1)
    assert CR.conv1x1_geometry(r, 1, 3) == dict(ntiles=102, kern2=True, nblk=13, nsplit=1)
    assert CR.conv1x1_geometry(r, 1, 4)["kern2"] is False and CR.conv1x1_geometry(r, 0, 1)["kern2"] is False
    assert CR.conv1x1_geometry(R(1, 384, 64, 17, 33, k=1), 1, 1)["kern2"] is False                         # six blocks: no kern2
    # 1024 couts on 2 x 8 rows x 1 tile = 16 tiles = 4 workgroups: the couts cut eight ways on the whole chip, not at all on one CU
    r = R(2, 64, 1024, 8, 8, k=1)
    assert [CR.conv1x1_geometry(r, p, c)["nsplit"] for p in (0, 1, 3) for c in (256, 1, 2, 3)] == [8, 1, 2, 3] * 3
    assert CR.conv1x1_geometry(R(2, 64, 992, 8, 8, k=1), 0)["nsplit"] == 1
    # the register-resident fp32-grade 1x1: 16 tiles, two a wave -> 2 workgroups; 256 couts = 16 tiles of 16 in 4 slices of 4
    assert CR.conv1x1_x6_geometry(R(2, 64, 256, 8, 8, k=1)) == dict(ntiles=16, nblk=2, per=4, slices=4)
    assert CR.conv1x1_x6_geometry(R(2, 64, 256, 8, 8, k=1), 1) == dict(ntiles=16, nblk=2, per=8, slices=2)
    assert CR.conv1x1_x6_geometry(R(2, 256, 480, 5, 17, k=1), 1) == dict(ntiles=20, nblk=5, per=30, slices=1)
    assert CR.block_geometry(3, 20, 24, 1) == dict(items=12, grid=1) and CR.block_geometry(3, 20, 24) == dict(items=12, grid=12)


def test_sweeps_reach_the_other_launch_form():
    """Every sweep case: unlimited it is one form, under the limits the other — and under a limit of 1 a workgroup of a
    persistent kernel walks at least four items, across cout slices and image boundaries (three images)."""
    for r, p, what in CR.SWEEP_CASES:
        if what in ("stream", "tile", "x6"):
            geo = {"stream": lambda c: CR.stream_geometry(r, p, c), "tile": lambda c: CR.tile_geometry(r, c),
                   "x6": lambda c: CR.x6_geometry(r, c)}[what]
            full, one = geo(CR.CUS), geo(1)
            assert r.n == 3 and full["grid"] == full["items"] and one["grid"] == 2 and one["items"] // one["grid"] >= 4, (r, p)
            if what == "stream" and r.stride == 1:
                assert full["double_buffered"] and not one["double_buffered"]
            assert {geo(c)["grid"] for c in CR.CU_LIMITS} != {full["grid"]}
        elif what == "kern2":
            assert not CR.conv1x1_geometry(r, p)["kern2"] and all(CR.conv1x1_geometry(r, p, c)["kern2"] for c in CR.CU_LIMITS), (r, p)
        elif what == "nsplit":
            assert [CR.conv1x1_geometry(r, p, c)["nsplit"] for c in (CR.CUS,) + CR.CU_LIMITS] == [8, 1, 2, 3]
        else:
            assert len({CR.conv1x1_x6_geometry(r, c)["slices"] for c in (CR.CUS,) + CR.CU_LIMITS}) > 1, r
        assert CR.dispatch(r, p) != "none"
    for n, h, w in CR.SWEEP_BLOCKS:
        assert CR.block_geometry(n, h, w, 1)["items"] >= 4 and CR.block_geometry(n, h, w)["grid"] == CR.block_geometry(n, h, w)["items"]


def test_merged_groups_are_reordered_by_the_launcher():
    """Every 3x3 group: the members' steps are not in descending order as given, so the launcher's longest-first sort moves
    them (conv1x1_jobs keeps the given order: nothing to reorder there); no group exceeds its launcher's maximum."""
    for p, k, s, members in CR.group_cases():
        assert 2 <= len(members) <= CR.MAXJOBS[(p, k)]
        rows = [CR.member_row(m, k, s) for m in members]
        assert len({(r.cin, r.cout, r.h, r.w) for r in rows}) == len(rows)
        if k == 3 or p == 2:
            steps = CR.group_steps(rows, p)
            assert steps != sorted(steps, reverse=True), (CR.group_id((p, k, s, members)), steps)
        if k == 1 and p == 0:
            assert all(CR.pad(r.cin, 0) // 32 in (2, 4, 8) and not r.res for r in rows)


# ---------------------------------------------------------------------------------------------- coverage
def test_table_covers_every_reachable_kernel(lib):
    """The names esahrnet_op_conv_kernel (host only) returns over the table are the committed list of reachable names; every row
    is filed under the name its home precision gives it; the Python restatement of the dispatch agrees on every row in every
    precision; every row is served by at least one precision."""
    assert set(CR.TABLE) == set(CR.REACHABLE) == set(CR.PRECISION_OF) and not set(CR.REACHABLE) & set(CR.EXCLUDED)
    hit = set()
    for name, rows in CR.TABLE.items():
        for r in rows:
            assert _kernel(lib, r, CR.PRECISION_OF[name]) == name, (name, r)
    for r in CR.table_rows():
        names = {p: _kernel(lib, r, p) for p in (0, 1, 2, 3)}
        assert names == {p: CR.dispatch(r, p) for p in (0, 1, 2, 3)}, r
        assert any(v != "none" for v in names.values()), r
        hit |= set(names.values()) - {"none"}
    assert hit == set(CR.REACHABLE)
    assert {(r, p) for r, p, _ in CR.single_cases()} == {(r, p) for r in CR.table_rows() for p in (0, 1, 2, 3) if _kernel(lib, r, p) != "none"}


def test_table_has_the_chunk_counts_the_issue_lists():
    chunks = lambda name, p, unit: {CR.pad(r.cin, p) // unit for r in CR.TABLE[name]}
    assert chunks(CR.X6_C1, 2, 32) == set(CR.C1_X6_CHUNKS)
    assert chunks(CR.SB_1X1, 0, 32) == set(CR.C1_SB_CHUNKS)
    assert chunks(CR.BF_1X1, 1, 64) == set(CR.C1_16_BLOCKS) == chunks(CR.HF_1X1, 3, 64)
    assert any(CR.pad(r.cout, 0) >= 1024 and r.cin == 64 and (r.h, r.w) == (8, 8) for r in CR.TABLE[CR.SB_1X1])
    every = {CR.pad(r.cin, 0) // 32 for r in CR.table_rows()}
    assert {1, 2, 3, 4, 8, 15} <= every
    assert {CR.pad(r.cout, 0) for r in CR.table_rows()} >= {32, 64, 96, 128} and {8, 48} <= {r.cin for r in CR.table_rows()}
    assert {11, 16} <= {r.cout for r in CR.table_rows()} and {1, 2, 3} == {r.n for r in CR.table_rows()}
    assert {(7, 5), (16, 16), (17, 33), (20, 24), (17, 31), (34, 30)} <= {(r.h, r.w) for r in CR.table_rows()}


def test_excluded_names_stand_in_the_sources_and_nowhere_in_the_table(lib):
    src = ""
    for f in ("conv_mfma.hip", "conv_x6.hip"):
        with open(os.path.join(ROOT, "esa-pose-estimation_amd", "csrc", f)) as fh:
            src += fh.read()
    for name in list(CR.EXCLUDED) + list(CR.REACHABLE):
        assert f'"{name}"' in src or name.split("<")[0] in src, name
    assert re.search(r"#define S2_TH16 0", open(os.path.join(ROOT, "esa-pose-estimation_amd", "csrc", "conv_s2c32.hip")).read())
    assert _kernel(lib, R(1, 64, 64, 8, 8, k=1, res=True), 1) == "none"            # the 16-bit 1x1 has no residual form


def test_kernel_entry_refuses_on_the_host(lib):
    buf = C.create_string_buffer(8)
    assert lib.esahrnet_op_conv_kernel(1, 32, 32, 8, 8, 3, 1, 0, 4, buf, 8) != 0 and b"precision" in lib.esahrnet_last_error()
    assert lib.esahrnet_op_conv_kernel(1, 32, 32, 8, 8, 5, 1, 0, 0, buf, 8) != 0
    assert lib.esahrnet_op_conv_kernel(1, 32, 32, 8, 8, 3, 1, 0, 0, None, 8) != 0
    assert lib.esahrnet_debug_set_cu_limit(2) == 0 and lib.esahrnet_debug_set_cu_limit(0) == 0        # (host state only)


def test_entries_are_declared_and_abi_stays():
    from esa_pose_estimation_amd import _lib
    with open(os.path.join(ROOT, "include", "esahrnet.h")) as f:
        header = f.read()
    names = ("esahrnet_debug_set_cu_limit", "esahrnet_op_conv_kernel", "esahrnet_op_conv_group", "esahrnet_op_conv_multi",
             "esahrnet_op_block32", "esahrnet_op_stem2")
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for n in names:
        assert f"int {n}(" in header and n in _lib.exported_symbols() and f"`{n}(" in doc, n
    assert "test use only" in header[header.index("esahrnet_op_conv_kernel") - 1200:header.index("esahrnet_op_conv_kernel")]
    assert int(re.search(r"#define ESAHRNET_ABI_VERSION (\d+)", header).group(1)) == 6 == _lib.ABI_VERSION     # entries were only added
    with open(os.path.join(ROOT, "esa-pose-estimation_amd", "hrnet.py")) as f:
        assert not any(n in f.read() for n in names)                              # on no forward path
