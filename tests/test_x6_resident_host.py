"""CPU: ESAHRNET_X6_RELOAD_WEIGHTS chooses between two bodies INSIDE the same kernels (conv_x6.hip: weights resident in registers
or reloaded every step).  It must not show in the plan: the same launches, names, FLOP and byte figures with and without it."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_op_descs", os.path.join(ROOT, "tests", "golden", "make_op_descs.py"))
make_op_descs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_op_descs)


def test_the_switch_changes_no_op_description(monkeypatch):
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        monkeypatch.delenv(k)
    combo = ("seg_hrnet2", "fp32", make_op_descs.W32)
    default = make_op_descs.op_descs(*combo)
    for value in ("1", "0"):
        got = make_op_descs.op_descs(*combo, (("X6_RELOAD_WEIGHTS", value),))
        assert got
        for shape, rows in got.items():
            assert rows == default[shape], (value, shape)
            assert any(r[1] == "conv_x6_kernel<3, 1, 2, 4, 4, 2, 2>" for r in rows) and any(r[1] == "conv_x6_jobs_kernel<3, 1>" for r in rows)


def test_the_grid_limit_hook_and_the_switch_are_declared_and_documented():
    from esa_pose_estimation_amd import _lib
    header = open(os.path.join(ROOT, "include", "esahrnet.h")).read()
    assert re.search(r"\bint\s+esahrnet_debug_set_x6_grid_limit\s*\(\s*int\s+workgroups\s*\)", header)
    assert "esahrnet_debug_set_x6_grid_limit" in _lib.exported_symbols()
    lib = _lib.lib()
    assert lib.esahrnet_debug_set_x6_grid_limit(3) == 0 and lib.esahrnet_debug_set_x6_grid_limit(0) == 0      # (host state only)
    assert "`ESAHRNET_X6_RELOAD_WEIGHTS=1`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
