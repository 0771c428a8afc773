"""The refusals of the seventeen stand-alone operator entries (csrc/op_abi.hip: esahrnet_op_conv .. esahrnet_op_tile_max) that
come before the first HIP call.  Every call of tests/golden/op_refusals.json must return non-zero with, byte for byte, the
message recorded there, and leave every buffer it was given as it was.  The record was written by
tests/golden/make_op_refusals.py from the library built BEFORE the entries moved out of plan.hip onto esa::Format, DevScope
and finish: equality with a record, not with a formula, so a slip in a `who` prefix, in a format's padding or in the order of
two checks fails.  No GPU: nothing here reaches a HIP function.

A record is data: {"entry", "args", "error"}.  An argument is a number; null; for a pointer parameter a byte offset into one
64-byte aligned host buffer of floats (so 0 is aligned and 4 is not); for a parameter that is an array of ints a list of
numbers, for one that is an array of pointers a list of offsets and nulls (how _lib binds the entry decides which).

Not covered, because no machine without a device reaches them: every "<who>: hipMalloc failed", upload's
"hipMalloc(...)" / "hipMemcpy(...)" texts, "<who>: launch failed: ...", "op_conv_group: layout conversion failed: ...",
"op_cbam: copying a step's output: ...", "op_stem: copying the partials: ...", the "<who>: <sync error>" of finish, and
"op_conv_multi: launch_conv_s2c32_multi does not serve these heads" (asked after the buffers are allocated).  Not reachable at
all: "op_stem: launch_stem_pool does not serve H x W" (stem_pool_slabs serves every positive H and W at cin 1, cout 64).
Every other refusal line of the file is in the record at least once."""
import ctypes as C
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_refusals.json")
ENTRIES = ("esahrnet_op_conv", "esahrnet_op_conv_ex", "esahrnet_op_fuse", "esahrnet_op_fuse_ex", "esahrnet_op_cbam",
           "esahrnet_op_cbam_steps", "esahrnet_op_stem", "esahrnet_op_resample", "esahrnet_op_zero_slice", "esahrnet_op_conv_kernel",
           "esahrnet_op_conv_group", "esahrnet_op_conv_multi", "esahrnet_op_block32", "esahrnet_op_stem2", "esahrnet_op_stem_ex",
           "esahrnet_op_layout", "esahrnet_op_tile_max")
FLOATS, FILL = 4096, 7.0


def host_buffer():
    """(keep-alive, 64-byte aligned address) of FLOATS floats, all FILL."""
    raw = (C.c_float * (FLOATS + 16))(*([FILL] * (FLOATS + 16)))
    return raw, (C.addressof(raw) + 63) & ~63


def refuse(lib, sigs, rec, base):
    """Makes the call of `rec`; returns (return code, message, the int arrays passed with what they held before)."""
    ints = []

    def arg(t, v):
        if v is None or t in (C.c_int, C.c_size_t):
            return v
        if t is C.c_void_p:
            return C.c_void_p(base + v)
        if t is C.c_char_p:
            return C.cast(base + v, C.c_char_p)
        if t is C.POINTER(C.c_int):
            ints.append(((C.c_int * len(v))(*v), v))
            return ints[-1][0]
        assert t is C.POINTER(C.c_void_p), t
        return (C.c_void_p * len(v))(*[None if e is None else base + e for e in v])

    types = sigs[rec["entry"]][1]
    assert len(types) == len(rec["args"]), rec
    rc = getattr(lib, rec["entry"])(*[arg(t, v) for t, v in zip(types, rec["args"])])
    return rc, lib.esahrnet_last_error().decode(), ints


def test_every_entry_refuses_as_recorded():
    from esa_pose_estimation_amd import _lib
    lib = _lib.lib()
    with open(GOLDEN) as f:
        records = json.load(f)
    assert {r["entry"] for r in records} == set(ENTRIES)
    assert len(records) == 290 and len({r["error"] for r in records}) == 161
    raw, base = host_buffer()
    for r in records:
        rc, msg, ints = refuse(lib, _lib._SIGS, r, base)
        assert rc != 0 and msg == r["error"], (r, msg)
        assert all(list(a) == v for a, v in ints), r
    assert all(v == FILL for v in raw)                                          # outputs untouched
