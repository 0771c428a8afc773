#!/usr/bin/env python3
"""Generate tests/golden/op_descs.json.gz: what esahrnet_op_desc_get says about every launch of the forward plan.

    python tests/golden/make_op_descs.py

For each (variant, precision, widths) in COMBOS and each (n, h, w) in SHAPES it records (rc, kernel, label,
flops, bytes) of every op index of the net's uncommitted probe handle.  Needs no GPU.  bench.py's roofline
leg and the GPU tests read these descriptions, so tests/test_host_cpu.py pins them to this fixture: a change
of dispatch rule that changes them shows up on the host.  The ESAHRNET_* switches are cleared first
(esahrnet_create reads them).  An entry may carry plan switches of its own (SWITCHED, at SWITCH_SHAPES): each must
change its descriptions, else it is refused here.  SCHEDULE records the (wave, lane) of every op of one plan
under ESAHRNET_STREAMS=4.  The JSON, one op per line, is stored gzip-compressed with a zero time stamp, so that
the same descriptions give the same bytes."""
import ctypes as C
import gzip
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "op_descs.json.gz")
W32, W48 = (32, 64, 128, 256), (48, 96, 192, 384)
COMBOS = ([(v, p, W32) for v in ("seg_hrnet", "seg_hrnet2", "seg_hrnet3") for p in ("fp32", "bf16x3")]
          + [(v, "bf16", W32) for v in ("seg_hrnet", "seg_hrnet2")]
          + [("seg_hrnet2", p, W48) for p in ("bf16", "bf16x3")]
          + [("seg_hrnet3", "bf16", w) for w in (W32, W48)])
SHAPES = [(32, 256, 256), (1, 256, 256), (2, 96, 64), (64, 384, 384)]
# one entry per plan switch that changes the op list, on a net where it does (switches: ((name without ESAHRNET_, value),))
SWITCHED = ([("seg_hrnet2", "bf16x3", W32, ((s, "1"),))
             for s in ("NO_JOBS", "NO_MULTIHEAD", "NO_BBLOCK", "UNFUSED", "HEAD_V1")]
            + [("seg_hrnet3", "fp32", W32, ((s, "1"),))
               for s in ("HEAD3_DIRECT", "HEAD3_COUT32", "STEM_POOL_SEPARATE", "CBAM_UNFUSED", "NO_CBAM_JOBS")]
            + [("seg_hrnet2", "bf16", W32, (("BF_UNFUSED_HEAD", "1"),))]
            + [("seg_hrnet2", "fp32", W32, ((s, "1"),)) for s in ("X6_UNFUSED_HEAD", "X6_UNFUSED_STEM")]
            + [("seg_hrnet3", "fp32", W32, (("X6_UNFUSED_STEM", "1"),))])
SWITCH_SHAPES = [(32, 256, 256), (2, 96, 64)]
SCHEDULE = ("seg_hrnet2", "fp32", W32, (("STREAMS", "4"),))


def combo_key(variant, precision, widths, switches=()):
    return f"{variant}/{precision}/w{widths[0]}" + "".join(f" {k}={v}" for k, v in switches)


def clear_env():
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        del os.environ[k]


def _probe(variant, precision, widths, switches):
    """The net's runtime; its probe handle is created with `switches` set (and only those)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: the library shares torch's HIP runtime, see _lib.lib)
    from esa_pose_estimation_amd import config
    mod = importlib.import_module(f"esa_pose_estimation_amd.{variant}")
    saved = {k: os.environ.pop(k) for k in [k for k in os.environ if k.startswith("ESAHRNET_")]}
    try:
        os.environ.update({"ESAHRNET_" + k: v for k, v in switches})
        return mod.get_seg_model(config.make_config(widths=widths), precision=precision)._rt
    finally:
        clear_env()
        os.environ.update(saved)


def op_descs(variant, precision, widths, switches=()):
    """{"n,h,w": [[rc, kernel, label, flops, bytes], ...]} for one net."""
    rt = _probe(variant, precision, widths, switches)
    from esa_pose_estimation_amd import _lib
    out = {}
    for n, h, w in SWITCH_SHAPES if switches else SHAPES:
        rows = []
        for i in range(rt.launch_count()):
            d = _lib.OpDesc()
            rc = rt.lib.esahrnet_op_desc_get(rt._probe, i, n, h, w, C.byref(d))
            rows.append([rc, d.kernel.decode(), d.label.decode(), d.flops, d.bytes])
        out[f"{n},{h},{w}"] = rows
    return out


def op_schedule(variant, precision, widths, switches=()):
    """{"schedule": [[wave, lane], ...]} of every op of one net."""
    rt = _probe(variant, precision, widths, switches)
    rows = []
    for i in range(rt.launch_count()):
        wave, lane = C.c_int(), C.c_int()
        rc = rt.lib.esahrnet_debug_op_schedule(rt._probe, i, C.byref(wave), C.byref(lane))
        assert rc == 0, rt.lib.esahrnet_last_error().decode()
        rows.append([wave.value, lane.value])
    return {"schedule": rows}


def main():
    clear_env()
    res = {combo_key(*c): op_descs(*c) for c in COMBOS}
    for c in SWITCHED:
        got = op_descs(*c)
        default = op_descs(*c[:3])
        assert any(got[s] != default[s] for s in got), f"{combo_key(*c)} describes the same launches as the default plan"
        res[combo_key(*c)] = got
    res[combo_key(*SCHEDULE)] = op_schedule(*SCHEDULE)
    assert any(lane for _, lane in res[combo_key(*SCHEDULE)]["schedule"]), "the schedule has no side lane"
    with open(OUT, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:   # one op per line
        f.write(("{\n" + ",\n".join(
            f"{json.dumps(c)}: {{\n" + ",\n".join(
                f"{json.dumps(s)}: [\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]" for s, rows in v.items())
            + "\n}" for c, v in res.items()) + "\n}\n").encode())
    print(f"wrote {OUT}: {sum(len(r) for v in res.values() for r in v.values())} descriptions")


if __name__ == "__main__":
    main()
