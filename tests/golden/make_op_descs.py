#!/usr/bin/env python3
"""Generate tests/golden/op_descs.json.gz: what esahrnet_op_desc_get says about every launch of the forward plan.

    python tests/golden/make_op_descs.py

For each (variant, precision, widths) in COMBOS and each (n, h, w) in SHAPES it records (rc, kernel, label,
flops, bytes) of every op index of the net's uncommitted probe handle.  Needs no GPU.  bench.py's roofline
leg and the GPU tests read these descriptions, so tests/test_host_cpu.py pins them to this fixture: a change
of dispatch rule that changes them shows up on the host.  The ESAHRNET_* switches are cleared first
(esahrnet_create reads them).  The JSON, one op per line, is stored gzip-compressed with a zero time stamp, so that
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
          + [(v, "bf16", W32) for v in ("seg_hrnet", "seg_hrnet2")]          # bf16 is built for variant 0 only
          + [("seg_hrnet2", p, W48) for p in ("bf16", "bf16x3")])
SHAPES = [(32, 256, 256), (1, 256, 256), (2, 96, 64), (64, 384, 384)]


def combo_key(variant, precision, widths):
    return f"{variant}/{precision}/w{widths[0]}"


def clear_env():
    for k in [k for k in os.environ if k.startswith("ESAHRNET_")]:
        del os.environ[k]


def op_descs(variant, precision, widths):
    """{"n,h,w": [[rc, kernel, label, flops, bytes], ...]} for one net."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: the library shares torch's HIP runtime, see _lib.lib)
    from esa_pose_estimation_amd import _lib, config
    mod = importlib.import_module(f"esa_pose_estimation_amd.{variant}")
    net = mod.get_seg_model(config.make_config(widths=widths), precision=precision)
    rt = net._rt
    out = {}
    for n, h, w in SHAPES:
        rows = []
        for i in range(rt.launch_count()):
            d = _lib.OpDesc()
            rc = rt.lib.esahrnet_op_desc_get(rt._probe, i, n, h, w, C.byref(d))
            rows.append([rc, d.kernel.decode(), d.label.decode(), d.flops, d.bytes])
        out[f"{n},{h},{w}"] = rows
    return out


def main():
    clear_env()
    res = {combo_key(*c): op_descs(*c) for c in COMBOS}
    with open(OUT, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:   # one op per line
        f.write(("{\n" + ",\n".join(
            f"{json.dumps(c)}: {{\n" + ",\n".join(
                f"{json.dumps(s)}: [\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]" for s, rows in v.items())
            + "\n}" for c, v in res.items()) + "\n}\n").encode())
    print(f"wrote {OUT}: {sum(len(r) for v in res.values() for r in v.values())} descriptions")


if __name__ == "__main__":
    main()
