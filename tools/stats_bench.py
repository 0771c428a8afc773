"""What the activation range report costs, seg_hrnet2 W32, 256 x 256, batch 8, precision "fp32" and "fp16":
  (a) esahrnet_forward_stats against the keep-mode forward alone (esahrnet_forward under esahrnet_set_debug_keep(h, 1)): the
      difference is the scan of every tensor of the plan.  HIP events around a window of --steps calls.
  (b) esahrnet_tensor_stats on a tensor of the shape and format of the plan's largest one, at batch 8 (it fits the Infinity
      Cache) and at a batch that makes it 1 GiB (it does not): GB/s of bytes read.
  (c) for the named taps only, the way there was before — net.taps(x), then torch reductions of every tap (abs().amax(), min,
      max, isfinite, isnan, the fp16 counts, an f64 sum) and one copy to the host — against net.activation_stats(x), which
      reports those rows and every other.  Wall clock per call, synchronised.
The forms of a group are timed in alternation, --reps windows each after a warm-up; per form the median window and the
[min, max] spread.  One JSON line per precision, appended to --out (default profiles/stats_bench.jsonl).  Each precision runs
in a child process of its own under `timeout`, and the first one that fails ends the run.

    python tools/stats_bench.py [--steps 20] [--reps 7] [--precisions fp32,fp16] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS, HW, N = (32, 64, 128, 256), 256, 8
STEP_TIMEOUT_S = 420
FMT_BYTES = {0: 4, 1: 2, 2: 4, 3: 2}        # bytes per stored channel


def torch_stats(taps):
    """The figures of a record from f32 NCHW taps with torch, per crop, one copy to the host."""
    import torch
    rows = []
    for t in taps.values():
        v = t.reshape(t.shape[0], -1)
        fin = torch.isfinite(v)
        a = torch.where(fin, v.abs(), torch.zeros_like(v))
        rows.append(torch.stack([a.amax(1).double(), torch.where(fin, v, torch.full_like(v, float("inf"))).amin(1).double(),
                                 torch.where(fin, v, torch.full_like(v, float("-inf"))).amax(1).double(), a.double().sum(1),
                                 fin.sum(1).double(), torch.isnan(v).sum(1).double(), torch.isinf(v).sum(1).double(),
                                 ((a == 0) & fin).sum(1).double(), (a >= 65504).sum(1).double(),
                                 ((a > 0) & (a < 2.0 ** -14)).sum(1).double()], 1))
    return torch.stack(rows).cpu()


def windows(forms, reps, run):
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():              # alternating: the forms share whatever the box is doing
            ms[k].append(run(f))
    return {k: (statistics.median(v), [min(v), max(v)]) for k, v in ms.items()}


def run_precision(prec, steps, reps, out):
    import torch
    from esa_pose_estimation_amd import _lib, config, seg_hrnet2, synth
    if not torch.cuda.is_available():
        raise SystemExit("stats_bench needs a GPU")
    lib = _lib.lib()
    x = synth.make_crops(N, 1, HW, HW, seed=0).cuda()
    net = seg_hrnet2.get_seg_model(config.make_config(widths=WIDTHS), precision=prec)
    net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0, gain=0.5), strict=True)
    net = net.cuda().eval().freeze_weights()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def events(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    with torch.no_grad():
        st = net.activation_stats(x)
        h = net._rt._handle_for(net, x.device)
        # (a) on the handle, with the keep state set once so that neither form re-plans
        _lib.check(lib.esahrnet_set_debug_keep(h, 1))
        need = C.c_size_t()
        _lib.check(lib.esahrnet_forward_stats_workspace_bytes(h, N, HW, HW, C.byref(need)))
        ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
        ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
        heat = torch.empty((N, net.num_keypoints, HW, HW), dtype=torch.float32, device="cuda")
        rec = torch.empty((len(st.rows), N, 64), dtype=torch.uint8, device="cuda")
        forms_a = {
            "keep_forward": lambda: _lib.check(lib.esahrnet_forward(h, x.data_ptr(), N, HW, HW, heat.data_ptr(), ws_ptr, need.value, stream)),
            "forward_stats": lambda: _lib.check(lib.esahrnet_forward_stats(h, x.data_ptr(), N, HW, HW, heat.data_ptr(), ws_ptr,
                                                                           need.value, rec.data_ptr(), stream)),
        }
        for f in forms_a.values():
            for _ in range(5):
                f()
        a = windows(forms_a, reps, events)
        _lib.check(lib.esahrnet_set_debug_keep(h, 0))
        # (b) the largest scanned tensor of the plan, as a raw tensor of random bytes' worth of small values
        fmt_code = {v: k for k, v in _lib.STATS_FORMATS.items()}
        big = max((r for r in st.rows[:-1] if r["scanned"]),
                  key=lambda r: r["shape"][1] * r["shape"][2] * r["shape"][0] * FMT_BYTES[fmt_code[r["format"]]])
        fmt = fmt_code[big["format"]]
        c, th, tw = big["shape"]
        cp = (c + 63) // 64 * 64 if fmt in (1, 3) else (c + 31) // 32 * 32
        img_bytes = th * tw * cp * FMT_BYTES[fmt]
        b = {}
        for tag, n in (("b8", N), ("1gib", max(N, (1 << 30) // img_bytes))):
            t = torch.zeros(n * img_bytes, dtype=torch.uint8, device="cuda")
            t.view(torch.int16).random_(0, 0x3C00)          # positive finite values in every format
            wsb = C.c_size_t()
            _lib.check(lib.esahrnet_tensor_stats_workspace_bytes(fmt, n, c, cp, th, tw, C.byref(wsb)))
            pw = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
            out_rec = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
            f = lambda: _lib.check(lib.esahrnet_tensor_stats(t.data_ptr(), fmt, n, c, cp, th, tw, pw.data_ptr(), wsb.value,  # noqa: E731
                                                             out_rec.data_ptr(), stream))
            for _ in range(5):
                f()
            med, spread = windows({"scan": f}, reps, events)["scan"]
            b[tag] = dict(batch=n, bytes=n * img_bytes, ms=med, spread=spread, gb_per_s=n * img_bytes / med / 1e6)
            del t
        # (c) the named taps: the way there was against the report
        forms_c = {"taps_torch": lambda: torch_stats(net.taps(x)), "activation_stats": lambda: net.activation_stats(x)}
        for f in forms_c.values():
            for _ in range(3):
                f()
        cc = windows(forms_c, reps, wall)
    row = {"bench": "stats", "workload": f"hrnet2_w32_{HW}_b{N}", "precision": prec, "steps": steps, "reps": reps,
           "box": platform.node(), "device": torch.cuda.get_device_name(0), "launches": net.launch_count(),
           "rows": len(st.rows), "rows_scanned": sum(r["scanned"] for r in st.rows), "taps": len(net.taps(x)),
           "largest": dict(name=big["name"], shape=big["shape"], format=big["format"], scan=b)}
    for k, (med, spread) in {**a, **cc}.items():
        row[f"{k}_ms"] = med
        row[f"{k}_spread"] = spread
    row["scan_cost_ms"] = row["forward_stats_ms"] - row["keep_forward_ms"]
    row["activation_stats_over_taps_torch"] = row["activation_stats_ms"] / row["taps_torch_ms"]
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--precisions", default="fp32,fp16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_precision(a.child, a.steps, a.reps, a.out)
    for prec in a.precisions.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", prec,
               "--steps", str(a.steps), "--reps", str(a.reps), "--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc:                          # a fault, an abort, a time limit: nothing more is started on the GPU
            raise SystemExit(f"stats_bench: precision {prec} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
