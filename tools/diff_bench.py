"""What the precision report costs, seg_hrnet2 W32, 256 x 256, batch 8, precision "fp16" and "bf16x3" against "fp32":
  (a) esahrnet_forward_diff against the two keep-mode forwards alone (esahrnet_forward under esahrnet_set_debug_keep(h, 1) on
      either handle, each in its own workspace): the difference is the scan of every compared row.  HIP events around a window
      of --steps calls.
  (b) esahrnet_tensor_diff on a pair of tensors of the shape and formats of the largest compared row, at batch 8 and at a batch
      that makes the reference side 1 GiB: GB/s of bytes read, both operands counted.
  (c) for the named taps only, the way there was before — net.taps(x) on both nets, then torch reductions of every pair (the
      maxima, the sums in f64, the counts) and one copy to the host — against net.precision_report(x, reference=ref), which
      reports those rows and every other.  Wall clock per call, synchronised.
The forms of a group are timed in alternation, --reps windows each after a warm-up; per form the median window and the
[min, max] spread.  One JSON line per precision, appended to --out (default profiles/diff_bench.jsonl).  Each precision runs in
a child process of its own under `timeout`, and the first one that fails ends the run.

    python tools/diff_bench.py [--steps 20] [--reps 7] [--precisions fp16,bf16x3] [--out FILE]"""
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


def torch_diff(ta, tb):
    """The figures of a record from the f32 NCHW taps of both nets with torch, per crop, one copy to the host."""
    import torch
    rows = []
    for k, a in ta.items():
        if k not in tb or tb[k].shape != a.shape:
            continue
        a, b = a.reshape(a.shape[0], -1), tb[k].reshape(a.shape[0], -1)
        both = torch.isfinite(a) & torch.isfinite(b)
        z = torch.zeros_like(a)
        err = torch.where(both, (a - b).abs(), z)
        bz = torch.where(both, b, z)
        rows.append(torch.stack([err.double().sum(1), (err.double() ** 2).sum(1), (bz.double() ** 2).sum(1), err.amax(1).double(),
                                 bz.abs().amax(1).double(), torch.where(both, a, z).abs().amax(1).double(), err.argmax(1).double(),
                                 both.sum(1).double(), (~torch.isfinite(a)).sum(1).double(), (~torch.isfinite(b)).sum(1).double()], 1))
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
        raise SystemExit("diff_bench needs a GPU")
    lib = _lib.lib()
    x = synth.make_crops(N, 1, HW, HW, seed=0).cuda()
    nets = []
    for p in (prec, "fp32"):
        net = seg_hrnet2.get_seg_model(config.make_config(widths=WIDTHS), precision=p)
        net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0, gain=0.5), strict=True)
        nets.append(net.cuda().eval().freeze_weights())
    net, ref = nets
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
        rep = net.precision_report(x, reference=ref)
        h, hr = net._rt._handle_for(net, x.device), ref._rt._handle_for(ref, x.device)
        # (a) on the handles, with the keep state set once so that no form re-plans
        for hh in (h, hr):
            _lib.check(lib.esahrnet_set_debug_keep(hh, 1))
        need, na, nb = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _lib.check(lib.esahrnet_forward_diff_workspace_bytes(h, hr, N, HW, HW, C.byref(need)))
        _lib.check(lib.esahrnet_workspace_bytes(h, N, HW, HW, C.byref(na)))
        _lib.check(lib.esahrnet_workspace_bytes(hr, N, HW, HW, C.byref(nb)))
        ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
        ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
        off_b = (na.value + 255) // 256 * 256
        heat = torch.empty((2, N, net.num_keypoints, HW, HW), dtype=torch.float32, device="cuda")
        rec = torch.empty((len(rep.keys), N, 64), dtype=torch.uint8, device="cuda")

        def two_forwards():
            _lib.check(lib.esahrnet_forward(h, x.data_ptr(), N, HW, HW, heat[0].data_ptr(), ws_ptr, na.value, stream))
            _lib.check(lib.esahrnet_forward(hr, x.data_ptr(), N, HW, HW, heat[1].data_ptr(), ws_ptr + off_b, nb.value, stream))
        forms_a = {
            "keep_forwards": two_forwards,
            "forward_diff": lambda: _lib.check(lib.esahrnet_forward_diff(h, hr, x.data_ptr(), N, HW, HW, heat[0].data_ptr(),
                                                                         heat[1].data_ptr(), ws_ptr, need.value, rec.data_ptr(), stream)),
        }
        for f in forms_a.values():
            for _ in range(5):
                f()
        a = windows(forms_a, reps, events)
        for hh in (h, hr):
            _lib.check(lib.esahrnet_set_debug_keep(hh, 0))
        # (b) the largest compared row (by the bytes of both operands), as raw tensors of small positive values
        def row_bytes(d):
            return d.h * d.w * (d.c * FMT_BYTES[d.fmt] + d.c * 4)
        big = max((d for d, c in zip(rep.descs[:-1], rep.compared[:-1]) if c), key=row_bytes)
        c, th, tw, fmt = big.c, big.h, big.w, big.fmt
        cpa = (c + 63) // 64 * 64 if fmt in (1, 3) else (c + 31) // 32 * 32
        cpb = (c + 31) // 32 * 32
        img_a, img_b = th * tw * cpa * FMT_BYTES[fmt], th * tw * cpb * 4
        b = {}
        for tag, n in (("b8", N), ("1gib", max(N, (1 << 30) // img_b))):
            ta = torch.zeros(n * img_a, dtype=torch.uint8, device="cuda")
            tb = torch.zeros(n * img_b, dtype=torch.uint8, device="cuda")
            ta.view(torch.int16).random_(0, 0x3C00)          # positive finite values in every format
            tb.view(torch.int16).random_(0, 0x3C00)
            wsb = C.c_size_t()
            _lib.check(lib.esahrnet_tensor_diff_workspace_bytes(fmt, cpa, 2, cpb, n, c, th, tw, C.byref(wsb)))
            pw = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
            out_rec = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
            f = lambda: _lib.check(lib.esahrnet_tensor_diff(ta.data_ptr(), fmt, cpa, tb.data_ptr(), 2, cpb, 0, n, c, th, tw,  # noqa: E731
                                                            pw.data_ptr(), wsb.value, out_rec.data_ptr(), stream))
            for _ in range(5):
                f()
            med, spread = windows({"scan": f}, reps, events)["scan"]
            real = n * th * tw * ((c + 7) // 8 * 8) * (FMT_BYTES[fmt] + 4)          # the groups with a real channel, both sides
            b[tag] = dict(batch=n, bytes=real, ms=med, spread=spread, gb_per_s=real / med / 1e6,
                          values_per_s=n * th * tw * c / med * 1e3)
            del ta, tb
        # (c) the named taps: the way there was against the report
        forms_c = {"taps_torch": lambda: torch_diff(net.taps(x), ref.taps(x)),
                   "precision_report": lambda: net.precision_report(x, reference=ref)}
        for f in forms_c.values():
            for _ in range(3):
                f()
        cc = windows(forms_c, reps, wall)
    row = {"bench": "diff", "workload": f"hrnet2_w32_{HW}_b{N}", "precision": prec, "reference": "fp32", "steps": steps, "reps": reps,
           "box": platform.node(), "device": torch.cuda.get_device_name(0),
           "rows": len(rep.keys), "rows_compared": int(rep.compared.sum()), "taps": len(net.taps(x)),
           "largest": dict(key=big.key.decode(), shape=[c, th, tw], format=_lib.STATS_FORMATS[fmt], scan=b)}
    for k, (med, spread) in {**a, **cc}.items():
        row[f"{k}_ms"] = med
        row[f"{k}_spread"] = spread
    row["scan_cost_ms"] = row["forward_diff_ms"] - row["keep_forwards_ms"]
    row["precision_report_over_taps_torch"] = row["precision_report_ms"] / row["taps_torch_ms"]
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--precisions", default="fp16,bf16x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diff_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_precision(a.child, a.steps, a.reps, a.out)
    for prec in a.precisions.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", prec,
               "--steps", str(a.steps), "--reps", str(a.reps), "--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc:                          # a fault, an abort, a time limit: nothing more is started on the GPU
            raise SystemExit(f"diff_bench: precision {prec} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
