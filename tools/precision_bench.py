"""Step time of the two single-pass modes side by side: precision="bf16" against precision="fp16" (DESIGN §3c), same
commit, same run, seg_hrnet2:
  w32_256_b32    HRNet-W32, 256 x 256, batch 32
  w48_384_b64    HRNet-W48, 384 x 384, batch 64
each as eager forwards and as one graph replay.  The four forms of a workload (bf16 / fp16 x eager / graph) are timed in
alternation, --reps windows of --steps forwards each after a warm-up, HIP events around a window; per form the median window
and the [min, max] spread, ms per forward.  One JSON line per workload, appended to --out (default
profiles/fp16_bench.jsonl).

Each workload runs in a child process of its own under `timeout`, one after the other, and the first one that fails ends
the run (`&&`): nothing more is started on a GPU after a fault or a hang.

    python tools/precision_bench.py [--steps 30] [--reps 7] [--workloads w32_256_b32,w48_384_b64] [--out FILE]"""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"w32_256_b32": ((32, 64, 128, 256), 256, 32), "w48_384_b64": ((48, 96, 192, 384), 384, 64)}
STEP_TIMEOUT_S = 420        # per workload: build two nets, capture two graphs, 4 forms x reps x steps forwards


def run_workload(name, steps, reps, out):
    import torch
    from esa_pose_estimation_amd import config, seg_hrnet2, synth
    if not torch.cuda.is_available():
        raise SystemExit("precision_bench needs a GPU")
    widths, hw, n = WORKLOADS[name]
    x = synth.make_crops(n, 1, hw, hw, seed=0).cuda()
    nets, graphs, outs, forms = {}, {}, {}, {}
    with torch.no_grad():
        for prec in ("bf16", "fp16"):
            net = seg_hrnet2.get_seg_model(config.make_config(widths=widths), precision=prec)
            net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0), strict=True)
            nets[prec] = net.cuda().eval().freeze_weights()
            ref = nets[prec](x)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                nets[prec](x)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs[prec] = nets[prec](x)
            graphs[prec] = g
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(outs[prec], ref), prec               # a replay computes what the eager forward computes
            forms[f"{prec}_eager"] = (lambda net=nets[prec]: net(x))
            forms[f"{prec}_graph"] = g.replay
        for f in forms.values():                                    # warm-up of every form
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(reps):
            for k, f in forms.items():                              # alternating: the forms share whatever the box is doing
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(steps):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / steps)
    row = {"bench": "precision", "workload": f"hrnet2_{name}", "batch": n, "steps": steps, "reps": reps,
           "box": platform.node(), "device": torch.cuda.get_device_name(0), "launches": nets["fp16"].launch_count(),
           "gflop_per_crop": nets["fp16"].flops_per_crop(hw, hw) / 1e9}
    for k in forms:
        row[f"{k}_ms"] = statistics.median(ms[k])
        row[f"{k}_spread"] = [min(ms[k]), max(ms[k])]
    for form in ("eager", "graph"):
        row[f"fp16_over_bf16_{form}"] = row[f"fp16_{form}_ms"] / row[f"bf16_{form}_ms"]
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp16_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return run_workload(a.child, a.steps, a.reps, a.out)
    for name in a.workloads.split(","):
        if name not in WORKLOADS:
            raise SystemExit(f"unknown workload {name!r}: {sorted(WORKLOADS)}")
    for name in a.workloads.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", name,
               "--steps", str(a.steps), "--reps", str(a.reps), "--out", a.out]
        rc = subprocess.run(cmd).returncode
        if rc:                          # a fault, an abort, a time limit: nothing more is started on the GPU
            raise SystemExit(f"precision_bench: workload {name} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
