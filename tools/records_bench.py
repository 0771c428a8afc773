"""What the exchange of the packed records costs on ONE GPU (world size 1 under the nccl backend: the all-gather moves a rank's
block to itself, the kernel copies the record once), W32 256 x 256 seg_hrnet2 fp32, gray 1920 x 1200 frames, at batch 1 and 32:
  n  net.frames_to_correspondences: the single-device call, no exchange.
  s  parallel.sharded_frames_to_correspondences: the same call, then two all_gather_into_tensor of uint8 and two launches of
     gather_records_kernel (the correspondence record and the keypoint record).
  g  the two kernel launches alone, on blocks that are already gathered (parallel.gather_records_device).
This is the overhead a single process pays for going through the sharded entry point; it says NOTHING about more than one GPU,
where the all-gather crosses the fabric.  The forms are timed in alternation, --reps windows of --steps steps each after a
warm-up; per form the median window and the [min, max] spread, ms per step, from HIP events around the window (*_ms) and from the
host clock around the window and a synchronise (*_wall_ms).  One JSON line per batch size, appended to --out.

    python tools/records_bench.py [--steps 50] [--reps 7] [--batches 1,32] [--refine get_final2] [--out FILE]"""
import argparse
import json
import os
import platform
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--refine", default="get_final2", choices=("get_final", "get_final2", "gaussfit"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records_world1_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.distributed as dist
    from esa_pose_estimation_amd import config, inference, parallel, seg_hrnet2, synth
    if not torch.cuda.is_available():
        raise SystemExit("records_bench needs a GPU")
    net = seg_hrnet2.get_seg_model(config.make_config(), precision="fp32")
    net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0), strict=True)
    net = net.cuda().eval().freeze_weights()
    k = net.num_keypoints
    weights = "peak" if a.refine == "get_final" else "hessian"
    kw = dict(scale=256, refine=a.refine, thresh=0.8, min_k=8, weights=weights)
    cfields = inference.record_fields(k, "correspondences")
    kfields = inference.record_fields(k, "keypoints", a.refine == "gaussfit")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(s.getsockname()[1])
    s.close()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for n in [int(v) for v in a.batches.split(",")]:
            scene = synth.make_scene(n, k, seed=0)
            frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(n, 1200, 1920), dtype=np.uint8)).cuda()
            det = torch.tensor(scene["bboxes"], dtype=torch.int32, device="cuda")
            with torch.no_grad():
                whole = net._loader(inference.LoaderRequest(a.refine, None, None, (0.8, 8, weights)), frames, det, None, 256, "val",
                                    None, 0.229, None)
            whole = (whole.records["correspondences"][0], whole.records["keypoints"][0])
            blocks = (whole[0].clone(), whole[1].clone())           # world size 1: a block is the record

            def gather_only():
                return (parallel.gather_records_device(blocks[0], 1, n, cfields), parallel.gather_records_device(blocks[1], 1, n, kfields))

            forms = {"n": lambda: net.frames_to_correspondences(frames, det, **kw),
                     "s": lambda: parallel.sharded_frames_to_correspondences(net, frames, det, **kw),
                     "g": gather_only}
            with torch.no_grad():
                for f in forms.values():
                    for _ in range(5):
                        f()
                torch.cuda.synchronize()
                same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(forms["n"](), forms["s"]()))
                same = same and torch.equal(gather_only()[0], whole[0]) and torch.equal(gather_only()[1], whole[1])
                ms = {f: [] for f in forms}
                wall = {f: [] for f in forms}
                for _ in range(a.reps):
                    for name, f in forms.items():                   # alternating: the forms share whatever the box is doing
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        e0.record()
                        for _ in range(a.steps):
                            f()
                        e1.record()
                        e1.synchronize()
                        wall[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
                        ms[name].append(e0.elapsed_time(e1) / a.steps)
            row = {"bench": "records_world1", "workload": f"hrnet2_w32_256_b{n}_fp32_gray1920x1200", "batch": n, "refine": a.refine,
                   "world": 1, "backend": dist.get_backend(), "record_bytes_per_crop": [sum(b for _, b in cfields), sum(b for _, b in kfields)],
                   "steps": a.steps, "reps": a.reps, "box": platform.node(), "device": torch.cuda.get_device_name(0),
                   "bit_identical": bool(same)}
            for name in forms:
                row[f"{name}_ms"] = statistics.median(ms[name])
                row[f"{name}_spread"] = [min(ms[name]), max(ms[name])]
                row[f"{name}_wall_ms"] = statistics.median(wall[name])
                row[f"{name}_wall_spread"] = [min(wall[name]), max(wall[name])]
            line = json.dumps(row)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
