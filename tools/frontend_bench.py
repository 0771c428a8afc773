"""Cost of the loader in front of the forward, W32 256 x 256 seg_hrnet2 fp32, gray 1920 x 1200 frames, at batch 1 and 32:
  a  the host loader: crops.crop_batch (Python box rule, blocking upload of the boxes, crop kernel) -> net(x, output="keypoints"),
     eager.  a_ms: HIP events around the step; a_wall_ms: host clock around the step and a synchronise (what a caller waits).
  b  net.frames_to_keypoints (include/esahrnet.h esahrnet_frames_keypoints), eager, boxes already on the device.
  c  the same call as one graph replay.
The three are timed in alternation, --reps windows of --steps steps each after a warm-up; per form the median window and the
[min, max] spread, ms per step.  One JSON line per batch size, appended to --out (default profiles/frontend_bench.jsonl).

    python tools/frontend_bench.py [--steps 50] [--reps 7] [--batches 1,32] [--out FILE]"""
import argparse
import json
import os
import platform
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from esa_pose_estimation_amd import config, crops, seg_hrnet2, synth
    if not torch.cuda.is_available():
        raise SystemExit("frontend_bench needs a GPU")
    net = seg_hrnet2.get_seg_model(config.make_config(), precision="fp32")
    net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0), strict=True)
    net = net.cuda().eval().freeze_weights()
    for n in [int(v) for v in a.batches.split(",")]:
        scene = synth.make_scene(n, net.num_keypoints, seed=0)
        boxes = scene["bboxes"]
        frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(n, 1200, 1920), dtype=np.uint8)).cuda()
        det = torch.tensor(boxes, dtype=torch.int32, device="cuda")

        def host_loader():
            x, _, _ = crops.crop_batch(frames, boxes, 256)
            return net(x, output="keypoints")

        def one_call():
            return net.frames_to_keypoints(frames, det, scale=256)[0]

        with torch.no_grad():
            ref = host_loader()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                one_call()
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                kpg = one_call()
            forms = {"a": host_loader, "b": one_call, "c": g.replay}
            for f in forms.values():                                # warm-up of every form
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            same = bool(torch.equal(one_call().view(torch.int32), ref.view(torch.int32)) and
                        torch.equal(kpg.view(torch.int32), ref.view(torch.int32)))
            ms = {k: [] for k in forms}
            wall = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, f in forms.items():                          # alternating: the forms share whatever the box is doing
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    for _ in range(a.steps):
                        f()
                    e1.record()
                    e1.synchronize()
                    wall[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
                    ms[k].append(e0.elapsed_time(e1) / a.steps)
        row = {"bench": "frontend", "workload": f"hrnet2_w32_256_b{n}_fp32_gray1920x1200", "batch": n, "steps": a.steps,
               "reps": a.reps, "box": platform.node(), "device": torch.cuda.get_device_name(0), "bit_identical": same}
        for k in forms:
            row[f"{k}_ms"] = statistics.median(ms[k])
            row[f"{k}_spread"] = [min(ms[k]), max(ms[k])]
            row[f"{k}_wall_ms"] = statistics.median(wall[k])
            row[f"{k}_wall_spread"] = [min(wall[k]), max(wall[k])]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del g, kpg


if __name__ == "__main__":
    main()
