"""Cost of handing keypoints to the pose solver, W32 256 x 256 seg_hrnet2 fp32, gray 1920 x 1200 frames, at batch 1 and 32:
  a  net.frames_to_keypoints, one device->host copy of its packed outputs, then the host selection per image
     (inference.select_keypoints + crop_to_image: what pipeline.estimate_poses(device_loader=True) leaves to the host).
  b  net.frames_to_correspondences (include/esahrnet.h esahrnet_frames_correspondences) and one device->host copy of the
     correspondence record: nothing left to do on the host before the solver.
  k  net.frames_to_keypoints alone, no copy: the existing call, through this build of the library.
  p  the same call through another build of the library (--parent-lib: the parent commit's libesahrnet.so), when given: shows
     whether the existing call changed.
Neither a nor b includes the solver.  The forms are timed in alternation, --reps windows of --steps steps each after a
warm-up; per form the median window and the [min, max] spread, ms per step: *_ms from HIP events around the window, *_wall_ms
from the host clock around the window and a synchronise (a and b end on the host, so the wall clock is their figure).  One JSON
line per batch size, appended to --out (default profiles/correspond_bench.jsonl); its "refine" field names the decoder of the
row (default get_final2: the decoder whose Hessian the "hessian" weights need).

    python tools/correspond_bench.py [--steps 50] [--reps 7] [--batches 1,32] [--refine get_final2] [--parent-lib FILE] [--out FILE]"""
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
    ap.add_argument("--refine", default="get_final2", choices=("get_final", "get_final2"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correspond_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from esa_pose_estimation_amd import _lib, config, inference, seg_hrnet2, synth
    if not torch.cuda.is_available():
        raise SystemExit("correspond_bench needs a GPU")

    def make_net(lib_path=None):
        net = seg_hrnet2.get_seg_model(config.make_config(), precision="fp32")
        net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0), strict=True)
        if lib_path:                                            # this net's runtime talks to another build of the library
            net._rt.use_library(_lib.load_other(lib_path))
        return net.cuda().eval().freeze_weights()

    net = make_net()
    parent = make_net(a.parent_lib) if a.parent_lib else None
    thresh, min_k = 0.8, 8
    for n in [int(v) for v in a.batches.split(",")]:
        scene = synth.make_scene(n, net.num_keypoints, seed=0)
        frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(n, 1200, 1920), dtype=np.uint8)).cuda()
        det = torch.tensor(scene["bboxes"], dtype=torch.int32, device="cuda")

        def host_select():
            v = net._loader(inference.LoaderRequest(a.refine), frames, det, None, 256, "val", None, 0.229, None).host("keypoints")
            rates, kp, boxes = v["rates"], v["kp"], v["boxes"]
            rec = []
            for i in range(n):
                idxs = inference.select_keypoints(kp[i, :, 2], thresh, min_k)
                ori = inference.crop_to_image(kp[i, :, :2].astype(np.float64), float(rates[i]), int(boxes[i, 0]), int(boxes[i, 1]))
                rec.append((idxs, ori[idxs], kp[i, idxs, 2]))
            return rec

        def device_select():
            request = inference.LoaderRequest(a.refine, None, None, (thresh, min_k, "peak"))
            v = net._loader(request, frames, det, None, 256, "val", None, 0.229, None).host("correspondences")
            return v["count"], v["order"], v["pts"], v["w"]

        def keypoints_only(m=net):
            return m.frames_to_keypoints(frames, det, scale=256, refine=a.refine)[0]

        forms = {"a": host_select, "b": device_select, "k": keypoints_only}
        if parent is not None:
            forms["p"] = lambda: keypoints_only(parent)
        with torch.no_grad():
            for f in forms.values():                                # warm-up of every form
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            rec, (count, order, pts, w) = host_select(), device_select()
            same = all(count[i] == len(rec[i][0]) and order[i, :count[i]].tolist() == list(rec[i][0]) and
                       np.array_equal(pts[i, :count[i]].view(np.int64), np.ascontiguousarray(rec[i][1]).view(np.int64))
                       for i in range(n))
            if parent is not None:
                same = same and bool(torch.equal(keypoints_only().view(torch.int32), keypoints_only(parent).view(torch.int32)))
            ms = {f: [] for f in forms}
            wall = {f: [] for f in forms}
            for _ in range(a.reps):
                for name, f in forms.items():                       # alternating: the forms share whatever the box is doing
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
        row = {"bench": "correspond", "workload": f"hrnet2_w32_256_b{n}_fp32_gray1920x1200", "batch": n, "refine": a.refine,
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


if __name__ == "__main__":
    main()
