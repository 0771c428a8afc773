"""Cost of the Gaussian-fit decoder fused into the forward: seg_hrnet2 and seg_hrnet3, W32, 256 x 256 crops, batch 32,
precision="fp32", synthetic weights and crops.  Per network three forms, each a sequence of C calls on one stream:
  u   esahrnet_forward + esahrnet_keypoints_gaussfit through another build of the library (--parent-lib: the parent commit's
      libesahrnet.so), the yardstick; left out when no library is given
  u2  the same two calls through this build: must equal u within u's spread, the existing calls have not changed
  f   esahrnet_forward_keypoints_gaussfit: no heat-map tensor (2 x n * K * H * W * 4 bytes less traffic than u)
The forms are timed in alternation, --reps windows of --steps calls each after a warm-up, HIP events around each window; per
form the median window and the [min, max] spread, in microseconds per call.  The fused outputs are compared with the unfused
ones bit for bit before anything is timed.  One JSON line per network, appended to --out (default
profiles/gaussfit_fwd_bench.jsonl).

    python tools/gaussfit_fwd_bench.py [--steps 10] [--reps 7] [--n 32] [--size 256] [--nets seg_hrnet2,seg_hrnet3]
                                       [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--nets", default="seg_hrnet2,seg_hrnet3")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussfit_fwd_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from esa_pose_estimation_amd import _lib, config, seg_hrnet2, seg_hrnet3, synth
    if not torch.cuda.is_available():
        raise SystemExit("gaussfit_fwd_bench needs a GPU")
    mods = {"seg_hrnet2": seg_hrnet2, "seg_hrnet3": seg_hrnet3}
    n, s = a.n, a.size
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def make_net(name, lib_path=None):
        net = mods[name].get_seg_model(config.make_config(), precision="fp32")
        net.load_state_dict(synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0), strict=True)
        if lib_path:                                            # this net's runtime talks to another build of the library
            net._rt.use_library(_lib.load_other(lib_path))
        return net.cuda().eval().freeze_weights()

    def ok(lib, rc):
        if rc:
            raise RuntimeError(lib.esahrnet_last_error().decode(errors="replace"))

    def scratch(lib, h, query):
        nb = C.c_size_t()
        ok(lib, query(h, n, s, s, C.byref(nb)))
        t = torch.empty(nb.value + 256, dtype=torch.uint8, device=dev)
        return t, t.data_ptr() + (-t.data_ptr()) % 256, nb.value

    for name in a.nets.split(","):
        x = synth.make_crops(n, 1, s, s, seed=0).cuda()
        nets = {"u2": make_net(name)}
        if a.parent_lib:
            nets["u"] = make_net(name, a.parent_lib)
        k = nets["u2"].num_keypoints
        heat = torch.empty((n, k, s, s), dtype=torch.float32, device=dev)
        outs = {f: (torch.empty((n, k, 3), dtype=torch.float32, device=dev), torch.empty((n, k), dtype=torch.int32, device=dev),
                    torch.empty((n, k, 8), dtype=torch.float64, device=dev), torch.empty((n, k), dtype=torch.int32, device=dev),
                    torch.empty((n, k, 3), dtype=torch.float64, device=dev)) for f in ("u", "u2", "f")}
        forms, keep = {}, []
        for f, net in nets.items():
            lib, h = net._rt.lib, net._rt._handle_for(net, dev)
            ws = scratch(lib, h, lib.esahrnet_workspace_bytes)
            keep.append(ws)

            def unfused(lib=lib, h=h, ws=ws, o=outs[f]):
                ok(lib, lib.esahrnet_forward(h, x.data_ptr(), n, s, s, heat.data_ptr(), ws[1], ws[2], stream))
                ok(lib, lib.esahrnet_keypoints_gaussfit(heat.data_ptr(), n, k, s, s, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                        o[3].data_ptr(), o[4].data_ptr(), stream))
            forms[f] = unfused
        lib, h = nets["u2"]._rt.lib, nets["u2"]._rt._handle_for(nets["u2"], dev)
        wsf = scratch(lib, h, lib.esahrnet_keypoints_gaussfit_forward_workspace_bytes)

        def fused(o=outs["f"]):
            ok(lib, lib.esahrnet_forward_keypoints_gaussfit(h, x.data_ptr(), n, s, s, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                                            o[3].data_ptr(), o[4].data_ptr(), wsf[1], wsf[2], stream))
        forms["f"] = fused
        forms = {f: forms[f] for f in ("u", "u2", "f") if f in forms}
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        view = lambda t: t.view({4: torch.int32, 8: torch.int64}[t.element_size()])      # noqa: E731
        same = {f: all(torch.equal(view(p), view(q)) for p, q in zip(outs[f], outs["u2"])) for f in forms if f != "u2"}
        us = {f: [] for f in forms}
        for _ in range(a.reps):
            for f, fn in forms.items():                                 # alternating: the forms share whatever the box is doing
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                e1.synchronize()
                us[f].append(e0.elapsed_time(e1) * 1e3 / a.steps)
        row = {"bench": "gaussfit_fwd", "workload": f"{name}_w32_{s}_b{n}_fp32", "steps": a.steps, "reps": a.reps, "box": platform.node(),
               "device": torch.cuda.get_device_name(0), "status_counts": torch.bincount(outs["f"][3].flatten(), minlength=4).tolist(),
               "heat_bytes": n * k * s * s * 4, "bit_identical_to_u2": same}
        for f in forms:
            row[f"{f}_us"] = statistics.median(us[f])
            row[f"{f}_spread"] = [min(us[f]), max(us[f])]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del nets, forms, keep, heat, outs


if __name__ == "__main__":
    main()
