"""Cost of the Gaussian-fit decoder on 32 x 11 x 256 x 256 f32 heat-maps (one rotated anisotropic blob per plane, 1 % noise):
  g  esahrnet_keypoints_gaussfit (arg-max sweep, then one wave per plane fitting its 13 x 13 window), all outputs
  h  esahrnet_keypoints_final2_hess, the decoder whose Hessian it replaces, through this build of the library
  p  the same call through another build of the library (--parent-lib: the parent commit's libesahrnet.so), when given: the
     yardstick the issue names, and a check that the existing call did not change
The forms are timed in alternation, --reps windows of --steps calls each after a warm-up, HIP events around each window; per
form the median window and the [min, max] spread, in microseconds per call.  One JSON line, appended to --out (default
profiles/gaussfit_bench.jsonl), with the number of planes per status (status_counts[0]: accepted).

    python tools/gaussfit_bench.py [--steps 50] [--reps 7] [--n 32] [--k 11] [--size 256] [--parent-lib FILE] [--out FILE]"""
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussfit_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from esa_pose_estimation_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("gaussfit_bench needs a GPU")
    lib = _lib.lib()
    parent = _lib.load_other(a.parent_lib) if a.parent_lib else None
    n, k, s = a.n, a.k, a.size
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda lo, hi: torch.rand((n, k, 1, 1), device="cuda", generator=g) * (hi - lo) + lo      # noqa: E731
    cx, cy, sx, sy, th = rnd(8, s - 9), rnd(8, s - 9), rnd(1.5, 3.5), rnd(1.5, 3.5), rnd(0, 3.14159)
    yy, xx = torch.meshgrid(torch.arange(s, device="cuda", dtype=torch.float32), torch.arange(s, device="cuda", dtype=torch.float32),
                            indexing="ij")
    u = torch.cos(th) * (xx - cx) + torch.sin(th) * (yy - cy)
    v = -torch.sin(th) * (xx - cx) + torch.cos(th) * (yy - cy)
    heat = (torch.exp(-0.5 * ((u / sx) ** 2 + (v / sy) ** 2)) + 0.01 * torch.randn((n, k, s, s), device="cuda", generator=g)).contiguous()
    del u, v
    kp = torch.empty((n, k, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    fit = torch.empty((n, k, 8), dtype=torch.float64, device="cuda")
    status = torch.empty((n, k), dtype=torch.int32, device="cuda")
    hess = torch.empty((n, k, 3), dtype=torch.float64, device="cuda")
    kp2, idx2, hess2 = torch.empty_like(kp), torch.empty_like(idx), torch.empty_like(hess)
    nbytes = C.c_size_t()
    _lib.check(lib.esahrnet_keypoints_final2_workspace_bytes(n, k, s, s, C.byref(nbytes)))
    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device="cuda")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def gaussfit():
        _lib.check(lib.esahrnet_keypoints_gaussfit(heat.data_ptr(), n, k, s, s, kp.data_ptr(), idx.data_ptr(), fit.data_ptr(),
                                                   status.data_ptr(), hess.data_ptr(), stream))

    def final2_hess(l=lib):
        if l.esahrnet_keypoints_final2_hess(heat.data_ptr(), n, k, s, s, kp2.data_ptr(), idx2.data_ptr(), hess2.data_ptr(), ws_ptr,
                                            nbytes.value, stream):
            raise RuntimeError(l.esahrnet_last_error().decode(errors="replace"))

    forms = {"g": gaussfit, "h": final2_hess}
    if parent is not None:
        forms["p"] = lambda: final2_hess(parent)
    for f in forms.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    same = None
    if parent is not None:
        final2_hess()
        a_kp, a_h = kp2.clone(), hess2.clone()
        final2_hess(parent)
        torch.cuda.synchronize()
        same = bool(torch.equal(a_kp.view(torch.int32), kp2.view(torch.int32)) and torch.equal(a_h.view(torch.int64), hess2.view(torch.int64)))
    us = {f: [] for f in forms}
    for _ in range(a.reps):
        for name, f in forms.items():                               # alternating: the forms share whatever the box is doing
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                f()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    row = {"bench": "gaussfit", "workload": f"heat_{n}x{k}x{s}x{s}_f32_blobs", "steps": a.steps, "reps": a.reps, "box": platform.node(),
           "device": torch.cuda.get_device_name(0), "status_counts": torch.bincount(status.flatten(), minlength=4).tolist(),
           "parent_bit_identical": same}
    for name in forms:
        row[f"{name}_us"] = statistics.median(us[name])
        row[f"{name}_spread"] = [min(us[name]), max(us[name])]
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
