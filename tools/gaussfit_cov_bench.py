"""Cost of the covariance pass of the Gaussian-fit decoder on 32 x 11 x 256 x 256 f32 heat-maps (one rotated anisotropic blob per
plane, 1 % noise; the workload of tools/gaussfit_bench.py):
  c  esahrnet_keypoints_gaussfit_cov with cov_dev and info_dev: the fit, one more Jacobian pass, an undamped 7 x 7 factorisation
     and two pairs of triangular solves per plane
  z  the same entry with both pointers NULL: it must launch the sibling's kernels
  g  esahrnet_keypoints_gaussfit, the sibling, through this build of the library
  p  the sibling through another build of the library (--parent-lib: the parent commit's libesahrnet.so), when given: the
     yardstick, and a check that the existing call did not change
The forms are timed in alternation, --reps windows of --steps calls each after a warm-up, HIP events around each window; per
form the median window and the [min, max] spread, in microseconds per call.  One JSON line, appended to --out (default
profiles/gaussfit_cov_bench.jsonl), with the number of planes per status and how many have a finite cov / info.

    python tools/gaussfit_cov_bench.py [--steps 50] [--reps 7] [--n 32] [--k 11] [--size 256] [--parent-lib FILE] [--out FILE]"""
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
    ap.add_argument("--cov-floor", type=float, default=1e-6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussfit_cov_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from esa_pose_estimation_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("gaussfit_cov_bench needs a GPU")
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

    def outputs():
        return dict(kp=torch.empty((n, k, 3), dtype=torch.float32, device="cuda"), idx=torch.empty((n, k), dtype=torch.int32, device="cuda"),
                    fit=torch.empty((n, k, 8), dtype=torch.float64, device="cuda"), status=torch.empty((n, k), dtype=torch.int32, device="cuda"),
                    hess=torch.empty((n, k, 3), dtype=torch.float64, device="cuda"))

    oc, oz, og, op = outputs(), outputs(), outputs(), outputs()
    cov = torch.empty((n, k, 3), dtype=torch.float64, device="cuda")
    info = torch.empty((n, k, 3), dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def with_cov(o, cv, nf):
        _lib.check(lib.esahrnet_keypoints_gaussfit_cov(heat.data_ptr(), n, k, s, s, o["kp"].data_ptr(), o["idx"].data_ptr(),
                                                       o["fit"].data_ptr(), o["status"].data_ptr(), o["hess"].data_ptr(), cv, nf,
                                                       a.cov_floor, stream))

    def sibling(l, o):
        if l.esahrnet_keypoints_gaussfit(heat.data_ptr(), n, k, s, s, o["kp"].data_ptr(), o["idx"].data_ptr(), o["fit"].data_ptr(),
                                         o["status"].data_ptr(), o["hess"].data_ptr(), stream):
            raise RuntimeError(l.esahrnet_last_error().decode(errors="replace"))

    forms = {"c": lambda: with_cov(oc, cov.data_ptr(), info.data_ptr()), "z": lambda: with_cov(oz, None, None),
             "g": lambda: sibling(lib, og)}
    if parent is not None:
        forms["p"] = lambda: sibling(parent, op)
    for f in forms.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()

    def same(x, y):
        return all(bool(torch.equal(x[m].view(torch.uint8), y[m].view(torch.uint8))) for m in x)

    same_fit = same(oc, og) and same(oz, og)
    same_parent = same(og, op) if parent is not None else None
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
    row = {"bench": "gaussfit_cov", "workload": f"heat_{n}x{k}x{s}x{s}_f32_blobs", "steps": a.steps, "reps": a.reps, "box": platform.node(),
           "device": torch.cuda.get_device_name(0), "status_counts": torch.bincount(oc["status"].flatten(), minlength=4).tolist(),
           "finite_cov": int(torch.isfinite(cov).all(-1).sum()), "finite_info": int(torch.isfinite(info).all(-1).sum()),
           "median_cxx": float(cov[..., 0].nanmedian()), "fit_outputs_bit_identical": same_fit, "parent_bit_identical": same_parent}
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
