"""Which precision can a checkpoint afford?  One forward of a network on a few crops with net.activation_stats:
the range of every tensor of the plan, scanned on the device where the forward left it.

Prints the table (one row per tensor of the plan in plan order, then the heat-maps), the fp16 headroom
(65504 / the largest stored |value|), the rows that hold a finite |value| >= 65504 or a NaN / infinity, and max|heat-map|.

    python tools/range_report.py [--net seg_hrnet2] [--widths 32,64,128,256] [--precision fp32] [--state-dict FILE.pth]
                                 [--crops FILE.npy | --size 256 --batch 4] [--gain 0.5] [--calibrate [--headroom-bits 3]]

Without --state-dict the synthetic weights of synth.make_state_dict (gain --gain) are used; without --crops, synthetic
normalised crops.  A crops file holds f32 [n, cin, h, w], already normalised as the network expects them.

--calibrate (precision fp16 only): first net.calibrate_fp16 on the crops and its table — one exponent per scale
group, the largest stored and true magnitude of each —; the report that follows is the calibrated net's, whose rows are the
STORED values (true value x 2^-exponent)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# DESIGN §3a′, quoted: the only threshold this tool mentions
BF16X3_STATEMENT = ("DESIGN §3a′: the relative error of precision=\"bf16x3\" \"is flat at 1–3 × 10⁻⁵ of the heat-map scale …, "
                    "i.e. it reaches the 1e-3 absolute tolerance when max|out| ≈ 40–50\"")
NETS = {"seg_hrnet": (3, 32), "seg_hrnet2": (1, 11), "seg_hrnet3": (1, 30)}        # module -> (cin, keypoints)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="seg_hrnet2", choices=sorted(NETS))
    ap.add_argument("--widths", default="32,64,128,256")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16x3", "bf16", "fp16"])
    ap.add_argument("--state-dict", default=None)
    ap.add_argument("--gain", type=float, default=0.5)
    ap.add_argument("--crops", default=None)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--calibrate", action="store_true")
    ap.add_argument("--headroom-bits", type=int, default=3)
    a = ap.parse_args()
    if a.calibrate and a.precision != "fp16":
        raise SystemExit("--calibrate belongs to --precision fp16")
    import importlib

    import numpy as np
    import torch
    from esa_pose_estimation_amd import config, synth
    if not torch.cuda.is_available():
        raise SystemExit("range_report needs a GPU: the scan runs where the forward runs")
    module = importlib.import_module(f"esa_pose_estimation_amd.{a.net}")
    net = module.get_seg_model(config.make_config(widths=tuple(int(v) for v in a.widths.split(","))), precision=a.precision)
    if a.state_dict:
        sd = torch.load(a.state_dict, map_location="cpu")
        sd = sd.get("state_dict", sd)
    else:
        sd = synth.make_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed=0, gain=a.gain)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    cin = NETS[a.net][0]
    x = torch.from_numpy(np.load(a.crops).astype(np.float32)) if a.crops else synth.make_crops(a.batch, cin, a.size, a.size, seed=0)
    with torch.no_grad():
        if a.calibrate:
            cal = net.calibrate_fp16(x.cuda(), headroom_bits=a.headroom_bits)
            print(cal.table())
            print()
        st = net.activation_stats(x.cuda())
    print(st.table())
    print()
    print(f"{a.net} {a.widths} precision={a.precision}: {len(st.rows)} rows, {len(st.scanned())} scanned, "
          f"{tuple(x.shape)} crops")
    print(f"fp16 headroom (65504 / largest stored |value|): {st.headroom_fp16():.4g}")
    sat = st.saturated()
    word = "saturated stores (a genuine 65504 cannot be told apart)" if a.precision == "fp16" else "values fp16 would clamp"
    print(f"rows with finite |value| >= 65504, {word}: {len(sat)}")
    for r in sat:
        print(f"    {r['name']:<44} {r['n_ge_f16max']:>10} of {r['n_finite']}")
    bad = [r for r in st.scanned() if r["n_nan"] + r["n_inf"] > 0]
    print(f"rows with a NaN or an infinity: {len(bad)}" + (f" (first in plan order: {st.first_nonfinite()})" if bad else ""))
    for r in bad:
        print(f"    {r['name']:<44} nan {r['n_nan']:>10}  inf {r['n_inf']:>10}")
    print(f"max|heat-map| = {st.rows[-1]['max_abs']:.4g}")
    print(BF16X3_STATEMENT)


if __name__ == "__main__":
    main()
