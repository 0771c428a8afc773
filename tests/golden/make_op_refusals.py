"""Writes op_refusals.json: what each call of the table below is refused with by ONE build of the library, the one given on the
command line — a build of the commit before the stand-alone operator entries left plan.hip.  The record is the reference of
tests/test_op_refusals_host.py; it is made once and regenerated only when a message is changed on purpose.  No GPU is needed:
a call that is not refused before its first HIP call does not belong here, and one that returns 0 stops the script.

    python tests/golden/make_op_refusals.py path/to/libesahrnet.so [out.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_op_refusals_host as T  # noqa: E402

BIG = 65536
# entry -> (the good call: (name, value) in the entry's order; the bad calls: overrides of it).  Pointers are offsets into the
# test's host buffer (test_op_refusals_host.py): 0 is aligned, 4 is not 8- or 16-byte aligned, 2 not 4-byte aligned.
CONV = (("x", 0), ("n", 1), ("cin", 32), ("h", 8), ("w", 8), ("wt", 0), ("b", 0), ("cout", 32), ("k", 3), ("stride", 1), ("relu", 0),
        ("res", None), ("y", 0))
CONV_BAD = [dict(x=None), dict(wt=None), dict(b=None), dict(y=None), dict(k=5), dict(k=1, stride=2), dict(k=3, stride=3), dict(k=3, stride=0),
            dict(y=None, k=5)]
FUSE = (("xs", [0, 0]), ("hs", [4, 2]), ("ws", [4, 2]), ("nterms", 2), ("n", 1), ("c", 32), ("h", 4), ("w", 4), ("relu", 0), ("y", 0))
FUSE_BAD = [dict(xs=None), dict(hs=None), dict(ws=None), dict(y=None), dict(nterms=0), dict(nterms=5)]
CBAM = (("x", 0), ("res", None), ("n", 1), ("c", 32), ("h", 8), ("w", 8), ("fc0", 0), ("fc2", 0), ("sa", 0), ("relu", 0), ("y", 0),
        ("cy", 32), ("c0", 0), ("fused", 0), ("p", 0))
CBAM_BAD = [dict(x=None), dict(fc0=None), dict(fc2=None), dict(sa=None), dict(y=None), dict(n=0), dict(h=0), dict(w=-1),
            dict(p=3), dict(p=-1), dict(c=8), dict(c=20), dict(c=0), dict(c=544, cy=544), dict(c=520, cy=520, p=1), dict(c0=-8),
            dict(c0=4), dict(c0=8), dict(cy=64, c0=40), dict(c=32, cy=32, p=1, c0=8), dict(c=96, cy=96, fused=1),
            dict(h=BIG, w=BIG), dict(n=3, h=BIG, w=16384), dict(p=3, c=8), dict(c=8, c0=4)]
STEPS = CBAM + (("slabs", 0), ("partial", None), ("ca", None), ("maps", None), ("s", None))
STEPS_BAD = CBAM_BAD + [dict(fused=1, maps=0), dict(slabs=-1), dict(slabs=65), dict(slabs=1025, h=64, w=64), dict(h=2, w=2, slabs=5)]
STEM = (("x", 0), ("n", 1), ("h", 8), ("w", 8), ("wt", 0), ("b", 0), ("relu", 0), ("pooled", 0), ("p", 0), ("y", 0), ("partial", None),
        ("slabs", None), ("s", None))
STEM_BAD = [dict(x=None), dict(wt=None), dict(b=None), dict(y=None), dict(n=0), dict(h=0), dict(w=0), dict(p=3), dict(p=-1),
            dict(h=8192, w=8192), dict(n=2, h=4096, w=4097), dict(pooled=1), dict(pooled=1, partial=0), dict(pooled=1, slabs=[-5]),
            dict(pooled=1, p=3), dict(pooled=1, n=0)]
RESAMPLE = (("x", 0), ("n", 1), ("c", 16), ("h", 4), ("w", 4), ("y", 0), ("cy", 64), ("c0", 8), ("H", 8), ("W", 8), ("align", 0),
            ("p", 0), ("s", None))
RESAMPLE_BAD = [dict(x=None), dict(y=None), dict(n=0), dict(c=0), dict(cy=0), dict(h=0), dict(w=0), dict(H=0), dict(W=0), dict(p=3),
                dict(p=-1), dict(c0=-8), dict(c0=4), dict(c0=56), dict(c=9, c0=56), dict(cy=65, c0=88, p=2),
                dict(cy=65, c0=120, p=1), dict(c0=4, p=3)]
ZERO = (("y", 0), ("n", 1), ("cy", 64), ("h", 4), ("w", 4), ("c0", 8), ("nchan", 16), ("p", 0), ("s", None))
ZERO_BAD = [dict(y=None), dict(n=0), dict(cy=0), dict(h=0), dict(w=0), dict(p=3), dict(p=-1), dict(c0=-8), dict(c0=4), dict(nchan=0),
            dict(nchan=12), dict(c0=56, nchan=16), dict(cy=65, c0=88, nchan=16, p=2), dict(cy=65, c0=120, nchan=16, p=1), dict(c0=64, nchan=8)]
KERNEL = (("n", 1), ("cin", 32), ("cout", 32), ("h", 8), ("w", 8), ("k", 3), ("stride", 1), ("res", 0), ("p", 0), ("out", 0), ("cap", 64))
DIMS_BAD = [dict(n=0), dict(cin=0), dict(cout=0), dict(h=0), dict(w=0), dict(k=5), dict(k=1, stride=2), dict(k=3, stride=3),
            dict(n=64, h=512, w=512), dict(n=1, h=2048, w=2048, cin=129)]
KERNEL_BAD = [dict(out=None), dict(cap=0), dict(p=4), dict(p=-1)] + DIMS_BAD
GROUP = (("count", 2), ("xs", [0, 0]), ("ns", [1, 1]), ("cins", [32, 32]), ("hs", [8, 8]), ("ws", [8, 8]), ("wts", [0, 0]), ("bs", [0, 0]),
         ("couts", [32, 32]), ("k", 3), ("stride", 1), ("relus", [0, 1]), ("res", None), ("ys", [0, 0]), ("p", 2), ("kernel", None),
         ("cap", 0), ("s", None))
GROUP_BAD = [dict(xs=None), dict(ns=None), dict(cins=None), dict(hs=None), dict(ws=None), dict(wts=None), dict(bs=None), dict(couts=None),
             dict(relus=None), dict(ys=None), dict(count=0), dict(count=7), dict(p=4), dict(p=-1), dict(xs=[0, None]), dict(wts=[None, 0]),
             dict(bs=[0, None]), dict(ys=[0, None]), dict(ns=[1, 0]), dict(cins=[0, 32]), dict(k=5), dict(k=1, stride=2),
             dict(hs=[8, BIG], ws=[8, BIG]),
             # no merged launch: the split format's stride-1 3x3 below the stream kernel's size, 1x1s of 32 input channels, 1x1s of
             # a 16-bit format; no kernel: a 16-bit 1x1 of 512 input channels
             dict(p=0), dict(k=1, p=0), dict(k=1, p=1, cins=[64, 64], couts=[64, 64]), dict(k=1, p=3, cins=[64, 64], couts=[64, 64]),
             dict(count=1, k=1, p=1, cins=[2048, 32], hs=[1, 8], ws=[1, 8])]
MULTI = (("x", 0), ("n", 1), ("cin", 32), ("h", 8), ("w", 8), ("nheads", 2), ("wts", [0, 0]), ("bs", [0, 0]), ("couts", [32, 64]),
         ("relus", [0, 1]), ("ys", [0, 0]), ("s", None))
MULTI_BAD = [dict(x=None), dict(wts=None), dict(bs=None), dict(couts=None), dict(relus=None), dict(ys=None), dict(nheads=1), dict(nheads=4),
             dict(wts=[0, None]), dict(bs=[None, 0]), dict(ys=[0, None]), dict(couts=[32, 48]), dict(couts=[0, 32]), dict(couts=[-32, 32]),
             dict(n=0), dict(cin=0), dict(h=0), dict(n=64, h=512, w=512)]
BLOCK = (("x", 0), ("n", 1), ("h", 8), ("w", 8), ("w1", 0), ("b1", 0), ("w2", 0), ("b2", 0), ("y", 0), ("s", None))
BLOCK_BAD = [dict(x=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(y=None), dict(n=0), dict(h=0), dict(w=0),
             dict(n=64, h=512, w=512)]
STEM2 = (("x", 0), ("n", 1), ("cin", 1), ("h", 8), ("w", 8), ("w1", 0), ("b1", 0), ("cmid", 64), ("w2", 0), ("b2", 0), ("cout", 64),
         ("p", 0), ("y", 0), ("s", None))
STEM2_BAD = [dict(x=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(y=None), dict(p=1), dict(p=3), dict(p=4),
             dict(p=-1), dict(cin=0), dict(cin=5), dict(cmid=0), dict(cmid=48), dict(n=0), dict(cout=0), dict(h=0), dict(n=64, h=512, w=512),
             dict(p=2, cin=2), dict(p=2, cmid=32), dict(p=2, cout=96)]
STEM_EX = (("x", 0), ("n", 1), ("cin", 1), ("h", 4), ("w", 4), ("wt", 0), ("b", 0), ("cout", 64), ("relu", 0), ("p", 0), ("y", 0), ("s", None))
STEM_EX_BAD = [dict(x=None), dict(wt=None), dict(b=None), dict(y=None), dict(p=4), dict(p=-1), dict(cin=0), dict(cin=5), dict(cout=48),
               dict(cout=0), dict(cout=32, p=1), dict(cout=96, p=3), dict(n=0), dict(h=0), dict(w=-1), dict(h=BIG, w=BIG)]
LAYOUT = (("dir", 0), ("x", 0), ("n", 1), ("c", 9), ("h", 4), ("w", 4), ("cp", 32), ("p", 0), ("raw", 0), ("y", 0), ("s", None))
LAYOUT_BAD = [dict(dir=2), dict(dir=-1), dict(x=None), dict(raw=None), dict(y=None), dict(dir=1, raw=None), dict(p=4), dict(p=-1), dict(n=0),
              dict(c=0), dict(h=0), dict(w=0), dict(cp=8), dict(cp=36), dict(h=BIG, w=BIG), dict(raw=4), dict(raw=8), dict(y=2), dict(x=2),
              dict(dir=1, x=None, raw=4)]
TILE = (("raw", 0), ("n", 1), ("c", 11), ("h", 4), ("w", 4), ("cp", 32), ("p", 0), ("store", 1), ("y", 0), ("part", 0), ("nt", [-5]),
        ("kp", None), ("idx", None), ("s", None))
TILE_BAD = [dict(raw=None), dict(part=None), dict(nt=None), dict(p=1), dict(p=3), dict(p=-1), dict(store=2), dict(store=-1), dict(y=None),
            dict(n=0), dict(h=0), dict(w=0), dict(c=0), dict(c=33, cp=64), dict(cp=8), dict(cp=36), dict(h=BIG, w=BIG), dict(raw=8),
            dict(part=4), dict(y=2), dict(kp=2), dict(idx=2), dict(store=0, y=2)]

TABLE = {
    "esahrnet_op_conv": (CONV + (("s", None),), CONV_BAD),
    "esahrnet_op_conv_ex": (CONV + (("p", 0), ("s", None)), CONV_BAD + [dict(p=4), dict(p=-1), dict(p=4, k=5)]),
    "esahrnet_op_fuse": (FUSE + (("s", None),), FUSE_BAD),
    "esahrnet_op_fuse_ex": (FUSE + (("p", 0), ("s", None)), FUSE_BAD + [dict(p=4), dict(p=-1), dict(p=4, nterms=0)]),
    "esahrnet_op_cbam": (CBAM + (("s", None),), CBAM_BAD),
    "esahrnet_op_cbam_steps": (STEPS, STEPS_BAD),
    "esahrnet_op_stem": (STEM, STEM_BAD),
    "esahrnet_op_resample": (RESAMPLE, RESAMPLE_BAD),
    "esahrnet_op_zero_slice": (ZERO, ZERO_BAD),
    "esahrnet_op_conv_kernel": (KERNEL, KERNEL_BAD),
    "esahrnet_op_conv_group": (GROUP, GROUP_BAD),
    "esahrnet_op_conv_multi": (MULTI, MULTI_BAD),
    "esahrnet_op_block32": (BLOCK, BLOCK_BAD),
    "esahrnet_op_stem2": (STEM2, STEM2_BAD),
    "esahrnet_op_stem_ex": (STEM_EX, STEM_EX_BAD),
    "esahrnet_op_layout": (LAYOUT, LAYOUT_BAD),
    "esahrnet_op_tile_max": (TILE, TILE_BAD),
}


def main(lib_path, out=os.path.join(HERE, "op_refusals.json")):
    from esa_pose_estimation_amd import _lib as L
    lib = L.load_other(lib_path)
    _raw, base = T.host_buffer()
    records = []
    for entry, (good, bads) in TABLE.items():
        names = [n for n, _ in good]
        for bad in bads:
            assert set(bad) <= set(names), (entry, bad)
            rec = {"entry": entry, "args": [bad.get(n, v) for n, v in good]}
            rc, msg, _ = T.refuse(lib, L._SIGS, rec, base)
            if rc == 0 or "hip" in msg or "launch" in msg.split(": ", 1)[1][:6]:
                raise SystemExit(f"{entry} {bad}: not refused on the host ({rc}, {msg!r})")
            records.append(dict(rec, error=msg))
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")
    print(f"{len(records)} refusals, {len({r['error'] for r in records})} distinct messages -> {out}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
