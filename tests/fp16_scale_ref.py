"""Helpers of the fp16 scale tests — test code, never shipped.

  * checkpoints(sd, x): the golden state dict and crops moved out of fp16's range by powers of two, so that the fp32 reference
    of each is the committed golden times s EXACTLY (every operation of variant 0 commutes with a power of two):
      hot    crops, every `.bias` and every `running_mean` x 2^16: all activations and the heat-maps x 2^16        (s = 2^16)
      cold   the same with 2^-16                                                                                  (s = 2^-16)
      mixed  the same function as the golden: bn1.{weight, bias} x 2^k and conv2.weight x 2^-k in three blocks — k = 16 in
             layer1.1 and stage3.0.branches.1.0, k = -18 in stage4.0.branches.0.2; no single global factor cures it  (s = 1)
  * handle queries (groups, names, per-convolution ranges) through the C ABI;
  * rescale(sd, descs, convs, exps): the Python statement of what esahrnet_commit folds — BatchNorm weight and bias x 2^-e_out,
    the convolution's input channels x 2^e_in per range (a convolution without BatchNorm has e_out = 0: the output layer).
"""
import ctypes as C

import numpy as np
import torch

MIXED_BLOCKS = {"layer1.1": 16, "stage3.0.branches.1.0": 16, "stage4.0.branches.0.2": -18}
SCALE = {"plain": 1.0, "hot": 2.0 ** 16, "cold": 2.0 ** -16, "mixed": 1.0}


def checkpoints(sd, x):
    """-> {tag: (state dict, crops, s)}; the fp32 reference of a tag is the golden's x s."""
    out = {"plain": (sd, x, 1.0)}
    for tag in ("hot", "cold"):
        s = SCALE[tag]
        moved = {k: (v * s if k.endswith(".bias") or k.endswith(".running_mean") else v.clone()) for k, v in sd.items()}
        out[tag] = (moved, x * s, s)
    mixed = {k: v.clone() for k, v in sd.items()}
    for block, k in MIXED_BLOCKS.items():
        mixed[block + ".bn1.weight"] *= 2.0 ** k
        mixed[block + ".bn1.bias"] *= 2.0 ** k           # (the running mean is subtracted before the scale: untouched)
        mixed[block + ".conv2.weight"] *= 2.0 ** -k
    out["mixed"] = (mixed, x, 1.0)
    return out


def group_names(lib, h):
    g = C.c_int(-1)
    assert lib.esahrnet_scale_groups(h, C.byref(g)) == 0, lib.esahrnet_last_error()
    buf = C.create_string_buffer(96)
    names = []
    for i in range(g.value):
        assert lib.esahrnet_scale_group_name(h, i, buf, 96) == 0, lib.esahrnet_last_error()
        names.append(buf.value.decode())
    return names


def scale_convs(lib, L, h, descs):
    """{conv name: (out_group, [(c0, c1, in_group), ...])}"""
    out = {}
    for i, d in enumerate(descs):
        sc = L.ScaleConv()
        assert lib.esahrnet_scale_conv_get(h, i, C.byref(sc)) == 0, (d["name"], lib.esahrnet_last_error())
        out[d["name"]] = (sc.out_group, [(sc.c0[j], sc.c1[j], sc.in_group[j]) for j in range(sc.nranges)])
    return out


def ideal_exponents(tag, names, convs):
    """The exponents that undo a checkpoint of checkpoints() exactly: +-16 on every group (hot, cold); mixed: k on the group
    of each named block's conv1 output."""
    if tag in ("hot", "cold"):
        return [16 if tag == "hot" else -16] * len(names)
    e = [0] * len(names)
    if tag == "mixed":
        for block, k in MIXED_BLOCKS.items():
            e[convs[block + ".conv1"][0]] = k
    return e


def rescale(sd, descs, convs, exps):
    """The state dict whose plain folding is the library's folding of `sd` under exponents `exps`."""
    out = {k: v.clone() for k, v in sd.items()}
    ex = lambda g: exps[g] if g >= 0 else 0      # noqa: E731
    for d in descs:
        og, ranges = convs[d["name"]]
        if d["bn"]:
            out[d["bn"] + ".weight"] = out[d["bn"] + ".weight"] * 2.0 ** -ex(og)
            out[d["bn"] + ".bias"] = out[d["bn"] + ".bias"] * 2.0 ** -ex(og)
        else:
            assert og < 0, d["name"]            # only the output layer has no BatchNorm, and it writes the f32 heat-maps
        w = out[d["name"] + ".weight"]
        for c0, c1, g in ranges:
            w[:, c0:c1] = w[:, c0:c1] * 2.0 ** ex(g)
    return out


def arr32(values):
    return (C.c_int32 * len(values))(*[int(v) for v in values])


def fill_handle(lib, h, descs, sd):
    from esa_pose_estimation_amd.fold import fold_conv
    for i, d in enumerate(descs):
        w, b = fold_conv(sd, d["name"], d["bn"], d["has_bias"])
        assert lib.esahrnet_set_conv(h, i, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)) == 0


def scaled_conv(lib, h, i, d):
    w = np.empty((d["cout"], d["cin"], d["k"], d["k"]), dtype=np.float32)
    b = np.empty((d["cout"],), dtype=np.float32)
    assert lib.esahrnet_debug_scaled_conv(h, i, w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)) == 0, \
        lib.esahrnet_last_error()
    return w, b


def errors(y, g, s):
    """(L_inf, mean-abs, arg-max flips) of heat-maps y (numpy f32 [n,K,H,W], at scale s) against the golden fixture g, in
    units of the golden's scale (divided by s)."""
    sub = int(g["subsample"])
    d = np.abs(y[:, :, ::sub, ::sub].astype(np.float64) / s - g["out"])
    flips = int((y.reshape(*y.shape[:2], -1).argmax(-1) != g["plane_argmax"]).sum())
    return float(d.max()), float(d.mean()), flips


def as_torch(sd):
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))) for k, v in sd.items()}
