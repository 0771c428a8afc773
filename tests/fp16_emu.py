"""CPU emulation of the single-pass fp16 mode (esahrnet_cfg.precision = 3) — test helper, never shipped.

Two restatements, both nothing but roundings put on an existing oracle:

  * forward(sd, cfg, x): the recipe that sized the mode before it was built — weights and every stored tensor rounded
    once to fp16, f32 accumulation — applied through oracle.emulate_split_bf16.forward, whose Emu class and rounding
    function are replaced for the duration of the call (what oracle/emulate_precisions.py does for its table).  Its
    distance to the real reference's fp32 output is the yardstick of the GPU tests: EMU_LINF / EMU_MEAN below.
  * forward_plan(sd, cfg, x, taps): the plan's own rounding points (conv1 in f32 on the f32 crop, bias in the branch-0
    slice of last_layer[0], ...) through oracle.emulate_bf16.forward with its rounding function replaced; it keeps the
    intermediates the library's taps() exposes and handles every stage table.

The rounding is f32 -> IEEE binary16, round to nearest even, SATURATED at +-65504 (the kernels never store an inf),
subnormals kept — q16 below.
"""
from __future__ import annotations

import contextlib
import threading

import torch
import torch.nn.functional as F

import oracle.emulate_bf16 as EB
import oracle.emulate_split_bf16 as ES

F16_MAX = 65504.0
_lock = threading.Lock()
# The f32 sums of the emulation depend on how torch cuts a convolution over its threads, and through ~90 layers of fp16
# rounding boundaries the figures below move by up to 4 % with that (w32_hrnet2_128 mean-abs: 9.21e-5 on one thread,
# 9.06e-5 on four, 8.96e-5 on sixteen).  The yardstick is therefore taken at a fixed thread count.
EMU_THREADS = 4


def q16(t: torch.Tensor) -> torch.Tensor:
    """f32 -> fp16 (nearest even) -> f32, +-inf of the conversion replaced by +-65504.  A NaN stays a NaN here (torch.clamp
    propagates it), where sb.h's pack2_f16 stores +65504: the one class on which the two differ (tests/layout_ref.py
    F16_NAN_STORE); no tensor of a forward with finite weights and crops holds one."""
    return t.to(torch.float16).to(torch.float32).clamp(-F16_MAX, F16_MAX)


class _Emu16:
    """oracle.emulate_split_bf16.Emu with one fp16 rounding per operand and per stored result, f32 accumulate."""

    def __init__(self, sd, terms=3):
        self.sd = sd

    def conv(self, name, bn, x, stride=1, relu=False, res=None):
        sd = self.sd
        w = sd[name + ".weight"].double()
        b = sd.get(name + ".bias")
        b = torch.zeros(w.shape[0], dtype=torch.float64) if b is None else b.double()
        if bn:
            g = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
            w = w * g[:, None, None, None]
            b = (b - sd[bn + ".running_mean"].double()) * g + sd[bn + ".bias"].double()
        w, b = w.float(), b.float()
        y = F.conv2d(q16(x), q16(w), None, stride, (w.shape[-1] - 1) // 2) + b[None, :, None, None]
        if res is not None:
            y = y + q16(res)
        if relu:
            y = F.relu(y)
        return q16(y)


@contextlib.contextmanager
def _patched(mod, **attrs):
    with _lock:
        old = {k: getattr(mod, k) for k in attrs}
        try:
            for k, v in attrs.items():
                setattr(mod, k, v)
            yield
        finally:
            for k, v in old.items():
                setattr(mod, k, v)


@contextlib.contextmanager
def _threads(n):
    old = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        yield
    finally:
        torch.set_num_threads(old)


def forward(sd: dict, cfg: dict, x0: torch.Tensor) -> torch.Tensor:
    """The yardstick recipe (one HRModule per stage, BasicBlock stage 1 without a width-changing transition: the stage
    tables of every golden fixture)."""
    assert tuple(cfg["modules"]) == (1, 1, 1, 1), "oracle.emulate_split_bf16.forward walks one module per stage"
    with _patched(ES, Emu=_Emu16, rq=q16), _threads(EMU_THREADS), torch.no_grad():
        return ES.forward(sd, cfg, x0, 3)


def forward_plan(sd: dict, cfg: dict, x0: torch.Tensor, taps: dict | None = None) -> torch.Tensor:
    """The plan's rounding points, with the intermediates (same names as oracle.emulate_bf16)."""
    with _patched(EB, q=q16), _threads(EMU_THREADS), torch.no_grad():
        return EB.forward(sd, cfg, x0, taps)


# ---- the yardstick: forward() against the `out` of the golden fixtures (the real reference's fp32 output, sub-sampled as
# the fixture stores it).  Computed on the CPU by tests/test_fp16_host.py::test_emulation_constants (which keeps them
# honest to 1 %); the GPU tests bound the GPU's error by 3 x these.
EMU_LINF = {
    "tiny_hrnet_64": 3.69e-4,
    "tiny_hrnet2_64": 5.05e-4,
    "w32_hrnet2_128": 4.95e-4,
    "w32_hrnet2_256": 6.63e-4,
    "w32_hrnet_256": 5.68e-4,
}
EMU_MEAN = {
    "tiny_hrnet_64": 6.27e-5,
    "tiny_hrnet2_64": 5.98e-5,
    "w32_hrnet2_128": 9.06e-5,
    "w32_hrnet2_256": 7.49e-5,
    "w32_hrnet_256": 8.63e-5,
}
BOUND_FACTOR = 3.0      # the margin the bf16 mode gave itself over its pre-measurement (9.8e-3 -> 3e-2)


def golden_case(g, synth, hrnet_ref):
    """(variant, cin, K, widths, state dict, crops, cfg) of a golden fixture, as tests/test_gpu_bf16.py builds them."""
    variant = str(g["variant"])
    cin, K = (3, 32) if variant == "seg_hrnet" else (1, 11)
    widths = tuple(int(v) for v in g["widths"])
    shapes = {str(k): tuple(int(v) for v in s.split(",")) if s else () for k, s in zip(g["state_keys"], g["state_shapes"])}
    sd = synth.make_state_dict(shapes, seed=int(g["seed"]), gain=0.5)
    x = synth.make_crops(int(g["n"]), cin, int(g["hw"]), int(g["hw"]), seed=int(g["seed"]))
    return variant, cin, K, widths, sd, x, hrnet_ref.default_cfg(cin, K, widths=widths)
