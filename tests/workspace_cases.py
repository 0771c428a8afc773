"""The networks, precisions, shapes and plan switches that tests/test_gpu_workspace.py (results must not depend on what the
workspace held on entry) and tests/test_workspace_plan_host.py (the planner's recycling rule, checked on the host) share.

The networks are the smallest at which channel padding and every kernel family appear:
  hrnet2_w16   16 real channels in a 32-wide tensor (64-wide in bf16 / fp16)
  hrnet2_w32   the production kernels: bblock32, job groups, multi-head, 128- and 256-cout slices, stem_x6, the fused heads
  hrnet2_w48   W48: 48 -> 64 and 192 -> 256 padding in the split formats
  hrnet_w16    cin 3, K 32
  hrnet3_w16   CBAM
  hrnet3_w48   W48 with CBAM, slice writers, zero_slice, head_gather"""

# key -> (module, cin, K, variant, widths)
NETS = {
    "hrnet2_w16": ("seg_hrnet2", 1, 11, 0, (16, 32, 64, 128)),
    "hrnet2_w32": ("seg_hrnet2", 1, 11, 0, (32, 64, 128, 256)),
    "hrnet2_w48": ("seg_hrnet2", 1, 11, 0, (48, 96, 192, 384)),
    "hrnet_w16": ("seg_hrnet", 3, 32, 0, (16, 32, 64, 128)),
    "hrnet3_w16": ("seg_hrnet3", 1, 30, 1, (16, 16, 32, 64)),
    "hrnet3_w48": ("seg_hrnet3", 1, 30, 1, (48, 96, 192, 384)),
}


def precisions(key):
    """Every precision the network supports: fp16 is built for variant 0 only."""
    return ["fp32", "bf16x3", "bf16"] + (["fp16"] if NETS[key][3] == 0 else [])


def shapes(key):
    """(n, height, width): two square crops, two oblong ones, and one whose every level ends in partial tiles (lowest level 3 x 5)."""
    return [(2, 64, 64), (2, 48, 80), (1, 34, 18) if NETS[key][3] == 1 else (1, 18, 34)]


# plan switch -> [(network, precisions it changes the plan of)]: the rule is plan_options() in csrc/plan_build.hip
_SB, _X6, _H16 = ["bf16x3"], ["fp32"], ["bf16", "fp16"]
SWITCHES = {
    "UNFUSED": [("hrnet2_w32", _SB)],                        # split format: stem, bblock32 and the fused head
    "HEAD_V1": [("hrnet2_w32", _SB + _X6 + _H16)],           # no second-generation head in any format
    "FINAL_VALU": [("hrnet2_w32", _SB + ["bf16"])],          # (fp32 has no matrix-core output layer, fp16 no VALU one)
    "NO_MULTIHEAD": [("hrnet2_w32", _SB)],
    "NO_JOBS": [("hrnet2_w32", _SB + _X6 + _H16), ("hrnet3_w48", _SB + _X6 + ["bf16"])],
    "NO_BBLOCK": [("hrnet2_w32", _SB)],
    "NO_CBAM_JOBS": [("hrnet3_w48", _SB + _X6 + ["bf16"])],
    "CBAM_UNFUSED": [("hrnet3_w48", _SB + _X6 + ["bf16"])],
    "STEM_POOL_SEPARATE": [("hrnet3_w48", _SB + _X6 + ["bf16"])],
    "HEAD3_DIRECT": [("hrnet3_w48", _SB + _X6)],             # (bf16 always takes the direct head)
    "HEAD3_COUT32": [("hrnet3_w48", _SB + _X6)],
    "BF_UNFUSED_HEAD": [("hrnet2_w32", _H16)],
    "BF_HEAD_VALU": [("hrnet2_w32", ["bf16"])],              # (ignored in fp16)
    "X6_UNFUSED_HEAD": [("hrnet2_w32", _X6)],
    "X6_UNFUSED_STEM": [("hrnet2_w32", _X6), ("hrnet3_w48", _X6)],
}


def switch_cases():
    return [(sw, key, prec) for sw, rows in SWITCHES.items() for key, precs in rows for prec in precs]
