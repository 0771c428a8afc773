// plan.hip — host runtime behind the C-ABI (include/esahrnet.h): stage table -> static plan
// (list of fused kernels over SB tensors), weight packing, workspace planning, forward.  Every entry that takes a handle is
// here; the ones that take none are in abi_decode.hip and op_abi.hip (the stand-alone operator entries, esahrnet_op_*).
//
// Reference being replaced: models/seg_hrnet.py:260-423 (module construction) and :425-473
// (forward).  The plan is NOT a transcription of the module tree:
//   * every BatchNorm2d is folded into its convolution by the host before esahrnet_set_conv;
//   * conv + bias + residual + ReLU are one kernel (conv_mfma.hip);
//   * the cross-resolution sums are one kernel per output branch (fuse.hip);
//   * last_layer[0] (1x1, 480->480 on the concatenated, up-sampled branches, 26 % of the
//     reference's MACs) is evaluated per branch at the branch's own resolution and summed by the
//     fuse kernel — a 1x1 convolution commutes with bilinear interpolation (both linear, the
//     interpolation weights act per channel), so conv(cat(up(x_b))) = sum_b up(conv_b(x_b))
//     exactly in real arithmetic; it needs 8x fewer MACs and never builds the 480-channel concat;
//   * last_layer[6] + concat + output_layer are one kernel (head.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/esahrnet.h"
#include "devstate.h"
#include "host_util.h"
#include "kernels.h"

namespace esa {
int final_kt(int K);
// abi_decode.hip: the argument checks its handle-free entries share with the loader entries here (`who` names the entry)
extern const int kFrontendMaxRows;
int check_boxes_args(const char* who, int m, int frame_h, int frame_w, int scale, int rule);
int check_crops_args(const char* who, int nframes, int pixel_format, float stdv);
int check_cov_args(const char* who, const void* cov_dev, const void* info_dev, double cov_floor);
int check_corr_args(const char* who, int m, int k, int mode);
}

namespace {

thread_local char g_err[512] = "";

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return 1;
}

using esa::pad32;
using esa::pad64;
using esa::upload;

struct ConvSpec {               // one Conv2d of the reference module tree
    std::string name, bn;
    int cin, cout, k, stride, level;   // level: output resolution level (0 = crop, 1 = /2, ...)
    bool has_bias, relu;
    std::vector<float> w, b;    // folded weights as handed over by the host
    bool set = false;
    // derived spec (not visible to the host; filled at commit): the nine taps of input channels [pc0, pc1) of 3x3 spec `parent`
    // as ONE 1x1 convolution with 9 * cout outputs, output channel (co / 8) * 72 + tap * 8 + co % 8 (head_gather.hip)
    int parent = -1, pc0 = 0, pc1 = 0;
};

struct DevConv {                // one MFMA convolution launch (a ConvSpec or a cin-slice of one)
    int spec;                   // index into specs
    int c0, c1;                 // input-channel slice of the spec
    bool use_bias;
    bool out_f32 = false;       // output plain f32 NHWC instead of SB (head terms)
    std::vector<int> perm;      // optional input-channel permutation: packed ci -> spec ci
    int cinp, coutp;
    void* w = nullptr;          // device, packed
    float* bias = nullptr;      // device, f32 [coutp]
};

enum OpKind { OP_STEM, OP_STEMF, OP_CONV, OP_BLOCK, OP_FUSE, OP_HEAD, OP_HEADT, OP_HEAD2, OP_FINAL, OP_HEADBF,
              // seg_hrnet3 (CBAM) variant only:
              OP_STEMRAW, OP_POOL, OP_MLP, OP_MAPS, OP_APPLY, OP_RESAMPLE, OP_ZERO, OP_TONCHW, OP_GATHER };

struct AuxSpec {                // a non-conv parameter tensor (CBAM weights)
    std::string name;
    int shape[4];
    std::vector<float> data;
    bool set = false;
    float* dev = nullptr;
};

struct Tensor {
    int C, Cp, level;
    int flat = 0;               // > 0: plain f32 scratch of `flat` floats per sample (no spatial extent)
    std::string tap;            // name for esahrnet_tap_read, "" if anonymous
    std::string key;            // what the tensor is, whatever launch writes it (esahrnet_diff_row_get): the tap name, else the
                                // convolution whose output it is, else a name the builder gives it; "" for scratch
    bool tlayout = false;       // head term in the transposed T layout (head_t.hip): row pitch head_t_xp(w)
    bool f32 = false;           // plain f32 NHWC whatever the plan's format (the output of an out_f32 convolution)
    int alt = 0;                // 0: always; 1 / 2: only when the first / second generation head runs
    int def = -1, last = -1;    // op indices
    size_t off = 0;             // per-shape plan
};

struct Op {
    OpKind kind;
    int dconv = -1;             // OP_CONV / OP_STEMF / OP_BLOCK (conv1)
    int dconv2 = -1;            // OP_BLOCK (conv2)
    int in = -1, out = -1, res = -1;
    int out2 = -1;              // second tensor this op writes (OP_STEMRAW: the pooled partials of its output), allocated with it
    int terms[4] = {-1, -1, -1, -1};
    int nterms = 0;
    bool relu = false;
    int lane = 0;               // execution lane (stream): 0 = caller's stream, 1..3 = side streams (schedule_waves)
    int wave = 0;               // waves run one after another; inside a wave the lanes run beside each other
    int wait0 = -1;             // side-lane launch: lane-0 op whose event it waits for first (-1: none)
    bool wait_entry = false;    // side-lane launch: waits for the wave's entry event first
    bool record = false;        // lane-0 op: an event is recorded behind it (a side lane forks from here)
    unsigned join = 0;          // lane-0 launch: side lanes (bit l) lane 0 waits for first
    int aux[3] = {-1, -1, -1};  // CBAM ops: fc.0 (on every step: it names the layer), fc.2, sa.conv1
    int c0 = 0;                 // channel offset inside `out` (OP_APPLY / OP_RESAMPLE / OP_ZERO)
    int nchan = 0;              // OP_ZERO: channels to clear;  OP_RESAMPLE/OP_APPLY/OP_MAPS: real channels
    int align = 0;              // OP_RESAMPLE: align_corners
    int alt = 0;                // 0: always; 1: head_fused path only; 2: head_fused2 path only (chosen per shape)
    int multi = -1, mpos = 0;   // OP_CONV: member mpos of multi-head group `multi` (mpos 0 launches for all members)
    int jkey = -1;              // OP_CONV of an HRModule branch: (module id << 8) | position along the branch's conv chain
    int job = -1, jpos = 0;     // member jpos of job group `job` (independent same-depth convs of several branches, one launch)
};

// stride-2 3x3 convolutions of the SAME input tensor (the first links of the fuse-down chains of a stage), evaluated
// by one multi-head launch of the stream kernel: the input is read once instead of once per chain
struct Multi {
    int n = 0;
    int op[3] = {-1, -1, -1};   // op indices, consecutive: op[0] = leader
    void* w = nullptr;          // device: the members' packed weights, concatenated along cout
    float* bias = nullptr;
    int coutp = 0;
};

// the same-depth 3x3 convolutions of the branches of one HRModule: independent, evaluated by one launch of the stream
// kernel's multi-convolution form where every member is a 64-cout stream launch at the shape at hand
struct JobGroup {
    int n = 0;
    int op[6] = {-1, -1, -1, -1, -1, -1};   // op indices, consecutive: op[0] = leader
};

struct ShapePlan {
    int n = 0, h = 0, w = 0;
    bool keep = false;
    size_t bytes = 0;
    std::vector<int> lh, lw;    // resolution per level
    bool head2 = false;         // this shape runs the second-generation head (ops with alt == 2)
    bool head2_ulo = false;     // ... with the lo part of the interpolation weights
    std::vector<char> multi_on; // per Multi: evaluated as one launch at this shape
    std::vector<char> job_on;   // per JobGroup: evaluated as one launch at this shape
};

enum StemForm { STEM_SEPARATE, STEM_FUSED, STEM_FUSED_X6 };
enum HeadForm { HEAD_UNFUSED, HEAD_SB, HEAD_BF, HEAD_X6 };

// The plan switches and what follows from them and the configuration.  plan_options() fills it once, in
// esahrnet_create, and nothing writes it afterwards: a handle's plan and launches depend on the environment at its creation.
struct PlanOptions {
    // ESAHRNET_<NAME>, on unless unset, empty or "0"
    bool unfused, head_v1, final_valu, no_multihead, no_jobs, no_bblock, no_cbam_jobs, cbam_unfused, stem_pool_separate,
         head3_direct, head3_cout32, bf_unfused_head, bf_head_valu, x6_unfused_head, x6_unfused_stem, x6_reload_weights, tap_all;
    int nlanes;                 // 4 if ESAHRNET_STREAMS > 1 (the wave executor), else 1: everything on the caller's stream
    int fmt;                    // tensor format: FMT_SB (precision 0), FMT_BF (1: single bf16), FMT_F32 (2: bf16x6 arithmetic),
                                // FMT_HF (3: single fp16 — the bf16 mode's plan op for op, fp16 elements)
    StemForm stem;              // conv1 + conv2: stem_kernel + stride-2 convolution, stem_fused, or stem_x6_kernel
    bool fused_block;           // a 32-channel BasicBlock outside the job groups is one bblock32 launch
    HeadForm head;              // seg_hrnet / seg_hrnet2: the fused head kernel the plan carries (seg_hrnet3 has its own head)
    bool head2;                 // the second head alternative (head_fused2, head_fused_bf, head_x6) may be chosen per shape
    bool final_mfma;            // seg_hrnet / seg_hrnet2: output layer on the matrix cores (final_mfma_kernel)
};

PlanOptions plan_options(const esahrnet_cfg& g, const esa::Format& format) {
    const auto on = esa::env_on;
    PlanOptions o;
    o.unfused = on("ESAHRNET_UNFUSED"); o.head_v1 = on("ESAHRNET_HEAD_V1"); o.final_valu = on("ESAHRNET_FINAL_VALU");
    o.no_multihead = on("ESAHRNET_NO_MULTIHEAD"); o.no_jobs = on("ESAHRNET_NO_JOBS"); o.no_bblock = on("ESAHRNET_NO_BBLOCK");
    o.no_cbam_jobs = on("ESAHRNET_NO_CBAM_JOBS"); o.cbam_unfused = on("ESAHRNET_CBAM_UNFUSED");
    o.stem_pool_separate = on("ESAHRNET_STEM_POOL_SEPARATE"); o.head3_direct = on("ESAHRNET_HEAD3_DIRECT");
    o.head3_cout32 = on("ESAHRNET_HEAD3_COUT32"); o.bf_unfused_head = on("ESAHRNET_BF_UNFUSED_HEAD");
    o.bf_head_valu = on("ESAHRNET_BF_HEAD_VALU"); o.x6_unfused_head = on("ESAHRNET_X6_UNFUSED_HEAD");
    o.x6_unfused_stem = on("ESAHRNET_X6_UNFUSED_STEM"); o.tap_all = on("ESAHRNET_TAP_ALL");
    o.x6_reload_weights = on("ESAHRNET_X6_RELOAD_WEIGHTS");     // (changes no op: the same launches, the same names)
    const char* streams = getenv("ESAHRNET_STREAMS");
    o.nlanes = streams && atoi(streams) > 1 ? 4 : 1;
    o.fmt = format.fmt;
    const bool sb = o.fmt == esa::FMT_SB, v0 = g.variant == 0;
    // the fused stem kernels: stem_fused serves every (cin, stem width) in the split format, stem_x6_kernel one; none in bf16
    const bool x6_stem = esa::stem_fused_x6_supported(g.cin, pad32(g.stem_width), pad32(g.stem_width)) && g.stem_width == 64;
    o.stem = sb && (!v0 || !o.unfused) ? STEM_FUSED
           : o.fmt == esa::FMT_F32 && x6_stem && !o.x6_unfused_stem ? STEM_FUSED_X6 : STEM_SEPARATE;
    // bblock32 is built for the split format, and seg_hrnet3's block has a CBAM inside
    o.fused_block = sb && v0 && !o.unfused && !o.no_bblock;
    int nb4 = 0;                // branches of stage 4
    while (nb4 < ESAHRNET_MAX_BRANCHES && g.blocks[3][nb4] > 0) ++nb4;
    const int c0 = pad32(g.widths[0]);
    o.head = !v0 || nb4 != 4 ? HEAD_UNFUSED
           : sb ? (!o.unfused && (c0 == 32 || c0 == 64) ? HEAD_SB : HEAD_UNFUSED)
           : esa::fmt_half(o.fmt) ? (!o.bf_unfused_head && (pad64(g.widths[0]) == 64 || pad64(g.widths[0]) == 128) ? HEAD_BF : HEAD_UNFUSED)
           : !o.x6_unfused_head && (c0 == 32 || c0 == 64) ? HEAD_X6 : HEAD_UNFUSED;
    // head_fused2 needs head_t's channel counts on branches 2 and 3 and 64 or 96 on branch 1
    o.head2 = !o.head_v1 && (o.head != HEAD_SB || ((pad32(g.widths[1]) == 64 || pad32(g.widths[1]) == 96) &&
                                                   esa::head_t_supported(pad32(g.widths[2])) && esa::head_t_supported(pad32(g.widths[3]))));
    o.final_mfma = v0 && o.fmt != esa::FMT_F32 && !o.final_valu && esa::final_mfma_supported(g.num_keypoints, g.cin);
    return o;
}

}  // namespace

int esa::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return 1;
}

// May these convolutions of one format, kernel size and stride run as ONE merged launch?  A stride-1 3x3 of the other
// formats must be a stream-kernel launch on its own too (conv_is_stream_s1): the kernel serving a layer never depends
// on the grouping.  The rule of job_on_for and of esahrnet_op_conv_group.
bool esa::conv_group_mergeable(int fmt, const esa::ConvParams* ps, int n, int k, int stride) {
    if (fmt == esa::FMT_F32) return esa::conv_x6_jobs_supported(ps, n, k, stride);
    if (k == 1) return esa::conv1x1_jobs_supported(ps, n);
    if (stride == 1)
        for (int j = 0; j < n; ++j)
            if (!esa::conv_is_stream_s1(ps[j])) return false;
    return esa::conv_jobs_supported(ps, n, stride);
}

// name of the kernel that merged launch runs, as rocprofv3 prints it (op_desc_get, esahrnet_op_conv_group)
void esa::conv_group_kernel_name(char* out, size_t cap, int fmt, const esa::ConvParams* ps, int n, int k, int stride) {
    if (fmt == esa::FMT_F32 && k == 1 && esa::conv1x1_x6_jobs_supported(ps, n)) snprintf(out, cap, "conv1x1_x6_jobs_kernel");
    else if (fmt == esa::FMT_F32) snprintf(out, cap, "conv_x6_jobs_kernel<%d, %d>", k, stride);
    else if (k == 1) snprintf(out, cap, "conv1x1_jobs_kernel");
    else snprintf(out, cap, "conv_s2c32_jobs_kernel<%d, %d, %s>", stride, stride == 1 ? 8 : 4,
                  fmt == esa::FMT_HF ? "fp16" : esa::fmt_half(fmt) ? "true" : "false");
}

struct esahrnet_ctx {
    esahrnet_cfg cfg;
    int device;
    std::vector<ConvSpec> specs;
    std::map<std::string, int> spec_by_name;
    std::vector<DevConv> dconvs;
    std::vector<AuxSpec> aux;
    float *stemraw_w = nullptr, *stemraw_b = nullptr;     // variant 1: un-normalised conv1 for the skip
    std::vector<Tensor> tensors;
    std::vector<Op> ops;
    int spec_stem = -1, spec_final = -1;
    float *stem_w = nullptr, *stem_b = nullptr, *final_w = nullptr, *final_b = nullptr;
    void* final_wpk = nullptr;  // output_layer weights as MFMA fragments (head.hip, final_mfma_kernel)
    int spec_l0 = -1, spec_l3 = -1, head_c0 = 0;     // fused head (OP_HEAD)
    void *head_w0 = nullptr, *head_w3 = nullptr;
    float *head_b0 = nullptr, *head_b3 = nullptr;
    bool committed = false;
    bool keep = false;
    PlanOptions opt;
    esa::Format format;         // the format of cfg.precision (host_util.h; opt.fmt is its code): what the members below answer from
    bool h16() const { return format.half; }
    bool hf() const { return format.hf; }
    bool x6() const { return format.x6; }
    int padc(int ch) const { return format.pad(ch); }
    int eb() const { return format.eb; }
    size_t wbytes(int coutp, int cinp, int k) const { return format.wbytes(coutp, cinp, k); }
    std::vector<char> pack(const float* w, int cout, int cin, int k, int coutp, int cinp) const { return format.pack(w, cout, cin, k, coutp, cinp); }
    int head2_op = -1;          // index of the OP_HEAD2 op, -1 if the plan has none
    // wave executor (schedule_waves): the launches of a wave that do not depend on each other run on up to four lanes
    // (the caller's stream + three side streams), fork/join through the caller's stream at every wave boundary (opt.nlanes)
    int nwaves = 1;
    std::vector<int> wave_last;                       // per wave: index of its last op
    std::vector<unsigned char> wave_mask;             // per wave: bit l set = lane l has work
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> wave_entry;               // per wave: recorded on the caller's stream when the wave opens
    std::vector<hipEvent_t> wave_end;                 // per op x side lane (Op::join) + the final join
    std::vector<hipEvent_t> op_event;                 // per op with Op::record
    ShapePlan sp;
    int max_level = 0;
    int nhost_specs = -1;       // specs [nhost_specs, end) are derived (ConvSpec::parent); -1: none
    int stemraw_partial = -1;   // seg_hrnet3: tensor of the pooled partials of the raw stem output when the stem kernel makes them
    std::vector<Multi> multis;
    std::vector<JobGroup> jobs;
    // fp16 scale groups (build_scale_groups; variant 0 in a 16-bit format, else none): the group of every tensor (-1: none), a
    // name per group, and the exponent the host gave each (tensor T of group g is stored as T * 2^-exps[g]; all zero by default)
    std::vector<int> tgroup;
    std::vector<std::string> gnames;
    std::vector<int32_t> exps;
    bool scaled() const { for (int32_t e : exps) if (e) return true; return false; }
    int gexp(int g) const { return g < 0 ? 0 : exps[g]; }
};

namespace {

struct Builder {
    esahrnet_ctx& c;
    int jkey = -1;              // job key given to the next stride-1 convolutions (HRModule branches), -1: none
    int jkey2 = -1;             // job key given to the next stride-2 convolution (fuse-down chain link), -1: none
    explicit Builder(esahrnet_ctx& ctx) : c(ctx) {}

    int spec(const std::string& name, const std::string& bn, int cin, int cout, int k, int stride,
             int level, bool bias, bool relu) {
        ConvSpec s;
        s.name = name; s.bn = bn; s.cin = cin; s.cout = cout; s.k = k; s.stride = stride;
        s.level = level; s.has_bias = bias; s.relu = relu;
        c.specs.push_back(s);
        c.spec_by_name[name] = (int)c.specs.size() - 1;
        c.max_level = std::max(c.max_level, level);
        return (int)c.specs.size() - 1;
    }
    int taps_spec(int parent, int c0, int c1, int level) {
        const std::string name = c.specs[parent].name + "#taps[" + std::to_string(c0) + ":" + std::to_string(c1) + "]";
        const int cout9 = 9 * ((c.specs[parent].cout + 7) & ~7);
        const int sp = spec(name, "", c1 - c0, cout9, 1, 1, level, false, false);
        c.specs[sp].parent = parent; c.specs[sp].pc0 = c0; c.specs[sp].pc1 = c1;
        if (c.nhost_specs < 0) c.nhost_specs = sp;
        return sp;
    }
    int tensor(int C, int level, const std::string& tap = "") {
        Tensor t;
        t.C = C; t.Cp = c.padc(C); t.level = level; t.tap = tap; t.key = tap;
        c.tensors.push_back(t);
        return (int)c.tensors.size() - 1;
    }
    void use(int t, int op) {
        if (t < 0) return;
        c.tensors[t].last = std::max(c.tensors[t].last, op);
    }
    // conv op on a spec (optionally a cin slice, optionally plain-f32 output); returns the output tensor
    int conv(int sp, int in, int res, bool relu, const std::string& tap = "", int c0 = 0, int c1 = -1,
             bool use_bias = true, bool out_f32 = false) {
        const ConvSpec& s = c.specs[sp];
        DevConv d;
        d.spec = sp; d.c0 = c0; d.c1 = c1 < 0 ? s.cin : c1; d.use_bias = use_bias; d.out_f32 = out_f32;
        d.cinp = c.padc(d.c1 - d.c0); d.coutp = c.padc(s.cout);
        c.dconvs.push_back(d);
        Op o;
        o.kind = OP_CONV; o.dconv = (int)c.dconvs.size() - 1; o.in = in; o.res = res; o.relu = relu;
        if (jkey >= 0 && s.k == 3 && s.stride == 1) o.jkey = jkey++;
        if (jkey2 >= 0 && ((s.k == 3 && s.stride == 2) || s.k == 1)) o.jkey = jkey2;
        // ESAHRNET_TAP_ALL=1 (debugging): every convolution output becomes a named tap
        o.out = tensor(s.cout, s.level, tap.empty() && !out_f32 && c.opt.tap_all ? "conv:" + s.name : tap);
        c.tensors[o.out].f32 = out_f32;
        c.tensors[o.out].key = !tap.empty() ? tap : d.c0 != 0 || d.c1 != s.cin
            ? s.name + "[:, " + std::to_string(d.c0) + ":" + std::to_string(d.c1) + "]" : s.name;
        const int idx = (int)c.ops.size();
        c.tensors[o.out].def = idx;
        use(in, idx); use(res, idx);
        c.ops.push_back(o);
        return o.out;
    }
    int fuse(const std::vector<int>& terms, int C, int level, bool relu, const std::string& tap = "", const std::string& key = "") {
        Op o;
        o.kind = OP_FUSE; o.nterms = (int)terms.size(); o.relu = relu;
        o.out = tensor(C, level, tap);
        if (tap.empty()) c.tensors[o.out].key = key;
        const int idx = (int)c.ops.size();
        c.tensors[o.out].def = idx;
        for (int i = 0; i < o.nterms; ++i) { o.terms[i] = terms[i]; use(terms[i], idx); }
        c.ops.push_back(o);
        return o.out;
    }
    int aux(const std::string& name, int a, int b, int kh, int kw) {
        AuxSpec s;
        s.name = name; s.shape[0] = a; s.shape[1] = b; s.shape[2] = kh; s.shape[3] = kw;
        c.aux.push_back(s);
        return (int)c.aux.size() - 1;
    }
    int push(Op& o) {
        const int idx = (int)c.ops.size();
        if (o.out >= 0 && c.tensors[o.out].def < 0) c.tensors[o.out].def = idx;
        use(o.in, idx); use(o.res, idx);
        for (int i = 0; i < 4; ++i) use(o.terms[i], idx);
        c.ops.push_back(o);
        return idx;
    }
    int flat_tensor(int floats_per_sample) {
        Tensor t;
        t.C = t.Cp = 0; t.level = 0; t.flat = floats_per_sample;
        c.tensors.push_back(t);
        return (int)c.tensors.size() - 1;
    }
    // CBAM (seg_hrnet3.py:32-61, 90-91): y[:, c0:c0+C] = [relu]( sa(ca*x) * (ca*x) [+ res] ); prefix p
    // names the owner of .ca / .sa ("" = the network's own).  Returns nothing: writes into `y`.
    void cbam(const std::string& p, int x, int C, int res, bool relu, int y, int y_c0) {
        const std::string q = p.empty() ? "" : p + ".";
        const int cr = C / 16;
        const int a0 = aux(q + "ca.fc.0.weight", cr, C, 1, 1), a1 = aux(q + "ca.fc.2.weight", C, cr, 1, 1);
        const int a2 = aux(q + "sa.conv1.weight", 1, 2, 7, 7);
        const int level = c.tensors[x].level, Cp = c.tensors[x].Cp;
        const int partial = flat_tensor(esa::POOL_SLABS * Cp * 2), cav = flat_tensor(Cp);
        Tensor mt; mt.C = 2; mt.Cp = 2; mt.level = level; mt.f32 = true;       // (f32 [N][H][W][2] in every format)
        mt.key = q + "sa.maps";
        c.tensors.push_back(mt);
        const int maps = (int)c.tensors.size() - 1;
        // inside an HRModule branch (jkey >= 0) the four CBAM launches take the next depth keys behind the block's two
        // convolutions, so that group_jobs can put the module in depth-major order and merge the convolutions of its branches
        auto key = [&]() { return jkey >= 0 ? jkey++ : -1; };
        { Op o; o.kind = OP_POOL; o.in = x; o.out = partial; o.aux[0] = a0; o.jkey = key(); push(o); }
        { Op o; o.kind = OP_MLP; o.in = partial; o.out = cav; o.aux[0] = a0; o.aux[1] = a1; o.nchan = C; o.terms[0] = x; o.jkey = key(); push(o); }
        { Op o; o.kind = OP_MAPS; o.in = x; o.terms[1] = cav; o.out = maps; o.aux[0] = a0; o.nchan = C; o.jkey = key(); push(o); }
        { Op o; o.kind = OP_APPLY; o.in = x; o.res = res; o.terms[1] = cav; o.terms[2] = maps; o.aux[0] = a0; o.aux[2] = a2;
          o.out = y; o.c0 = y_c0; o.relu = relu; o.nchan = C; o.jkey = key(); push(o); }
    }
    // BasicBlock of seg_hrnet3.py:64-103: conv-bn-relu-conv-bn, CBAM, (+res), relu
    int basic_block_cbam(const std::string& p, int x, int cin, int cout, int level, const std::string& tap) {
        int res = x;
        const int c1 = spec(p + ".conv1", p + ".bn1", cin, cout, 3, 1, level, false, true);
        const int c2 = spec(p + ".conv2", p + ".bn2", cout, cout, 3, 1, level, false, false);
        if (cin != cout) {
            const int d = spec(p + ".downsample.0", p + ".downsample.1", cin, cout, 1, 1, level, false, false);
            res = conv(d, x, -1, false);
        }
        const int o1 = conv(c1, x, -1, true);
        const int o2 = conv(c2, o1, -1, false);
        const int y = tensor(cout, level, tap);
        if (tap.empty()) c.tensors[y].key = p + ".cbam";
        cbam(p, o2, cout, res, true, y, 0);
        return y;
    }
    // BasicBlock (seg_hrnet.py:32-61): conv-bn-relu-conv-bn (+res) relu
    int basic_block(const std::string& p, int x, int cin, int cout, int level, const std::string& tap) {
        if (c.cfg.variant == 1) return basic_block_cbam(p, x, cin, cout, level, tap);
        int res = x;
        const int c1 = spec(p + ".conv1", p + ".bn1", cin, cout, 3, 1, level, false, true);
        const int c2 = spec(p + ".conv2", p + ".bn2", cout, cout, 3, 1, level, false, true);
        // whole block in one kernel (bblock32.hip) — for layer1; inside the HRModules the block's two convolutions join the
        // same-depth convolutions of the other branches in one launch instead (group_jobs; ESAHRNET_NO_JOBS=1: fused block)
        const bool in_job = jkey >= 0 && !c.opt.no_jobs;
        if (c.opt.fused_block && cin == cout && pad32(cin) == 32 && !in_job) {
            Op o;
            o.kind = OP_BLOCK; o.in = x; o.relu = true;
            for (int k = 0; k < 2; ++k) {
                DevConv d;
                d.spec = k ? c2 : c1; d.c0 = 0; d.c1 = cin; d.use_bias = true; d.cinp = 32; d.coutp = 32;
                c.dconvs.push_back(d);
                (k ? o.dconv2 : o.dconv) = (int)c.dconvs.size() - 1;
            }
            o.out = tensor(cout, level, tap);
            if (tap.empty()) c.tensors[o.out].key = c.specs[c2].name;
            const int idx = (int)c.ops.size();
            c.tensors[o.out].def = idx;
            use(x, idx);
            c.ops.push_back(o);
            return o.out;
        }
        if (cin != cout) {
            const int d = spec(p + ".downsample.0", p + ".downsample.1", cin, cout, 1, 1, level, false, false);
            res = conv(d, x, -1, false);
        }
        const int o = conv(c1, x, -1, true);
        return conv(c2, o, res, true, tap);
    }
};

// Post-pass over the op list: find the stride-2 3x3 convolutions that share their input and make each such group
// consecutive (moving a member EARLIER is always legal: its only input is defined before the group's first member).
void group_multihead(esahrnet_ctx& c) {
    if (c.opt.no_multihead || c.opt.fmt != esa::FMT_SB) return;
    auto eligible = [&](const Op& o) {
        if (o.kind != OP_CONV || o.res >= 0 || o.alt != 0 || o.multi >= 0) return false;
        const DevConv& d = c.dconvs[o.dconv];
        const ConvSpec& s = c.specs[d.spec];
        return s.k == 3 && s.stride == 2 && !d.out_f32 && d.c0 == 0 && d.c1 == s.cin && d.perm.empty() && d.use_bias;
    };
    std::vector<Op> ops = c.ops;
    for (size_t i = 0; i < ops.size(); ++i) {
        if (!eligible(ops[i])) continue;
        std::vector<size_t> members{i};
        for (size_t j = i + 1; j < ops.size() && members.size() < 3; ++j)
            if (eligible(ops[j]) && ops[j].in == ops[i].in) members.push_back(j);
        if (members.size() < 2) continue;
        // measured (W32, batch 32): worth it only where the shared input is the big 32/48-channel branch AND the
        // heads add up to whole 64-cout workgroup slices (stage 4: 53.4 -> 40.8 us); 96 couts on 32-cout slices
        // (stage 3: 40.1 -> 45.2 us) and the 64-channel input (31.8 -> 32.6 us) are not
        {
            int tot = 0;
            for (size_t k : members) tot += c.dconvs[ops[k].dconv].coutp;
            if (tot % 64 != 0 || c.dconvs[ops[i].dconv].cinp > 64 || c.tensors[ops[i].in].level > 1) continue;
        }
        const int mi = (int)c.multis.size();
        Multi m;
        m.n = (int)members.size();
        // pull the members up behind the leader (back to front so that the indices stay valid)
        std::vector<Op> pulled;
        for (size_t k = members.size(); k-- > 1;) {
            pulled.insert(pulled.begin(), ops[members[k]]);
            ops.erase(ops.begin() + members[k]);
        }
        ops.insert(ops.begin() + i + 1, pulled.begin(), pulled.end());
        for (int k = 0; k < m.n; ++k) {
            ops[i + k].multi = mi;
            ops[i + k].mpos = k;
            m.op[k] = (int)(i + k);
            m.coutp += c.dconvs[ops[i + k].dconv].coutp;
        }
        c.multis.push_back(m);
    }
    c.ops = ops;
    // op indices moved: recompute first definition / last use of every tensor and the head2 op index
    for (Tensor& t : c.tensors) { t.def = -1; t.last = -1; }
    c.head2_op = -1;
    for (size_t k = 0; k < c.ops.size(); ++k) {
        const Op& o = c.ops[k];
        if (o.kind == OP_HEAD2) c.head2_op = (int)k;
        if (o.out >= 0 && c.tensors[o.out].def < 0) c.tensors[o.out].def = (int)k;
        if (o.out2 >= 0 && c.tensors[o.out2].def < 0) c.tensors[o.out2].def = (int)k;
        auto use = [&](int t) { if (t >= 0) c.tensors[t].last = std::max(c.tensors[t].last, (int)k); };
        use(o.in); use(o.res);
        for (int t = 0; t < 4; ++t) use(o.terms[t]);
    }
}

// Post-pass: inside one HRModule the branches are independent chains of 3x3 convolutions.  The builder emits them
// branch by branch; here the convolutions of a module are put in depth-major order (stable, so every branch keeps its own
// order) and the same-depth ones of up to three branches become a JobGroup.
void group_jobs(esahrnet_ctx& c) {
    if (c.opt.no_jobs) return;
    std::vector<Op> ops = c.ops;
    auto eligible = [&](const Op& o) {
        // the CBAM launches of a depth (seg_hrnet3): same kind on every branch, one launch (cbam.hip: cbam_jobs_kernel)
        if ((o.kind == OP_POOL || o.kind == OP_MLP || o.kind == OP_MAPS || o.kind == OP_APPLY) && o.jkey >= 0)
            return !c.opt.no_cbam_jobs;
        if (o.kind != OP_CONV || o.jkey < 0 || o.alt != 0 || o.multi >= 0) return false;
        const DevConv& d = c.dconvs[o.dconv];
        const ConvSpec& s = c.specs[d.spec];
        if (s.k == 1) return !c.h16() && o.res < 0 && !d.out_f32 && d.c0 == 0 && d.c1 == s.cin && d.perm.empty() && d.use_bias;
        return s.k == 3 && !d.out_f32 && d.c0 == 0 && d.c1 == s.cin && d.perm.empty() && d.use_bias &&
               d.coutp % (c.h16() ? 64 : 32) == 0;
    };
    size_t i = 0;
    while (i < ops.size()) {
        if (ops[i].jkey < 0) { ++i; continue; }
        const int mod = ops[i].jkey >> 8;
        size_t j = i;
        while (j < ops.size() && ops[j].jkey >= 0 && (ops[j].jkey >> 8) == mod) ++j;      // [i, j): this module's branch convs
        std::stable_sort(ops.begin() + i, ops.begin() + j, [](const Op& a, const Op& b) { return (a.jkey & 255) < (b.jkey & 255); });
        for (size_t a = i; a < j;) {
            size_t b = a;
            std::vector<size_t> mem;
            const size_t cap = ops[a].kind == OP_CONV && c.specs[c.dconvs[ops[a].dconv].spec].k == 1 ? 6 : 4;
            while (b < j && ops[b].jkey == ops[a].jkey) { if (eligible(ops[b]) && mem.size() < cap) mem.push_back(b); ++b; }
            // members must be consecutive for the leader to stand for them: move the ineligible ones of this depth behind
            if (mem.size() >= 2) {
                std::vector<Op> grp, rest;
                for (size_t k = a; k < b; ++k) (std::find(mem.begin(), mem.end(), k) != mem.end() ? grp : rest).push_back(ops[k]);
                JobGroup g;
                g.n = (int)grp.size();
                for (int k = 0; k < g.n; ++k) { grp[k].job = (int)c.jobs.size(); grp[k].jpos = k; g.op[k] = (int)(a + k); }
                std::copy(grp.begin(), grp.end(), ops.begin() + a);
                std::copy(rest.begin(), rest.end(), ops.begin() + a + grp.size());
                c.jobs.push_back(g);
            }
            a = b;
        }
        i = j;
    }
    c.ops = ops;
    for (Tensor& t : c.tensors) { t.def = -1; t.last = -1; }
    c.head2_op = -1;
    for (size_t k = 0; k < c.ops.size(); ++k) {
        const Op& o = c.ops[k];
        if (o.kind == OP_HEAD2 || o.kind == OP_HEADBF) c.head2_op = (int)k;
        if (o.out >= 0 && c.tensors[o.out].def < 0) c.tensors[o.out].def = (int)k;
        if (o.out2 >= 0 && c.tensors[o.out2].def < 0) c.tensors[o.out2].def = (int)k;
        auto use = [&](int t) { if (t >= 0) c.tensors[t].last = std::max(c.tensors[t].last, (int)k); };
        use(o.in); use(o.res);
        for (int t = 0; t < 4; ++t) use(o.terms[t]);
    }
    // the multi-head groups refer to op indices too
    for (Multi& m : c.multis) m.n = 0;
    for (size_t k = 0; k < c.ops.size(); ++k)
        if (c.ops[k].multi >= 0) { Multi& m = c.multis[c.ops[k].multi]; m.op[c.ops[k].mpos] = (int)k; m.n = std::max(m.n, c.ops[k].mpos + 1); }
}

// Post-pass: lanes and waves.  Lane 0 is the caller's stream (the trunk), lanes 1..3 are side streams.  A launch unit (one
// op, or the consecutive members of a job / multi-head group) is placed by what it depends on among the not yet joined
// launches of the current wave — earlier writers of what it reads, earlier readers and writers of what it writes:
//   lane 0 only, incl. its tail   -> lane 0: it continues the trunk;
//   lane 0 only, not the tail     -> it forks onto the least loaded side lane behind the event of its latest lane-0
//                                    dependency (or the wave's entry event): what lane 0 has queued since runs beside it;
//   one side lane, not the trunk tail -> that side lane (behind the event of its latest lane-0 dependency, if newer);
//   one side lane + the trunk tail, or two and more side lanes -> lane 0, which first waits for those side lanes (join).
// A join that covers every side lane with work in flight ends the wave: all earlier launches are complete when the joining
// unit starts.  plan_shape() keeps a tensor alive to the end of the wave of its last reader, so recycled scratch adds no
// dependency inside a wave, and the schedule — true dependencies only — does not depend on the shape.
// Side lanes only ever wait on events of lane 0, and lane 0 on theirs: ROCm 7.x overflows its stack in
// hipStreamEndCapture when two non-origin streams of one capture have waited on each other (found with
// tools/ubench/segv_bt.c); fork/join through the origin stream captures fine (tools/ubench/graph_branches.hip).
void schedule_waves(esahrnet_ctx& c) {
    const size_t nops = c.ops.size();
    for (Op& o : c.ops) { o.lane = 0; o.wave = 0; o.wait0 = -1; o.wait_entry = false; o.record = false; o.join = 0; }
    c.nwaves = 1;
    if (c.opt.nlanes > 1) {
        std::vector<std::vector<int>> readers(c.tensors.size()), writers(c.tensors.size());
        std::vector<int> unit_end(nops, 0);       // op -> last op of its launch unit
        int wave = 0, wave_start = 0, tail0 = -1;
        int load[4], waited0[4], tail[4], joined_tail[4], joined_op[4];
        bool active[4];
        auto reset = [&]() {
            for (int l = 0; l < 4; ++l) { load[l] = 0; waited0[l] = -1; tail[l] = -1; joined_tail[l] = -1; joined_op[l] = -1; active[l] = false; }
        };
        reset();
        for (size_t k = 0; k < nops;) {
            size_t e = k + 1;
            while (e < nops && ((c.ops[k].job >= 0 && c.ops[e].job == c.ops[k].job) ||
                                (c.ops[k].multi >= 0 && c.ops[e].multi == c.ops[k].multi))) ++e;
            unsigned side = 0;
            int zmax = -1;
            auto dep = [&](int d) {
                if (d < wave_start || d >= (int)k) return;
                const int l = c.ops[d].lane;
                if (l == 0) zmax = std::max(zmax, unit_end[d]);
                else if (d <= joined_tail[l]) zmax = std::max(zmax, joined_op[l]);      // already joined into the trunk
                else side |= 1u << l;
            };
            for (size_t m = k; m < e; ++m) {
                const Op& o = c.ops[m];
                for (int t : {o.in, o.res, o.terms[0], o.terms[1], o.terms[2], o.terms[3]})
                    if (t >= 0) for (int w : writers[t]) dep(w);
                if (o.out >= 0) {
                    for (int r : readers[o.out]) dep(r);
                    for (int w : writers[o.out]) dep(w);
                }
            }
            Op& lead = c.ops[k];
            int lane = 0;
            const int nside = __builtin_popcount(side);
            if (nside >= 2 || (nside == 1 && zmax == tail0)) {
                lead.join = side;
                bool all = true;
                for (int l = 1; l < 4; ++l) if (active[l] && !(side >> l & 1)) all = false;
                if (all) {
                    ++wave; wave_start = (int)k; tail0 = -1;
                    reset();
                } else {
                    for (int l = 1; l < 4; ++l)
                        if (side >> l & 1) { active[l] = false; joined_tail[l] = tail[l]; joined_op[l] = (int)e - 1; }
                }
            } else if (nside == 1) {
                lane = __builtin_ctz(side);
            } else if (zmax != tail0) {
                lane = 1;
                for (int l = 2; l < 4; ++l) if (load[l] < load[lane]) lane = l;
            }
            if (lane) {
                if (zmax > waited0[lane]) { lead.wait0 = zmax; c.ops[zmax].record = true; waited0[lane] = zmax; }
                else if (waited0[lane] < 0 && tail[lane] < 0) lead.wait_entry = true;
                active[lane] = true;
            }
            ++load[lane];
            for (size_t m = k; m < e; ++m) {
                Op& o = c.ops[m];
                o.lane = lane; o.wave = wave;
                unit_end[m] = (int)e - 1;
                for (int t : {o.in, o.res, o.terms[0], o.terms[1], o.terms[2], o.terms[3]}) if (t >= 0) readers[t].push_back((int)m);
                if (o.out >= 0) writers[o.out].push_back((int)m);
            }
            tail[lane] = (int)e - 1;
            if (!lane) tail0 = (int)e - 1;
            k = e;
        }
        c.nwaves = wave + 1;
    }
    c.wave_last.assign(c.nwaves, 0);
    c.wave_mask.assign(c.nwaves, 0);
    for (size_t k = 0; k < nops; ++k) {
        c.wave_last[c.ops[k].wave] = (int)k;
        c.wave_mask[c.ops[k].wave] |= (unsigned char)(1u << c.ops[k].lane);
    }
}

int build_plan_ops(esahrnet_ctx& c);
int build_plan(esahrnet_ctx& c) {
    if (build_plan_ops(c)) return 1;
    group_multihead(c);
    group_jobs(c);
    schedule_waves(c);
    return 0;
}

int build_plan_ops(esahrnet_ctx& c) {
    const esahrnet_cfg& g = c.cfg;
    Builder B(c);
    const int sw = g.stem_width;
    // ---- stem (seg_hrnet.py:265-270, 426-431) ----
    c.spec_stem = B.spec("conv1", "bn1", g.cin, sw, 3, 1, 0, false, true);
    const int spec_conv2 = B.spec("conv2", "bn2", sw, sw, 3, 2, 1, false, true);
    int x;
    int stem_raw = -1;
    if (g.variant == 1) {   // seg_hrnet3.py:473-475: x0 = conv1(x0) is kept (pre-BN) for the CBAM skip: conv1 a second time
        Op o; o.kind = OP_STEMRAW; o.out = B.tensor(sw, 0, "stem_raw"); stem_raw = o.out;
        o.aux[0] = B.aux("conv1.weight", sw, g.cin, 3, 3); B.push(o);
    }
    if (c.opt.stem != STEM_SEPARATE) {  // conv1 + bn1 + ReLU recomputed per tile inside the conv2 kernel (stem_fused.hip / conv_x6.hip)
        DevConv d;
        d.spec = spec_conv2; d.c0 = 0; d.c1 = sw; d.use_bias = true;
        d.cinp = pad32(sw); d.coutp = pad32(sw);
        c.dconvs.push_back(d);
        Op o; o.kind = OP_STEMF; o.dconv = (int)c.dconvs.size() - 1; o.out = B.tensor(sw, 1, "stem2");
        B.push(o);
        x = o.out;
    } else {                // conv1 + bn1 + ReLU on the stem kernel, conv2 on the stream kernel
        Op o; o.kind = OP_STEM; o.out = B.tensor(sw, 0, "stem1");
        B.push(o);
        x = B.conv(spec_conv2, o.out, -1, true, "stem2");
    }
    // ---- layer1 (:277, :432) ----
    int cin = sw;
    const int nb1 = g.blocks[0][0];
    for (int k = 0; k < nb1; ++k) {
        x = B.basic_block("layer1." + std::to_string(k), x, cin, g.widths[0], 1, k == nb1 - 1 ? "layer1" : "");
        cin = g.widths[0];
    }
    std::vector<int> ys{x};
    std::vector<int> pre{g.widths[0]};
    for (int s = 2; s <= 4; ++s) {
        int nb = 0;
        while (nb < ESAHRNET_MAX_BRANCHES && g.blocks[s - 1][nb] > 0) ++nb;
        if (nb < (int)pre.size() || nb > (int)pre.size() + 1)
            return fail("stage %d: %d branches after %zu (must grow by at most one)", s, nb, pre.size());
        std::vector<int> cur(g.widths, g.widths + nb);
        const std::string t = "transition" + std::to_string(s - 1);
        // ---- transition (:343-377, wiring :434-457: new branch from ys.back()) ----
        std::vector<int> xs;
        for (int i = 0; i < nb; ++i) {
            if (i < (int)pre.size()) {
                if (pre[i] != cur[i]) {
                    const std::string q = t + "." + std::to_string(i);
                    xs.push_back(B.conv(B.spec(q + ".0", q + ".1", pre[i], cur[i], 3, 1, 1 + i, false, true), ys[i], -1, true));
                } else {
                    xs.push_back(ys[i]);
                }
            } else {
                int tt = ys.back();
                const int nconv = i + 1 - (int)pre.size();
                for (int j = 0; j < nconv; ++j) {
                    const std::string q = t + "." + std::to_string(i) + "." + std::to_string(j);
                    const int co = j == nconv - 1 ? cur[i] : pre.back();
                    tt = B.conv(B.spec(q + ".0", q + ".1", pre.back(), co, 3, 2, (int)pre.size() + j + 1, false, true), tt, -1, true);
                }
                xs.push_back(tt);
            }
        }
        // ---- HighResolutionModule x NUM_MODULES (:105-249) ----
        for (int m = 0; m < g.modules[s - 1]; ++m) {
            const std::string p = "stage" + std::to_string(s) + "." + std::to_string(m);
            for (int b = 0; b < nb; ++b) {
                for (int k = 0; k < g.blocks[s - 1][b]; ++k) {
                    // conv1 / conv2 of block k take keys 2k / 2k + 1 (seg_hrnet3: 6k .. 6k + 5 with the block's CBAM launches)
                    B.jkey = (((s << 4) | m) << 8) | ((g.variant == 1 ? 6 : 2) * k);
                    xs[b] = B.basic_block(p + ".branches." + std::to_string(b) + "." + std::to_string(k),
                                          xs[b], cur[b], cur[b], 1 + b, "");
                    B.jkey = -1;
                }
            }
            // fuse layers (:176-220, :232-247).  Emitted family by family, not output branch by output branch, so that
            // independent launches of one kernel family stand next to each other (group_jobs / group_multihead merge them):
            // all 1x1 fuse-up convolutions, then the stride-2 fuse-down chains link by link, then the sums.
            std::vector<std::vector<int>> terms(nb, std::vector<int>(nb, -1));
            const int modkey = ((s << 4) | m) << 8;
            for (int i = 0; i < nb; ++i) {
                terms[i][i] = xs[i];
                for (int j = i + 1; j < nb; ++j) {      // 1x1 + BN on the low-res grid; up-sampled inside fuse
                    const std::string q = p + ".fuse_layers." + std::to_string(i) + "." + std::to_string(j);
                    B.jkey2 = modkey | 100;             // all fuse-up 1x1 convolutions of the module are independent (before the chains)
                    terms[i][j] = B.conv(B.spec(q + ".0", q + ".1", cur[j], cur[i], 1, 1, 1 + j, false, false), xs[j], -1, false);
                    B.jkey2 = -1;
                }
            }
            for (int k = 0; k + 1 < nb; ++k)            // link k of every chain of 3x3 s2 (:198-217) that has one
                for (int i = k + 1; i < nb; ++i)
                    for (int j = 0; j + k < i; ++j) {
                        const bool last = k == i - j - 1;
                        const std::string qq = p + ".fuse_layers." + std::to_string(i) + "." + std::to_string(j) + "." + std::to_string(k);
                        const int sp_ = B.spec(qq + ".0", qq + ".1", cur[j], last ? cur[i] : cur[j], 3, 2, 1 + j + k + 1, false, !last);
                        B.jkey2 = modkey | (128 + k);
                        terms[i][j] = B.conv(sp_, k == 0 ? xs[j] : terms[i][j], -1, !last);
                        B.jkey2 = -1;
                    }
            std::vector<int> outs;
            for (int i = 0; i < nb; ++i) {
                const bool final_module = m == g.modules[s - 1] - 1;
                outs.push_back(B.fuse(terms[i], cur[i], 1 + i, true,
                                      final_module ? "stage" + std::to_string(s) + "." + std::to_string(i) : "",
                                      p + ".fuse." + std::to_string(i)));
            }
            xs = outs;
        }
        ys = xs;
        pre = cur;
    }
    // ---- head (:313-340, :461-469) ----
    int tot = 0;
    for (int v : pre) tot += v;
    const int K = g.num_keypoints;
    if (g.variant == 1) {
        // seg_hrnet3.py:363-383, 506-520: cat of the up-sampled branches (materialised: last_layer[0] is a
        // 3x3 conv here), 3x3 480->480, 1x1 480->K, up x2 (align_corners=True), cat with CBAM(stem skip),
        // 3x3 (K+64)->K.  The second concat is laid out [skip | heat-maps] so that both slices start on
        // an 8-channel group; output_layer's input channels are permuted accordingly when packed.
        // bf16 mode: the direct head below (no gather), and the output layer leaves its heat-maps in f32 (out_f32: the
        // stream kernel's f32 epilogue), as variant 0's bf16 output layer does.
        const int l0 = B.spec("last_layer.0", "last_layer.1", tot, tot, 3, 1, 1, true, true);
        const int l3 = B.spec("last_layer.3", "last_layer.4", tot, K, 1, 1, 1, true, true);
        c.spec_final = B.spec("output_layer.0", "", K + sw, K, 3, 1, 0, true, false);
        int h0, wide_h0 = 0;
        if (ys.size() == 4 && !c.h16() && !c.opt.head3_direct) {
            // last_layer[0] by linearity (head_gather.hip): branches 2, 3 as nine 1x1 products on their own grids + a gather,
            // branch 0 and the up-sampled branch 1 as a direct 3x3 that takes the gather's result as its residual
            const int cd = pre[0] + pre[1];
            const int cat = B.tensor(cd, 1, "head_cat");
            int off = 0;
            for (int b = 0; b < 2; ++b) {
                Op o; o.kind = OP_RESAMPLE; o.in = ys[b]; o.out = cat; o.c0 = off; o.nchan = pre[b]; o.align = 0;
                B.push(o);
                off += pre[b];
            }
            if (pad32(cd) > ((cd + 7) & ~7)) {
                Op o; o.kind = OP_ZERO; o.out = cat; o.terms[0] = cat; o.c0 = (cd + 7) & ~7; o.nchan = pad32(cd) - ((cd + 7) & ~7);
                B.push(o);
            }
            int z[2];
            for (int b = 2; b < 4; ++b) {
                const int zs = B.taps_spec(l0, off, off + pre[b], 1 + b);
                z[b - 2] = B.conv(zs, ys[b], -1, false, "", 0, -1, false, true);      // plain f32: the gather needs no join
                off += pre[b];
            }
            Op gop; gop.kind = OP_GATHER; gop.in = z[0]; gop.nterms = 1; gop.terms[0] = z[1];
            gop.out = B.tensor(tot, 1, "head_gather");
            B.push(gop);
            h0 = B.conv(l0, cat, gop.out, true, "head0", 0, cd);
            // 64-cout workgroup slices for the direct convolution: the stream kernel stages an input tile once per 64 instead of
            // once per 32 couts (480 = 7.5 x 64: the output, its residual and the reader's input are padded to 512 channels,
            // the padding is exact zeros end to end: zero weights, zero bias, zero residual)
            if (pad64(tot) != pad32(tot) && !c.opt.head3_cout32) {
                const int cp = pad64(tot);
                c.tensors[gop.out].Cp = cp;
                c.tensors[h0].Cp = cp;
                c.dconvs[c.ops.back().dconv].coutp = cp;
                wide_h0 = cp;
            }
        } else {
            const int cat = B.tensor(tot, 1, "head_cat");
            int off = 0;
            for (size_t b = 0; b < ys.size(); ++b) {
                Op o; o.kind = OP_RESAMPLE; o.in = ys[b]; o.out = cat; o.c0 = off; o.nchan = pre[b]; o.align = 0;
                B.push(o);
                off += pre[b];
            }
            if (c.padc(tot) > ((tot + 7) & ~7)) {
                Op o; o.kind = OP_ZERO; o.out = cat; o.terms[0] = cat; o.c0 = (tot + 7) & ~7; o.nchan = c.padc(tot) - ((tot + 7) & ~7);
                B.push(o);
            }
            h0 = B.conv(l0, cat, -1, true, "head0");
        }
        const int h3 = B.conv(l3, h0, -1, true, "head3");
        if (wide_h0) c.dconvs[c.ops.back().dconv].cinp = wide_h0;
        const int cat2 = B.tensor(sw + K, 0, "head_cat2");
        const int first_cbam_op = (int)c.ops.size();
        B.cbam("", stem_raw, sw, -1, false, cat2, 0);
        // the pooling over the raw stem tensor rides in the kernel that writes it (stem.hip: launch_stem_pool): that op also
        // owns the partials, sized for the slabs that kernel makes (one per row piece) instead of pool_partial's 64
        if (c.ops[first_cbam_op].kind == OP_POOL && c.ops[first_cbam_op].in == stem_raw && !c.opt.stem_pool_separate)
            for (Op& so : c.ops)
                if (so.kind == OP_STEMRAW) {
                    const int partial = c.ops[first_cbam_op].out;
                    so.out2 = partial;
                    c.tensors[partial].flat = esa::STEM_POOL_SLABS_MAX * c.tensors[stem_raw].Cp * 2;
                    c.stemraw_partial = partial;
                }
        { Op o; o.kind = OP_RESAMPLE; o.in = h3; o.out = cat2; o.terms[0] = cat2; o.c0 = sw; o.nchan = K; o.align = 1; B.push(o); }
        if (c.padc(sw + K) > sw + ((K + 7) & ~7)) {
            Op o; o.kind = OP_ZERO; o.out = cat2; o.terms[0] = cat2; o.c0 = sw + ((K + 7) & ~7); o.nchan = c.padc(sw + K) - o.c0;
            B.push(o);
        }
        const int oc = B.conv(c.spec_final, cat2, -1, false, "out_sb", 0, -1, true, c.h16());
        std::vector<int>& perm = c.dconvs[c.ops.back().dconv].perm;     // packed ci -> reference ci
        for (int i = 0; i < sw; ++i) perm.push_back(K + i);              // skip channels come second in the reference
        for (int i = 0; i < K; ++i) perm.push_back(i);
        { Op o; o.kind = OP_TONCHW; o.in = oc; B.push(o); }
        return 0;
    }
    const int l0 = B.spec("last_layer.0", "last_layer.1", tot, tot, 1, 1, 1, true, true);
    const int l3 = B.spec("last_layer.3", "last_layer.4", tot, K, 1, 1, 1, true, true);
    c.spec_final = B.spec("output_layer.0", "", K + g.cin, K, 3, 1, 0, true, false);
    int h3;
    if (c.opt.head == HEAD_SB) {
        // t_b = W_b x_b on branch b's grid (f32 NHWC), b = 1..3; W_0, bias, ReLU, last_layer[3..5]
        // and the up-sampling of the t_b all happen inside head_fused.hip
        c.spec_l0 = l0; c.spec_l3 = l3; c.head_c0 = pre[0];
        // Two alternatives, chosen per input shape (plan_shape): alt 2 = head_t.hip + head_fused2.hip
        // (interpolation on the matrix cores, t_1 never materialised) when its geometry checks pass,
        // alt 1 = f32 NHWC terms + head_fused.hip otherwise.  Both read the same packed W_b slices.
        Op o; o.kind = OP_HEAD; o.in = ys[0]; o.nterms = 3; o.alt = c.opt.head2 ? 1 : 0;
        int off = pre[0];
        int dslice[4] = {-1, -1, -1, -1};
        for (int b = 1; b < 4; ++b) {
            const int save = c.specs[l0].level;
            c.specs[l0].level = 1 + b;
            o.terms[b - 1] = B.conv(l0, ys[b], -1, false, "", off, off + pre[b], false, true);
            c.ops.back().alt = o.alt;
            c.tensors[o.terms[b - 1]].alt = o.alt;
            dslice[b] = c.ops.back().dconv;
            c.specs[l0].level = save;
            off += pre[b];
        }
        o.out = B.tensor(K, 1, "head3");
        c.tensors[o.out].Cp = (K + 15) & ~15;     // read only by head.hip: 16-channel pitch halves its traffic for K <= 16
        const int idx = (int)c.ops.size();
        c.tensors[o.out].def = idx;
        B.use(o.in, idx);
        for (int i = 0; i < 3; ++i) B.use(o.terms[i], idx);
        c.ops.push_back(o);
        h3 = o.out;
        if (c.opt.head2) {
            int tt[4] = {-1, -1, -1, -1};
            for (int b = 2; b < 4; ++b) {
                Op t; t.kind = OP_HEADT; t.in = ys[b]; t.dconv = dslice[b]; t.alt = 2;
                t.out = B.tensor(tot, 1 + b);
                c.tensors[t.out].tlayout = true;
                c.tensors[t.out].alt = 2;
                B.push(t);
                tt[b] = t.out;
            }
            Op q; q.kind = OP_HEAD2; q.in = ys[0]; q.nterms = 3; q.alt = 2; q.dconv = dslice[1];
            q.terms[0] = ys[1]; q.terms[1] = tt[2]; q.terms[2] = tt[3];
            q.out = h3;
            c.head2_op = B.push(q);
        }
    } else {
        // bf16 mode: the slices t_1..t_3 are shared by two alternatives, chosen per input shape (plan_shape):
        // alt 2 = head_fused_bf.hip (W0, interpolation, ReLU, last_layer[3] in one kernel) where its source-region
        // geometry holds, alt 1 = slice 0 + fuse + 1x1 (the 720-channel tensors materialised) otherwise
        // (fp32-grade mode: the same arrangement with head_x6.hip; f32 NHWC slices, ESAHRNET_X6_UNFUSED_HEAD=1 keeps alt 1)
        const bool bf_head = c.opt.head == HEAD_BF || c.opt.head == HEAD_X6;
        std::vector<int> hterms(ys.size(), -1);
        int off = 0;
        std::vector<int> offs;
        for (size_t b = 0; b < ys.size(); ++b) { offs.push_back(off); off += pre[b]; }
        for (size_t b = bf_head ? 1 : 0; b < ys.size(); ++b) {
            // the slice runs at branch b's own resolution: fix the output level of the slice conv
            const int save = c.specs[l0].level;
            c.specs[l0].level = 1 + (int)b;
            hterms[b] = B.conv(l0, ys[b], -1, false, "", offs[b], offs[b] + pre[b], b == 0);
            c.specs[l0].level = save;
        }
        int h3b = -1;
        if (bf_head) {
            const int first_alt1 = (int)c.ops.size();
            const int save = c.specs[l0].level;
            hterms[0] = B.conv(l0, ys[0], -1, false, "", 0, pre[0], true);
            c.specs[l0].level = save;
            c.spec_l0 = l0; c.spec_l3 = l3; c.head_c0 = pre[0];
            Op q; q.kind = OP_HEADBF; q.in = ys[0]; q.nterms = 3; q.alt = 2;
            for (int b = 1; b < 4; ++b) q.terms[b - 1] = hterms[b];
            q.out = B.tensor(K, 1, "head3_fused");
            c.tensors[q.out].Cp = K <= 16 ? 16 : 32;      // read only by the output-layer kernel
            c.tensors[q.out].alt = 2;
            h3b = q.out;
            // alternative 1 first (its ops and tensors carry alt = 1), then the fused op
            const int h0 = B.fuse(hterms, tot, 1, true, "head0");
            h3 = B.conv(l3, h0, -1, true, "head3");
            for (int k = first_alt1; k < (int)c.ops.size(); ++k) {
                c.ops[k].alt = 1;
                if (c.ops[k].out >= 0) c.tensors[c.ops[k].out].alt = 1;
            }
            c.head2_op = B.push(q);
        } else {
            const int h0 = B.fuse(hterms, tot, 1, true, "head0");
            h3 = B.conv(l3, h0, -1, true, "head3");
        }
        if (h3b >= 0) {
            Op o; o.kind = OP_FINAL; o.in = h3b; o.alt = 2;
            B.push(o);
            Op o1; o1.kind = OP_FINAL; o1.in = h3; o1.alt = 1;
            B.push(o1);
            return 0;
        }
    }
    {
        Op o; o.kind = OP_FINAL; o.in = h3;
        B.use(h3, (int)c.ops.size());
        c.ops.push_back(o);
    }
    return 0;
}

// ---- fp16 scale groups ------------------------------------------------------------------------------------
// With BatchNorm folded, seg_hrnet / seg_hrnet2 is convolution, bias, ReLU, sums and bilinear interpolation, all of which
// commute exactly with a power of two: tensor T may be stored as T * 2^-e if the next convolution's weights take 2^(e_in -
// e_out) and its bias 2^-e_out.  Tensors that reach each other WITHOUT convolution weights in between must share e: a
// residual and the sum it enters, the terms of a fuse sum and its result, the slices of last_layer[0] with the h0 the fused
// head forms from them in registers, the head3 of either head alternative (one output layer reads both).  Read off the op
// list, so every stage table gets its own groups.  Groups are numbered by their first tensor in plan order.
int build_scale_groups(esahrnet_ctx& c) {
    c.tgroup.assign(c.tensors.size(), -1);
    c.gnames.clear();
    c.exps.clear();
    if (c.cfg.variant != 0 || !c.h16()) return 0;
    std::vector<int> parent(c.tensors.size());
    for (size_t i = 0; i < parent.size(); ++i) parent[i] = (int)i;
    auto find = [&](int a) { while (parent[a] != a) a = parent[a] = parent[parent[a]]; return a; };
    auto join = [&](int a, int b) {
        if (a < 0 || b < 0) return;
        a = find(a); b = find(b);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);      // the root is the group's first tensor
    };
    int final_in = -1;
    for (const Op& o : c.ops) {
        switch (o.kind) {
            case OP_STEM: break;
            case OP_CONV: join(o.out, o.res); break;
            case OP_FUSE: for (int i = 0; i < o.nterms; ++i) join(o.out, o.terms[i]); break;
            case OP_HEADBF: for (int i = 1; i < o.nterms; ++i) join(o.terms[0], o.terms[i]); break;
            case OP_FINAL: join(final_in, o.in); final_in = o.in; break;
            default: return fail("scale groups: the plan holds an op (kind %d) the 16-bit formats of variant 0 do not have", (int)o.kind);
        }
    }
    std::vector<int> gid(c.tensors.size(), -1);
    for (size_t t = 0; t < c.tensors.size(); ++t) {
        if (c.tensors[t].flat || c.tensors[t].f32 || c.tensors[t].def < 0) continue;
        const int r = find((int)t);
        if (gid[r] < 0) { gid[r] = (int)c.gnames.size(); c.gnames.push_back(""); }
        c.tgroup[t] = gid[r];
    }
    // names: the branch stream a "stageS.I" tap belongs to, else a tap of the group (stem1, stem2, head0, head3), else the
    // convolution that writes the group's first tensor
    for (size_t t = 0; t < c.tensors.size(); ++t) {
        const int g = c.tgroup[t];
        if (g < 0) continue;
        const std::string& tap = c.tensors[t].tap;
        int s = 0, i = 0;
        char tail = 0;
        if (sscanf(tap.c_str(), "stage%d.%d%c", &s, &i, &tail) == 2) c.gnames[g] = "stream" + std::to_string(i);
        else if (c.gnames[g].empty() && !tap.empty() && tap.compare(0, 5, "conv:") != 0 && tap != "layer1" && tap != "head3_fused") c.gnames[g] = tap;
    }
    for (size_t t = 0; t < c.tensors.size(); ++t) {
        const int g = c.tgroup[t];
        if (g < 0 || !c.gnames[g].empty()) continue;
        const Op& o = c.ops[c.tensors[t].def];
        c.gnames[g] = o.kind == OP_CONV ? c.specs[c.dconvs[o.dconv].spec].name : "tensor" + std::to_string(t);
    }
    c.exps.assign(c.gnames.size(), 0);
    return 0;
}

// Where convolution `index` (a host spec) sits among the groups: the group its output is stored in (-1: none, the f32 heat-maps)
// and the group of each range of its input channels (-1: the f32 crop), ranges in channel order.
struct ScaleRange { int c0, c1, group; };
int scale_conv_info(const esahrnet_ctx& c, int index, int* out_group, std::vector<ScaleRange>& ranges) {
    ranges.clear();
    const ConvSpec& s = c.specs[index];
    if (c.gnames.empty()) return fail("scale groups: this handle has none (variant 0 with precision 1 or 3 only)");
    int og = -2;
    auto add = [&](int c0, int c1, int in_group, int out) -> int {
        if (og != -2 && og != out) return fail("scale groups: the outputs of '%s' lie in two groups", s.name.c_str());
        og = out;
        for (const ScaleRange& r : ranges)
            if (r.c0 == c0) return r.c1 == c1 && r.group == in_group ? 0 : fail("scale groups: input slices of '%s' disagree", s.name.c_str());
        ranges.push_back({c0, c1, in_group});
        return 0;
    };
    for (const Op& o : c.ops) {
        if (o.kind == OP_STEM && index == c.spec_stem) { if (add(0, s.cin, -1, c.tgroup[o.out])) return 1; }
        else if (o.kind == OP_FINAL && index == c.spec_final) {
            const int K = c.cfg.num_keypoints;
            if (add(0, K, c.tgroup[o.in], -1) || add(K, s.cin, -1, -1)) return 1;
        } else if (o.kind == OP_CONV && c.dconvs[o.dconv].spec == index) {
            const DevConv& d = c.dconvs[o.dconv];
            if (add(d.c0, d.c1, c.tgroup[o.in], c.tgroup[o.out])) return 1;
        } else if (o.kind == OP_HEADBF && index == c.spec_l0) {
            if (add(0, c.head_c0, c.tgroup[o.in], c.tgroup[o.terms[0]])) return 1;
        } else if (o.kind == OP_HEADBF && index == c.spec_l3) {
            if (add(0, s.cin, c.tgroup[o.terms[0]], c.tgroup[o.out])) return 1;
        }
    }
    std::sort(ranges.begin(), ranges.end(), [](const ScaleRange& a, const ScaleRange& b) { return a.c0 < b.c0; });
    int at = 0;
    for (const ScaleRange& r : ranges) { if (r.c0 != at) break; at = r.c1; }
    if (og == -2 || at != s.cin) return fail("scale groups: the plan does not cover the input channels of '%s'", s.name.c_str());
    *out_group = og;
    return 0;
}

// Convolution `index` as esahrnet_commit packs it: the host's folded weights with 2^(e_in - e_out) on every range of input
// channels and 2^-e_out on the bias — ldexpf, exact unless the result leaves f32's normal range.  shift_at (optional): the
// exponent each input channel's weights were given.
int scaled_conv(const esahrnet_ctx& c, int index, std::vector<float>& w, std::vector<float>& b, std::vector<int>* shift_at) {
    const ConvSpec& s = c.specs[index];
    w = s.w; b = s.b;
    if (shift_at) shift_at->assign(s.cin, 0);
    if (!c.scaled()) return 0;
    int og = -1;
    std::vector<ScaleRange> ranges;
    if (scale_conv_info(c, index, &og, ranges)) return 1;
    const int taps = s.k * s.k, eo = c.gexp(og);
    for (const ScaleRange& r : ranges) {
        const int sh = c.gexp(r.group) - eo;
        for (int ci = r.c0; ci < r.c1; ++ci) {
            if (shift_at) (*shift_at)[ci] = sh;
            if (!sh) continue;
            for (int co = 0; co < s.cout; ++co)
                for (int t = 0; t < taps; ++t) {
                    float& v = w[((size_t)co * s.cin + ci) * taps + t];
                    v = ldexpf(v, sh);
                }
        }
    }
    if (eo) for (float& v : b) v = ldexpf(v, -eo);
    for (float v : w)
        if (!std::isfinite(v)) return fail("commit: a weight of '%s' is not finite in f32 under its scale shift", s.name.c_str());
    for (float v : b)
        if (!std::isfinite(v)) return fail("commit: a bias of '%s' is not finite in f32 under its scale shift 2^%d", s.name.c_str(), -eo);
    return 0;
}

void level_dims(const esahrnet_ctx& c, int h, int w, std::vector<int>& lh, std::vector<int>& lw) {
    lh.assign(c.max_level + 1, 0);
    lw.assign(c.max_level + 1, 0);
    lh[0] = h; lw[0] = w;
    for (int l = 1; l <= c.max_level; ++l) { lh[l] = (lh[l - 1] + 1) / 2; lw[l] = (lw[l - 1] + 1) / 2; }
}

int check_shape(int n, int h, int w) {
    if (n <= 0) return fail("batch must be positive (got %d)", n);
    if (h < 16 || w < 16 || (h & 1) || (w & 1))
        return fail("crop %dx%d: height and width must be even and >= 16 "
                    "(UpsamplingBilinear2d(x2) output must match the crop, seg_hrnet.py:330,469)", h, w);
    return 0;
}

// Device address of tensor `t` in the workspace `ws`.  Without a workspace (the per-shape decisions, op_desc_get) launch
// parameters are built for their shapes and flags only, and every tensor points at one non-null placeholder: the
// *_supported() predicates and conv_kernel_name() test some pointers (res, the multi-head outputs) against nullptr.
char* tensor_ptr(const esahrnet_ctx& c, char* ws, int t) {
    static char placeholder;
    return ws ? ws + c.tensors[t].off : &placeholder;
}

// does this input shape run the second-generation head (ops with alt == 2)?
bool head2_for_shape(const esahrnet_ctx& c, const std::vector<int>& lh, const std::vector<int>& lw, bool* ulo) {
    if (c.head2_op < 0 || !c.opt.head2) return false;
    const Op& o = c.ops[c.head2_op];
    int th[3], tw[3];
    for (int i = 0; i < 3; ++i) {
        const int lv = c.tensors[o.terms[i]].level;
        th[i] = lh[lv]; tw[i] = lw[lv];
    }
    const Tensor& t0 = c.tensors[o.in];
    if (o.kind == OP_HEADBF && c.x6()) {
        if (ulo) *ulo = false;
        return esa::head_x6_supported(lh[t0.level], lw[t0.level], th, tw, t0.Cp, c.cfg.num_keypoints);
    }
    if (o.kind == OP_HEADBF) {
        if (ulo) *ulo = false;
        return esa::head_fused_bf_supported(lh[t0.level], lw[t0.level], th, tw, t0.Cp, c.cfg.num_keypoints);
    }
    return esa::head_fused2_supported(lh[t0.level], lw[t0.level], th, tw, t0.Cp, c.tensors[o.terms[0]].Cp,
                                      c.cfg.num_keypoints, ulo);
}

// ConvParams of the multi-head launch of group `m` (conv_s2c32.hip), from the leader's input
esa::ConvParams multi_params(const esahrnet_ctx& c, const Multi& m, const ShapePlan& sp, char* ws) {
    const Op& o0 = c.ops[m.op[0]];
    const Tensor& ti = c.tensors[o0.in];
    const Tensor& to = c.tensors[o0.out];
    esa::ConvParams p{};
    p.x = tensor_ptr(c, ws, o0.in);
    p.w = static_cast<const uint4*>(m.w); p.bias = m.bias;
    p.N = sp.n; p.H = sp.lh[ti.level]; p.W = sp.lw[ti.level]; p.OH = sp.lh[to.level]; p.OW = sp.lw[to.level];
    p.Cinp = ti.Cp; p.Coutp = m.coutp; p.nheads = m.n;
    for (int k = 0; k < m.n; ++k) {
        const Op& ok = c.ops[m.op[k]];
        p.yh[k] = tensor_ptr(c, ws, ok.out);
        p.hb[k + 1] = p.hb[k] + c.dconvs[ok.dconv].coutp;
        p.hrelu[k] = ok.relu;
    }
    return p;
}

// ConvParams of a convolution op at a shape
esa::ConvParams conv_params_of(const esahrnet_ctx& c, const Op& o, const ShapePlan& sp, char* ws) {
    const DevConv& d = c.dconvs[o.dconv];
    const Tensor& ti = c.tensors[o.in];
    const Tensor& to = c.tensors[o.out];
    esa::ConvParams p{};
    p.x = tensor_ptr(c, ws, o.in);
    p.y = tensor_ptr(c, ws, o.out);
    p.res = o.res >= 0 ? tensor_ptr(c, ws, o.res) : nullptr;
    p.w = static_cast<const uint4*>(d.w); p.bias = d.bias;
    p.N = sp.n; p.H = sp.lh[ti.level]; p.W = sp.lw[ti.level]; p.OH = sp.lh[to.level]; p.OW = sp.lw[to.level];
    p.Cinp = d.cinp; p.Coutp = d.coutp; p.relu = o.relu; p.out_f32 = d.out_f32 && !c.x6(); p.fmt = c.opt.fmt;      // (fp32-grade: every tensor is plain f32)
    p.x6_reload = c.opt.x6_reload_weights;
    return p;
}

// is this job group evaluated as ONE launch at this shape?  Every member must be a stream-kernel launch of its own
// there (the kernel serving a layer depends on the shape only, never on the grouping)
bool job_on_for(const esahrnet_ctx& c, const JobGroup& g, const ShapePlan& sp) {
    if (c.ops[g.op[0]].kind != OP_CONV) return true;        // CBAM groups: the merged kernel runs every shape its members run
    const ConvSpec& s0 = c.specs[c.dconvs[c.ops[g.op[0]].dconv].spec];
    esa::ConvParams ps[6];
    for (int k = 0; k < g.n; ++k) {
        ps[k] = conv_params_of(c, c.ops[g.op[k]], sp, nullptr);
        const ConvSpec& sk = c.specs[c.dconvs[c.ops[g.op[k]].dconv].spec];
        // fp32-grade mode: conv_x6_jobs_kernel serves every kernel size / stride of the module, but one per launch
        if (c.x6() ? sk.k != s0.k || sk.stride != s0.stride : s0.k != 1 && sk.stride != s0.stride) return false;
    }
    return esa::conv_group_mergeable(c.opt.fmt, ps, g.n, s0.k, s0.stride);
}

// The per-shape dispatch decisions: level sizes, the head generation, which multi-head and job groups run as one launch.
// plan_shape adds the workspace offsets of a forward to them; op_desc_get describes the launches they make.
ShapePlan shape_decisions(const esahrnet_ctx& c, int n, int h, int w) {
    ShapePlan sp;
    sp.n = n; sp.h = h; sp.w = w; sp.keep = c.keep;
    level_dims(c, h, w, sp.lh, sp.lw);
    sp.head2 = head2_for_shape(c, sp.lh, sp.lw, &sp.head2_ulo);
    sp.multi_on.assign(c.multis.size(), 0);
    for (size_t mi = 0; mi < c.multis.size(); ++mi)       // (depends on the shape only through the kernel's limits)
        sp.multi_on[mi] = esa::conv_s2c32_multi_supported(multi_params(c, c.multis[mi], sp, nullptr)) ? 1 : 0;
    sp.job_on.assign(c.jobs.size(), 0);
    for (size_t ji = 0; ji < c.jobs.size(); ++ji) sp.job_on[ji] = job_on_for(c, c.jobs[ji], sp) ? 1 : 0;
    return sp;
}

// CBAM's per-pixel maps and their 7x7 attention in one kernel (cbam.hip: cbam_spatial) where the channel-group count allows
// and the image has at least 32 of its 16 x 32 tiles (measured, batch 32: 128x128x32ch 69 -> 47 us, 256x256x64ch 448 -> 323 us,
// but 64x64 and smaller lose: too few workgroups, each walking a halo that is mostly padding).  The batch size is
// deliberately not part of the rule: the kernel serving a layer must not depend on it.
// slabs per image the stem kernel pools the raw seg_hrnet3 skip tensor into; 0: pool_partial does it (plan without the
// arrangement, or a crop whose rows make more slabs than the partials tensor reserves)
int stem_pools(const esahrnet_ctx& c, int height, int width) {
    if (c.stemraw_partial < 0) return 0;
    const int slabs = esa::stem_pool_slabs(c.cfg.cin, c.padc(c.cfg.stem_width), height, width);
    return slabs <= esa::STEM_POOL_SLABS_MAX ? slabs : 0;
}

bool cbam_fused(const esahrnet_ctx& c, int Cp, int hh, int ww) {
    return esa::cbam_spatial_supported(Cp) && ((hh + 15) / 16) * ((ww + 31) / 32) >= 32 && !c.opt.cbam_unfused;
}

// one CBAM launch as a job description (cbam.hip); kind < 0: nothing to launch (the maps formed inside cbam_spatial, the
// pooling of the raw stem tensor done by the stem kernel)
esa::CbamJob cbam_job(const esahrnet_ctx& c, const Op& o, const ShapePlan& sp, char* ws) {
    auto T = [&](int t) { return tensor_ptr(c, ws, t); };
    esa::CbamJob q{};
    q.kind = -1;
    const Tensor& tx = c.tensors[o.kind == OP_MLP ? o.terms[0] : o.in];
    const int hh = sp.lh[tx.level], ww = sp.lw[tx.level];
    q.ap.N = sp.n; q.ap.H = hh; q.ap.W = ww; q.ap.Cp = tx.Cp; q.ap.C = o.nchan; q.ap.fmt = c.opt.fmt;
    q.HW = hh * ww; q.P = std::min(esa::POOL_SLABS, q.HW); q.Cr = o.nchan / 16;
    switch (o.kind) {
        case OP_POOL:
            if (o.out == c.stemraw_partial && stem_pools(c, sp.h, sp.w)) break;       // made by the stem kernel
            q.kind = esa::CBAM_POOL; q.ap.x = T(o.in); q.partial = reinterpret_cast<float*>(T(o.out)); q.ap.C = tx.C;
            break;
        case OP_MLP:
            q.kind = esa::CBAM_MLP; q.partial = reinterpret_cast<float*>(T(o.in)); q.ca = reinterpret_cast<float*>(T(o.out));
            q.w0 = c.aux[o.aux[0]].dev; q.w2 = c.aux[o.aux[1]].dev;
            if (const int slabs = o.in == c.stemraw_partial ? stem_pools(c, sp.h, sp.w) : 0) q.P = slabs;   // the stem kernel's
            break;
        case OP_MAPS:
            if (cbam_fused(c, tx.Cp, hh, ww)) break;
            q.kind = esa::CBAM_MAPS; q.ap.x = T(o.in); q.ap.ca = reinterpret_cast<const float*>(T(o.terms[1]));
            q.maps = reinterpret_cast<float*>(T(o.out));
            break;
        default: {
            const Tensor& to = c.tensors[o.out];
            q.kind = cbam_fused(c, tx.Cp, hh, ww) ? esa::CBAM_SPATIAL : esa::CBAM_APPLY;
            q.ap.x = T(o.in); q.ap.res = o.res >= 0 ? T(o.res) : nullptr;
            q.ap.ca = reinterpret_cast<const float*>(T(o.terms[1])); q.ap.maps = reinterpret_cast<const float*>(T(o.terms[2]));
            q.ap.w_sa = c.aux[o.aux[2]].dev; q.ap.y = T(o.out);
            q.ap.y_pix_bytes = to.Cp * c.eb(); q.ap.y_c0 = o.c0; q.ap.relu = o.relu;
        }
    }
    return q;
}

// bytes the planner reserves for tensor `t` at a shape (a multiple of 256)
size_t tensor_bytes(const esahrnet_ctx& c, const ShapePlan& sp, const Tensor& t) {
    const size_t wpix = t.tlayout ? (size_t)esa::head_t_xp(sp.lw[t.level]) : (size_t)sp.lw[t.level];
    size_t b = t.flat ? (size_t)sp.n * t.flat * 4 : (size_t)sp.n * sp.lh[t.level] * wpix * t.Cp * (t.f32 ? 4 : c.eb());
    return (b + 255) & ~(size_t)255;
}

// first-fit interval allocator over op order; tensors die after their last use
int plan_shape(esahrnet_ctx& c, int n, int h, int w) {
    if (c.sp.n == n && c.sp.h == h && c.sp.w == w && c.sp.keep == c.keep) return 0;
    if (check_shape(n, h, w)) return 1;
    ShapePlan sp = shape_decisions(c, n, h, w);
    // seg_hrnet3's head by linearity (head_gather.hip) stages the tap-product windows of two branches in LDS: a shape it
    // cannot serve is refused HERE with a message, not by a failed launch in the middle of a forward
    for (const Op& o : c.ops)
        if (o.kind == OP_GATHER) {
            const Tensor& to = c.tensors[o.out];
            const int zt[2] = {o.in, o.terms[0]};
            int zh[2], zw[2];
            for (int b = 0; b < 2; ++b) { zh[b] = sp.lh[c.tensors[zt[b]].level]; zw[b] = sp.lw[c.tensors[zt[b]].level]; }
            if (!esa::head_gather_supported(sp.lh[to.level], sp.lw[to.level], zh, zw, to.Cp))
                return fail("crop %dx%d: the interpolation windows of seg_hrnet3's last_layer[0] do not fit the gather kernel's LDS "
                            "budget (set ESAHRNET_HEAD3_DIRECT=1 before creating the net for the direct 480-channel 3x3)", h, w);
        } else if (o.kind >= OP_POOL && o.kind <= OP_APPLY) {
            // a CBAM step, alone or in a merged launch: cbam_job_blocks holds the predicates of every CBAM launcher, and
            // none of them depends on the batch
            esa::CbamJob q = cbam_job(c, o, sp, nullptr);
            if (q.kind >= 0 && esa::cbam_job_blocks(q) < 1) {
                static const char* steps[] = {"channel pooling", "channel-attention MLP", "spatial maps", "apply", "spatial attention"};
                const std::string& a = c.aux[o.aux[0]].name;        // "<layer>.ca.fc.0.weight"; the stem skip's has no layer
                const std::string layer = a.size() > 15 ? "'" + a.substr(0, a.size() - 15) + "'" : "the stem skip";
                return fail("seg_hrnet3: no kernel serves the CBAM %s of %s at %d channels (%d padded)", steps[q.kind],
                            layer.c_str(), q.ap.C, q.ap.Cp);
            }
        }
    const int active_alt = sp.head2 ? 2 : 1;
    struct Free { size_t off, len; };
    std::vector<Free> free_list;
    size_t top = 0;
    auto bytes_of = [&](const Tensor& t) { return tensor_bytes(c, sp, t); };
    auto alloc = [&](size_t len) {
        for (size_t i = 0; i < free_list.size(); ++i)
            if (free_list[i].len >= len) {
                const size_t off = free_list[i].off;
                free_list[i].off += len; free_list[i].len -= len;
                if (!free_list[i].len) free_list.erase(free_list.begin() + i);
                return off;
            }
        const size_t off = top;
        top += len;
        return off;
    };
    auto release = [&](size_t off, size_t len) {
        free_list.push_back({off, len});
        std::sort(free_list.begin(), free_list.end(), [](const Free& a, const Free& b) { return a.off < b.off; });
        for (size_t i = 0; i + 1 < free_list.size();)
            if (free_list[i].off + free_list[i].len == free_list[i + 1].off) {
                free_list[i].len += free_list[i + 1].len;
                free_list.erase(free_list.begin() + i + 1);
            } else ++i;
        if (!free_list.empty() && free_list.back().off + free_list.back().len == top) {
            top = free_list.back().off;
            free_list.pop_back();
        }
    };
    const size_t nops = c.ops.size();
    size_t high = 0;
    std::vector<char> allocated(c.tensors.size(), 0);
    for (size_t oi = 0; oi < nops; ++oi) {
        const Op& o = c.ops[oi];
        const bool active = o.alt == 0 || o.alt == active_alt;
        if (active && o.out >= 0 && !allocated[o.out]) {         // (slice writers re-use the allocation)
            allocated[o.out] = 1;
            const size_t len = bytes_of(c.tensors[o.out]);
            const size_t off = alloc(len);
            c.tensors[o.out].off = off;
            high = std::max(high, std::max(top, off + len));
        }
        if (active && o.out2 >= 0 && !allocated[o.out2]) {
            allocated[o.out2] = 1;
            const size_t len = bytes_of(c.tensors[o.out2]);
            const size_t off = alloc(len);
            c.tensors[o.out2].off = off;
            high = std::max(high, std::max(top, off + len));
        }
        // a job group runs as ONE launch: what one member reads last must not be handed to another member's output, so a
        // tensor whose last reader sits inside a group stays alive until the group's last member
        // (and with lanes: until the last op of the wave, whose launches run concurrently)
        auto last_of = [&](const Tensor& t) {
            if (t.last < 0) return t.last;
            if (c.opt.nlanes > 1) return c.wave_last[c.ops[t.last].wave];
            if (c.ops[t.last].job >= 0) {
                const JobGroup& g = c.jobs[c.ops[t.last].job];
                return g.op[g.n - 1];
            }
            return t.last;
        };
        if (!c.keep)
            for (size_t ti = 0; ti < c.tensors.size(); ++ti) {
                Tensor& t = c.tensors[ti];
                if (allocated[ti] && last_of(t) == (int)oi) release(t.off, bytes_of(t));
            }
        high = std::max(high, top);
    }
    sp.bytes = high;
    c.sp = sp;
    return 0;
}

void free_weights(esahrnet_ctx& c) {
    for (DevConv& d : c.dconvs) {
        if (d.w) (void)hipFree(d.w);
        if (d.bias) (void)hipFree(d.bias);
        d.w = nullptr; d.bias = nullptr;
    }
    for (float** p : {&c.stem_w, &c.stem_b, &c.final_w, &c.final_b, &c.head_b0, &c.head_b3})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    for (void** p : {&c.head_w0, &c.head_w3, &c.final_wpk})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    for (AuxSpec& a : c.aux) if (a.dev) { (void)hipFree(a.dev); a.dev = nullptr; }
    for (Multi& m : c.multis) {
        if (m.w) (void)hipFree(m.w);
        if (m.bias) (void)hipFree(m.bias);
        m.w = nullptr; m.bias = nullptr;
    }
    for (float** p : {&c.stemraw_w, &c.stemraw_b}) if (*p) { (void)hipFree(*p); *p = nullptr; }
    for (std::vector<hipEvent_t>* v : {&c.wave_entry, &c.wave_end, &c.op_event}) {
        for (hipEvent_t& e : *v) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        v->clear();
    }
    for (int i = 0; i < 3; ++i) {
        if (c.side[i]) { (void)hipStreamDestroy(c.side[i]); c.side[i] = nullptr; }
    }
    c.committed = false;
}

}  // namespace

// conv1 of a stem: host f32 [cout][cin][3][3] -> the stem kernels' [coutp/8][cin][9][8] (stem.hip, stem_fused.hip), the channels
// cout .. coutp-1 zero.  The one packing of that layout: esahrnet_commit and the stem test entries all come through here.
std::vector<float> esa::pack_stem_w(const float* w, int cout, int cin, int coutp) {
    std::vector<float> out((size_t)coutp * cin * 9, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < 9; ++t)
                out[(((size_t)(co >> 3) * cin + ci) * 9 + t) * 8 + (co & 7)] = w[((size_t)co * cin + ci) * 9 + t];
    return out;
}

using esa::pack_stem_w;

// ============================================ C ABI ============================================
extern "C" {

const char* esahrnet_last_error(void) { return g_err; }
int esahrnet_abi_version(void) { return ESAHRNET_ABI_VERSION; }

int esahrnet_create(const esahrnet_cfg* cfg, int device, esahrnet_handle* out) {
    if (!cfg || !out) return fail("esahrnet_create: null argument");
    if (cfg->final_conv_kernel != 1) return fail("FINAL_CONV_KERNEL=%d unsupported (reference default 1)", cfg->final_conv_kernel);
    if (cfg->cin < 1 || cfg->cin > 4) return fail("cin=%d unsupported (1..4)", cfg->cin);
    if (cfg->num_keypoints < 1 || esa::final_kt(cfg->num_keypoints) < 0) return fail("num_keypoints=%d unsupported (1..32)", cfg->num_keypoints);
    if (cfg->stem_width < 1 || cfg->blocks[0][0] < 1) return fail("bad stem_width/blocks");
    if (cfg->variant != 0 && cfg->variant != 1) return fail("variant=%d unsupported (0: seg_hrnet/2, 1: seg_hrnet3)", cfg->variant);
    if (cfg->precision < 0 || cfg->precision > 3)
        return fail("precision=%d unsupported (0..3 — 0: split-bf16 'bf16x3', 1: bf16, 2: fp32-grade 'bf16x6', 3: fp16)", cfg->precision);
    if (cfg->precision == 3 && cfg->variant == 1)
        return fail("precision=3 (fp16) is not built for variant 1 (seg_hrnet3): its CBAM kernels have no fp16 form; "
                    "seg_hrnet / seg_hrnet2 take it, seg_hrnet3 takes 0, 1 or 2");
    if (cfg->variant == 1) {
        if (cfg->stem_width % 16) return fail("variant 1: stem_width must be a multiple of 16 (ChannelAttention ratio)");
        for (int b = 0; b < ESAHRNET_MAX_BRANCHES; ++b)
            if (cfg->blocks[3][b] > 0 && (cfg->widths[b] < 16 || cfg->widths[b] % 8))
                return fail("variant 1: branch widths must be >= 16 and multiples of 8 (got %d)", cfg->widths[b]);
    }
    for (int s = 1; s < 4; ++s)
        if (cfg->modules[s] < 1) return fail("NUM_MODULES of stage %d must be >= 1", s + 1);
    for (int b = 0; b < ESAHRNET_MAX_BRANCHES; ++b)
        if (cfg->blocks[3][b] > 0 && cfg->widths[b] < 1) return fail("width of branch %d must be positive", b);
    // the job keys of group_jobs pack (stage << 4 | module) above an 8-bit depth field in which the branch convolutions take
    // (2 or 6) * block + 0..5, the fuse-up 1x1s 100 and the fuse-down links 128 + k: reject stage tables that overflow either
    for (int s = 0; s < 4; ++s) {
        if (cfg->modules[s] > 15) return fail("NUM_MODULES of stage %d is %d (at most 15)", s + 1, cfg->modules[s]);
        for (int b = 0; b < ESAHRNET_MAX_BRANCHES; ++b)
            if ((cfg->variant == 1 ? 6 : 2) * cfg->blocks[s][b] + (cfg->variant == 1 ? 5 : 1) >= 100)
                return fail("NUM_BLOCKS of stage %d branch %d is %d (at most %d)", s + 1, b, cfg->blocks[s][b], cfg->variant == 1 ? 15 : 49);
    }
    esahrnet_ctx* c = new esahrnet_ctx();
    c->cfg = *cfg;
    c->device = device;
    c->format = esa::Format(cfg->precision);
    c->opt = plan_options(*cfg, c->format);
    // fp16 tensors reach the output layer through the matrix-core kernel only (head.hip final_mfma_kernel<.., HF>)
    if (c->hf() && !c->opt.final_mfma) {
        delete c;
        return fail("precision=3 (fp16) needs the matrix-core output layer: unset ESAHRNET_FINAL_VALU (num_keypoints=%d, cin=%d)",
                    cfg->num_keypoints, cfg->cin);
    }
    if (build_plan(*c) || build_scale_groups(*c)) { delete c; return 1; }
    *out = c;
    return 0;
}

int esahrnet_destroy(esahrnet_handle h) {
    if (!h) return 0;
    if (h->committed) { (void)hipSetDevice(h->device); }
    free_weights(*h);
    delete h;
    return 0;
}

int esahrnet_handle_device(esahrnet_handle h) { return h ? h->device : -1; }

int esahrnet_debug_devstate(int* kernel_device_entries, int* devices) {
    esa::dev_state_counts(kernel_device_entries, devices);
    return 0;
}

int esahrnet_debug_set_launch_limit(long long bytes) {
    esa::set_stream_launch_limit(bytes);
    return 0;
}

int esahrnet_debug_set_x6_grid_limit(int workgroups) {
    esa::set_x6_grid_limit(workgroups);
    return 0;
}

int esahrnet_debug_set_cu_limit(int cus) {
    esa::set_cu_limit(cus);
    return 0;
}

int esahrnet_debug_op_schedule(esahrnet_handle h, int index, int* wave, int* lane) {
    if (!h || !wave || !lane || index < 0 || index >= (int)h->ops.size()) return fail("debug_op_schedule: bad argument");
    *wave = h->ops[index].wave;
    *lane = h->ops[index].lane;
    return 0;
}

// the plan ops that run at the planned shape: the head alternative the shape does not take is left out
static std::vector<int> active_ops(const esahrnet_ctx& c) {
    std::vector<int> idx;
    for (size_t k = 0; k < c.ops.size(); ++k)
        if (c.ops[k].alt == 0 || c.ops[k].alt == (c.sp.head2 ? 2 : 1)) idx.push_back((int)k);
    return idx;
}

int esahrnet_debug_op_count(esahrnet_handle h, int n, int height, int width, int* count) {
    if (!h || !count) return fail("debug_op_count: null argument");
    if (plan_shape(*h, n, height, width)) return 1;
    *count = (int)active_ops(*h).size();
    return 0;
}

int esahrnet_debug_op_regions(esahrnet_handle h, int n, int height, int width, int k, esahrnet_debug_op* out) {
    if (!h || !out) return fail("debug_op_regions: null argument");
    if (plan_shape(*h, n, height, width)) return 1;
    const std::vector<int> idx = active_ops(*h);
    if (k < 0 || k >= (int)idx.size()) return fail("debug_op_regions: op %d out of range (%zu run at this shape)", k, idx.size());
    const Op& o = h->ops[idx[k]];
    memset(out, 0, sizeof *out);
    out->index = idx[k]; out->wave = o.wave; out->lane = o.lane;
    out->job = o.job >= 0 && h->sp.job_on[o.job] ? o.job : -1;
    out->multi = o.multi >= 0 && h->sp.multi_on[o.multi] ? o.multi : -1;
    // slice: by the op's KIND — resample_slice, zero_slice and the CBAM apply write at a channel offset into `out`; the apply of
    // a BasicBlock fills its tensor alone (c0 = 0) and is flagged all the same.  The report is the PLAN, which is what the
    // allocator sees, not the launches: an op that launches nothing at this shape (the CBAM maps inside cbam_spatial, a
    // group member evaluated by its leader) is listed with the tensors the plan gives it.
    const bool slice = o.kind == OP_APPLY || o.kind == OP_RESAMPLE || o.kind == OP_ZERO;
    const int ts[ESAHRNET_DEBUG_MAX_REGIONS] = {o.in, o.res, o.terms[0], o.terms[1], o.terms[2], o.terms[3], o.out, o.out2};
    // the pooled partials of the raw stem tensor have one writer per shape: the stem kernel, or the pooling step
    const bool stem_pooled = stem_pools(*h, height, width) > 0;
    for (int role = 0; role < ESAHRNET_DEBUG_MAX_REGIONS; ++role) {
        if (ts[role] < 0) continue;
        if (role == 7 && o.kind == OP_STEMRAW && !stem_pooled) continue;
        if (role == 6 && o.kind == OP_POOL && o.out == h->stemraw_partial && stem_pooled) continue;
        const Tensor& t = h->tensors[ts[role]];
        esahrnet_debug_region& r = out->regions[out->nregions++];
        r.tensor = ts[role]; r.role = role; r.write = role >= 6; r.slice = role == 6 && slice;
        r.offset = t.off; r.bytes = tensor_bytes(*h, h->sp, t);
    }
    return 0;
}

// the convolutions the host fills: derived specs (ConvSpec::parent) sit behind them and are filled at commit
static int host_specs(const esahrnet_ctx* h) { return h->nhost_specs >= 0 ? h->nhost_specs : (int)h->specs.size(); }
int esahrnet_conv_count(esahrnet_handle h) { return h ? host_specs(h) : -1; }

int esahrnet_conv_desc_get(esahrnet_handle h, int i, esahrnet_conv_desc* out) {
    if (!h || !out || i < 0 || i >= host_specs(h)) return fail("conv_desc_get: bad index %d", i);
    const ConvSpec& s = h->specs[i];
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", s.name.c_str());
    snprintf(out->bn, sizeof out->bn, "%s", s.bn.c_str());
    out->cin = s.cin; out->cout = s.cout; out->k = s.k; out->stride = s.stride;
    out->has_bias = s.has_bias; out->relu = s.relu;
    return 0;
}

int esahrnet_set_conv(esahrnet_handle h, int i, const float* w, const float* b) {
    if (!h || !w || !b || i < 0 || i >= host_specs(h)) return fail("set_conv: bad argument (index %d)", i);
    ConvSpec& s = h->specs[i];
    const size_t nw = (size_t)s.cout * s.cin * s.k * s.k;
    s.w.assign(w, w + nw);
    s.b.assign(b, b + s.cout);
    for (size_t j = 0; j < nw; ++j)
        if (!std::isfinite(s.w[j])) return fail("set_conv(%s): non-finite weight", s.name.c_str());
    s.set = true;
    return 0;
}

int esahrnet_aux_count(esahrnet_handle h) { return h ? (int)h->aux.size() : -1; }

int esahrnet_aux_desc_get(esahrnet_handle h, int i, esahrnet_aux_desc* out) {
    if (!h || !out || i < 0 || i >= (int)h->aux.size()) return fail("aux_desc_get: bad index %d", i);
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", h->aux[i].name.c_str());
    for (int k = 0; k < 4; ++k) out->shape[k] = h->aux[i].shape[k];
    return 0;
}

int esahrnet_set_aux(esahrnet_handle h, int i, const float* w) {
    if (!h || !w || i < 0 || i >= (int)h->aux.size()) return fail("set_aux: bad argument (index %d)", i);
    AuxSpec& a = h->aux[i];
    const size_t n = (size_t)a.shape[0] * a.shape[1] * a.shape[2] * a.shape[3];
    a.data.assign(w, w + n);
    for (float v : a.data) if (!std::isfinite(v)) return fail("set_aux(%s): non-finite value", a.name.c_str());
    a.set = true;
    return 0;
}

int esahrnet_commit(esahrnet_handle h) {
    if (!h) return fail("commit: null handle");
    for (ConvSpec& s : h->specs) {
        if (s.parent < 0) continue;
        const ConvSpec& ps = h->specs[s.parent];
        if (!ps.set) return fail("commit: weights of '%s' were never set", ps.name.c_str());
        s.w.assign((size_t)s.cout * s.cin, 0.f);
        s.b.assign(s.cout, 0.f);
        for (int co = 0; co < ps.cout; ++co)
            for (int t = 0; t < 9; ++t)
                for (int ci = 0; ci < s.cin; ++ci)
                    s.w[(size_t)((co >> 3) * 72 + t * 8 + (co & 7)) * s.cin + ci] = ps.w[((size_t)co * ps.cin + s.pc0 + ci) * 9 + t];
        s.set = true;
    }
    for (const ConvSpec& s : h->specs)
        if (!s.set) return fail("commit: weights of '%s' were never set", s.name.c_str());
    for (const AuxSpec& a : h->aux)
        if (!a.set) return fail("commit: tensor '%s' was never set", a.name.c_str());
    // the scale exponents (esahrnet_set_scale_exponents), applied in f32 before any packer runs: the specs hold the scaled
    // weights for the length of this call and get the host's back when it returns.  All zero: nothing is touched.
    struct Unfold {
        esahrnet_ctx* c;
        std::vector<std::vector<float>> w, b;
        ~Unfold() { for (size_t i = 0; i < w.size(); ++i) { c->specs[i].w.swap(w[i]); c->specs[i].b.swap(b[i]); } }
    } unfold{h, {}, {}};
    std::vector<std::vector<int>> shifts(h->specs.size());
    if (h->scaled()) {
        std::vector<std::vector<float>> w(h->specs.size()), b(h->specs.size());
        for (size_t i = 0; i < h->specs.size(); ++i)
            if (scaled_conv(*h, (int)i, w[i], b[i], &shifts[i])) return 1;
        for (size_t i = 0; i < h->specs.size(); ++i) { h->specs[i].w.swap(w[i]); h->specs[i].b.swap(b[i]); }
        unfold.w.swap(w); unfold.b.swap(b);
    }
    if (h->hf()) {      // a folded weight that rounds to +-inf in fp16 is refused, not saturated (conv1 and the output layer stay f32 / split bf16)
        for (size_t i = 0; i < h->specs.size(); ++i) {
            const ConvSpec& s = h->specs[i];
            if ((int)i == h->spec_stem || (int)i == h->spec_final) continue;
            for (size_t j = 0; j < s.w.size(); ++j)
                if (!esa::host_f16_finite(s.w[j]))
                    return fail("commit: weight %g of '%s' is not finite in fp16 (|w| must stay below 65520; scale shift 2^%d): precision "
                                "'fp16' cannot hold this network, use 'bf16'", (double)s.w[j], s.name.c_str(),
                                shifts[i].empty() ? 0 : shifts[i][(j / ((size_t)s.k * s.k)) % s.cin]);
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail("commit: no HIP device visible — the MI355X kernels cannot run (no CPU fallback exists)");
    HIP_OK(hipSetDevice(h->device));
    free_weights(*h);
    std::vector<char> packed;
    for (DevConv& d : h->dconvs) {
        const ConvSpec& s = h->specs[d.spec];
        const int cin = d.c1 - d.c0, taps = s.k * s.k;
        std::vector<float> w((size_t)s.cout * cin * taps);
        for (int co = 0; co < s.cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < taps; ++t) {
                    const int src_ci = d.perm.empty() ? d.c0 + ci : d.perm[ci];
                    w[((size_t)co * cin + ci) * taps + t] = s.w[((size_t)co * s.cin + src_ci) * taps + t];
                }
        if (upload(h->pack(w.data(), s.cout, cin, s.k, d.coutp, d.cinp), &d.w)) return 1;
        std::vector<float> bias(d.coutp, 0.f);
        if (d.use_bias) std::copy(s.b.begin(), s.b.end(), bias.begin());
        if (upload(bias, reinterpret_cast<void**>(&d.bias))) return 1;
    }
    for (Multi& m : h->multis) {     // members' packed weights / biases back to back (cout-tile major packing)
        size_t wbytes = 0;
        for (int k = 0; k < m.n; ++k) {
            const DevConv& d = h->dconvs[h->ops[m.op[k]].dconv];
            wbytes += esa::packed_weight_bytes(d.coutp, d.cinp, 3);
        }
        HIP_OK(hipMalloc(&m.w, wbytes));
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&m.bias), (size_t)m.coutp * sizeof(float)));
        size_t wo = 0, bo = 0;
        for (int k = 0; k < m.n; ++k) {
            const DevConv& d = h->dconvs[h->ops[m.op[k]].dconv];
            const size_t wb = esa::packed_weight_bytes(d.coutp, d.cinp, 3);
            HIP_OK(hipMemcpy(static_cast<char*>(m.w) + wo, d.w, wb, hipMemcpyDeviceToDevice));
            HIP_OK(hipMemcpy(m.bias + bo, d.bias, (size_t)d.coutp * sizeof(float), hipMemcpyDeviceToDevice));
            wo += wb; bo += d.coutp;
        }
    }
    {   // stem: [cout/8][cin][9][8]
        const ConvSpec& s = h->specs[h->spec_stem];
        const int coutp = h->padc(s.cout);
        std::vector<float> w = pack_stem_w(s.w.data(), s.cout, s.cin, coutp), b(coutp, 0.f);
        std::copy(s.b.begin(), s.b.begin() + s.cout, b.begin());
        if (h->opt.stem == STEM_FUSED_X6) {      // stem_x6_kernel reads conv1 in its own layout (bias inside)
            std::vector<float> wx(2 * 4 * 10 * 8, 0.f);
            esa::pack_stem_w1_x6(s.w.data(), s.b.data(), wx.data());
            w = wx;
        }
        if (upload(w, reinterpret_cast<void**>(&h->stem_w)) || upload(b, reinterpret_cast<void**>(&h->stem_b))) return 1;
    }
    if (h->cfg.variant == 0) {   // final: [K+cin][9][KT]
        const ConvSpec& s = h->specs[h->spec_final];
        const int kt = esa::final_kt(s.cout);
        std::vector<float> w((size_t)s.cin * 9 * kt, 0.f), b(std::max(kt, 32), 0.f);
        if (h->opt.final_mfma) {
            packed.assign(esa::final_mfma_bytes(s.cout, s.cin - s.cout), 0);
            esa::pack_final_mfma(s.w.data(), s.cout, s.cin - s.cout, packed.data());
            if (upload(packed, &h->final_wpk)) return 1;
        }
        for (int co = 0; co < s.cout; ++co) {
            b[co] = s.b[co];
            for (int ci = 0; ci < s.cin; ++ci)
                for (int t = 0; t < 9; ++t)
                    w[((size_t)ci * 9 + t) * kt + co] = s.w[((size_t)co * s.cin + ci) * 9 + t];
        }
        if (upload(w, reinterpret_cast<void**>(&h->final_w)) || upload(b, reinterpret_cast<void**>(&h->final_b))) return 1;
    }
    for (AuxSpec& a : h->aux)
        if (upload(a.data, reinterpret_cast<void**>(&a.dev))) return 1;
    for (const Op& o : h->ops)
        if (o.kind == OP_STEMRAW) {   // un-normalised conv1 in the stem kernel's [cout/8][cin][9][8] layout, zero bias
            const AuxSpec& a = h->aux[o.aux[0]];
            const int cout = a.shape[0], cin = a.shape[1], coutp = h->padc(cout);
            const std::vector<float> w = pack_stem_w(a.data.data(), cout, cin, coutp), b(coutp, 0.f);
            if (upload(w, reinterpret_cast<void**>(&h->stemraw_w)) || upload(b, reinterpret_cast<void**>(&h->stemraw_b))) return 1;
        }
    if (h->spec_l0 >= 0) {   // fused head: W0 slice (standard pack), W3 (permuted-K pack), biases
        const ConvSpec& s0 = h->specs[h->spec_l0];
        const ConvSpec& s3 = h->specs[h->spec_l3];
        const int ct = s0.cout, ctp = h->padc(ct), c0 = h->head_c0, c0p = h->padc(c0), c3p = pad32(s3.cout);
        std::vector<float> w((size_t)ct * c0);
        for (int co = 0; co < ct; ++co)
            for (int ci = 0; ci < c0; ++ci) w[(size_t)co * c0 + ci] = s0.w[(size_t)co * s0.cin + ci];
        if (upload(h->pack(w.data(), ct, c0, 1, ctp, c0p), &h->head_w0)) return 1;
        if (h->h16()) {
            packed.assign(esa::head_w3_bf_bytes(s3.cout, ctp), 0);
            esa::pack_head_w3_bf(s3.w.data(), s3.cout, ct, ctp, packed.data(), h->hf());
            if (upload(packed, &h->head_w3)) return 1;
        } else if (h->x6()) {      // head_x6.hip: W3 in conv_x6's three-term fragments (its K order is the h0 fragment's)
            const int m3p = s3.cout <= 16 ? 16 : 32;
            packed.assign(esa::packed_weight_bytes_x6(m3p, ctp, 1), 0);
            esa::pack_conv_weights_x6(s3.w.data(), s3.cout, ct, 1, m3p, ctp, packed.data());
            if (upload(packed, &h->head_w3)) return 1;
        } else {
            packed.assign(esa::head_w3_bytes(s3.cout, ctp), 0);
            esa::pack_head_w3(s3.w.data(), s3.cout, ct, ctp, packed.data());
            if (upload(packed, &h->head_w3)) return 1;
        }
        std::vector<float> b0(ctp, 0.f), b3(c3p, 0.f);
        std::copy(s0.b.begin(), s0.b.end(), b0.begin());
        std::copy(s3.b.begin(), s3.b.end(), b3.begin());
        if (upload(b0, reinterpret_cast<void**>(&h->head_b0)) || upload(b3, reinterpret_cast<void**>(&h->head_b3))) return 1;
    }
    if (h->opt.nlanes > 1) {     // side streams + events for the wave executor
        for (int i = 0; i < 3; ++i) HIP_OK(hipStreamCreateWithFlags(&h->side[i], hipStreamNonBlocking));
        h->wave_entry.assign(h->nwaves, nullptr);
        h->wave_end.assign((h->ops.size() + 1) * 3, nullptr);
        for (hipEvent_t& e : h->wave_entry) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (size_t k = 0; k <= h->ops.size(); ++k)
            for (int l = 1; l < 4; ++l)
                if (k == h->ops.size() || (h->ops[k].join >> l & 1))
                    HIP_OK(hipEventCreateWithFlags(&h->wave_end[k * 3 + l - 1], hipEventDisableTiming));
        h->op_event.assign(h->ops.size(), nullptr);
        for (size_t k = 0; k < h->ops.size(); ++k)
            if (h->ops[k].record) HIP_OK(hipEventCreateWithFlags(&h->op_event[k], hipEventDisableTiming));
    }
    h->committed = true;
    return 0;
}

// ---- fp16 scale groups: queries, exponents, the folded weights (host only) -------------------------------------------------
int esahrnet_scale_groups(esahrnet_handle h, int* groups) {
    if (!h || !groups) return fail("scale_groups: null argument");
    *groups = (int)h->gnames.size();
    return 0;
}

int esahrnet_scale_group_name(esahrnet_handle h, int group, char* out, size_t cap) {
    if (!h || !out || !cap) return fail("scale_group_name: null argument");
    if (group < 0 || group >= (int)h->gnames.size()) return fail("scale_group_name: group %d out of range (%zu groups)", group, h->gnames.size());
    snprintf(out, cap, "%s", h->gnames[group].c_str());
    return 0;
}

int esahrnet_scale_conv_get(esahrnet_handle h, int index, esahrnet_scale_conv* out) {
    if (!h || !out) return fail("scale_conv_get: null argument");
    if (index < 0 || index >= host_specs(h)) return fail("scale_conv_get: bad index %d", index);
    std::vector<ScaleRange> ranges;
    int og = -1;
    if (scale_conv_info(*h, index, &og, ranges)) return 1;
    if (ranges.size() > ESAHRNET_SCALE_MAX_RANGES) return fail("scale_conv_get: '%s' reads %zu ranges", h->specs[index].name.c_str(), ranges.size());
    memset(out, 0, sizeof *out);
    out->out_group = og;
    out->nranges = (int)ranges.size();
    for (size_t i = 0; i < ranges.size(); ++i) { out->c0[i] = ranges[i].c0; out->c1[i] = ranges[i].c1; out->in_group[i] = ranges[i].group; }
    return 0;
}

int esahrnet_scale_row_group(esahrnet_handle h, int row, int* group) {
    if (!h || !group) return fail("scale_row_group: null argument");
    const int nt = (int)h->tensors.size();
    if (row < 0 || row > nt) return fail("scale_row_group: row %d out of range (0..%d)", row, nt);
    *group = row == nt ? -1 : h->tgroup[row];
    return 0;
}

int esahrnet_set_scale_exponents(esahrnet_handle h, const int32_t* exponents, int count) {
    if (!h || (!exponents && count)) return fail("set_scale_exponents: null argument");
    if (count != (int)h->gnames.size())
        return fail("set_scale_exponents: %d exponents for a handle with %zu scale groups", count, h->gnames.size());
    for (int g = 0; g < count; ++g) {
        if (exponents[g] < -ESAHRNET_SCALE_MAX_EXPONENT || exponents[g] > ESAHRNET_SCALE_MAX_EXPONENT)
            return fail("set_scale_exponents: exponent %d of group %d ('%s') is outside [-%d, %d]", exponents[g], g, h->gnames[g].c_str(),
                        ESAHRNET_SCALE_MAX_EXPONENT, ESAHRNET_SCALE_MAX_EXPONENT);
        if (exponents[g] && h->cfg.precision != 3)
            return fail("set_scale_exponents: a non-zero exponent (group %d, '%s': %d) needs precision 3 (fp16); this handle has precision %d, "
                        "whose format has f32's exponent range", g, h->gnames[g].c_str(), exponents[g], h->cfg.precision);
    }
    h->exps.assign(exponents, exponents + count);
    h->committed = false;       // the packed weights on the device belong to the old exponents: esahrnet_commit again
    return 0;
}

int esahrnet_get_scale_exponents(esahrnet_handle h, int32_t* exponents, int count) {
    if (!h || (!exponents && count)) return fail("get_scale_exponents: null argument");
    if (count != (int)h->exps.size()) return fail("get_scale_exponents: room for %d exponents, the handle has %zu scale groups", count, h->exps.size());
    std::copy(h->exps.begin(), h->exps.end(), exponents);
    return 0;
}

int esahrnet_debug_scaled_conv(esahrnet_handle h, int index, float* w, float* b) {
    if (!h || !w || !b) return fail("debug_scaled_conv: null argument");
    if (index < 0 || index >= host_specs(h)) return fail("debug_scaled_conv: bad index %d", index);
    if (!h->specs[index].set) return fail("debug_scaled_conv: weights of '%s' were never set", h->specs[index].name.c_str());
    std::vector<float> sw, sb;
    if (scaled_conv(*h, index, sw, sb, nullptr)) return 1;
    std::copy(sw.begin(), sw.end(), w);
    std::copy(sb.begin(), sb.end(), b);
    return 0;
}

static int stats_row_name(esahrnet_handle h, int row, char* out, size_t cap);

int esahrnet_scale_exponents_from_stats(esahrnet_handle h, const void* records, int rows, int n_total, const void* h0_records,
                                        int headroom_bits, int32_t* exponents, int count) {
    if (!h || !records || !exponents) return fail("scale_exponents_from_stats: null argument");
    const int ng = (int)h->gnames.size();
    if (!ng) return fail("scale_exponents_from_stats: this handle has no scale groups (variant 0 with precision 1 or 3 only)");
    if (count != ng) return fail("scale_exponents_from_stats: room for %d exponents, the handle has %d scale groups", count, ng);
    if (rows != (int)h->tensors.size() + 1) return fail("scale_exponents_from_stats: %d rows, the handle's report has %zu", rows, h->tensors.size() + 1);
    if (n_total < 1) return fail("scale_exponents_from_stats: n_total must be positive (got %d)", n_total);
    if (headroom_bits < 0 || headroom_bits > 14) return fail("scale_exponents_from_stats: headroom_bits %d outside 0..14", headroom_bits);
    const esahrnet_stats_record* rec = static_cast<const esahrnet_stats_record*>(records);
    const esahrnet_stats_record* h0 = static_cast<const esahrnet_stats_record*>(h0_records);
    std::vector<float> top(ng, 0.f);
    char name[96];
    for (int r = 0; r < rows; ++r)
        for (int i = 0; i < n_total; ++i) {
            const esahrnet_stats_record& v = rec[(size_t)r * n_total + i];
            if (v.n_nan || v.n_inf) {
                if (stats_row_name(h, r, name, sizeof name)) snprintf(name, sizeof name, "?");
                return fail("scale_exponents_from_stats: row %d ('%s') holds %u NaN and %u infinite values in crop %d: no exponent cures that",
                            r, name, v.n_nan, v.n_inf, i);
            }
            const int g = r < rows - 1 ? h->tgroup[r] : -1;
            if (g >= 0 && std::isfinite(v.max_abs)) top[g] = std::max(top[g], v.max_abs);
        }
    if (h0) {
        int g0 = -1;
        for (const Op& o : h->ops)
            if (o.kind == OP_HEADBF) g0 = h->tgroup[o.terms[0]];
        for (size_t t = 0; t < h->tensors.size() && g0 < 0; ++t)
            if (h->tensors[t].tap == "head0") g0 = h->tgroup[t];
        for (int i = 0; i < n_total && g0 >= 0; ++i) {
            if (h0[i].n_nan || h0[i].n_inf)
                return fail("scale_exponents_from_stats: h0 holds %u NaN and %u infinite values in crop %d", h0[i].n_nan, h0[i].n_inf, i);
            if (std::isfinite(h0[i].max_abs)) top[g0] = std::max(top[g0], h0[i].max_abs);
        }
    }
    // M * 2^-e in (2^(14 - headroom), 2^(15 - headroom)]: e = ceil(log2 M) - (15 - headroom); frexp: M = m * 2^k, 0.5 <= m < 1
    for (int g = 0; g < ng; ++g) {
        int e = 0;
        if (top[g] > 0.f) {
            int k = 0;
            const float m = frexpf(top[g], &k);
            e = (m == 0.5f ? k - 1 : k) - (15 - headroom_bits);
            e = std::max(-ESAHRNET_SCALE_MAX_EXPONENT, std::min(ESAHRNET_SCALE_MAX_EXPONENT, e));
        }
        exponents[g] = e;
    }
    return 0;
}

int esahrnet_set_debug_keep(esahrnet_handle h, int keep) {
    if (!h) return fail("null handle");
    h->keep = keep != 0;
    return 0;
}

// kernel and (printf-formatted) label of an op description
__attribute__((format(printf, 3, 4)))
static void describe(esahrnet_op_desc* d, const char* kernel, const char* label, ...) {
    snprintf(d->kernel, sizeof d->kernel, "%s", kernel);
    va_list ap;
    va_start(ap, label);
    vsnprintf(d->label, sizeof d->label, label, ap);
    va_end(ap);
}

// What a forward leaves in caller memory in place of heat-maps: the decoder and where its results go.
// none (heat-maps), get_final, get_final2, the Gaussian fit, the M best peaks (get_final at each)
enum Decoder { DEC_NONE, DEC_FINAL, DEC_FINAL2, DEC_GAUSSFIT, DEC_CAND };
struct Request {
    Decoder decoder = DEC_NONE;
    float* kp = nullptr;        // f32 [n * K][3], never null
    int* idx = nullptr;         // int32 [n * K] (nullptr: not asked for)
    double* hess = nullptr;     // f64 [n * K][3], the Hessian each get_final2 step / the fit used (nullptr: not asked for)
    double* fit = nullptr;      // the Gaussian fit: f64 [n * K][8] (may be null) and int32 [n * K] (never null)
    int* status = nullptr;
    double* cov = nullptr;      // ... f64 [n * K][3] each, the covariance of the fitted centre and -cov^-1 (both nullptr: not
    double* info = nullptr;     // asked for, the kernels then compute what esahrnet_forward_keypoints_gaussfit computes)
    double cov_floor = 0.0;
    float* cand = nullptr;      // the candidates: f32 [n * K][M][3] (= kp, never null) and int32 [n * K][M] (= idx, may be null),
    int* cidx = nullptr;        // M in 1..ESAHRNET_MAX_CANDIDATES peaks per plane, r >= 0 pixels apart
    int M = 0, r = 0;
    int refine = -1;            // the candidates refined at their own pixels: the decoder of keypoints_at.hip (0..2) behind the
                                // search, its outputs in hess / fit / status / cov / info; -1: the plain search
};

// The one place a request is built, for the four forms the entries come in: (kp, idx), + hess, + fit and status, + cov, info and
// cov_floor.  Two rules are stated here and nowhere else: get_final computes no Hessian, so hess is ignored by it; cov and
// info belong to the Gaussian fit, and are ignored without it.  The candidates' form is (cand, cidx) in the place of (kp, idx),
// with M and r, and with `refine` (0..2) the decoder that refines every candidate and may write all of the other outputs.
static Request make_request(Decoder d, void* kp, void* idx, void* hess = nullptr, void* fit = nullptr, void* status = nullptr,
                            void* cov = nullptr, void* info = nullptr, double cov_floor = 0.0, int M = 0, int nms_radius = 0,
                            int refine = -1) {
    Request r;
    r.decoder = d;
    r.kp = static_cast<float*>(kp);
    r.idx = static_cast<int*>(idx);
    r.hess = d == DEC_FINAL ? nullptr : static_cast<double*>(hess);
    r.fit = static_cast<double*>(fit);
    r.status = static_cast<int*>(status);
    r.cov = d == DEC_GAUSSFIT || d == DEC_CAND ? static_cast<double*>(cov) : nullptr;
    r.info = d == DEC_GAUSSFIT || d == DEC_CAND ? static_cast<double*>(info) : nullptr;
    r.cov_floor = cov_floor;
    if (d == DEC_CAND) {
        r.cand = r.kp;
        r.cidx = r.idx;
        r.M = M;
        r.r = nms_radius;
        r.refine = refine;
    }
    return r;
}
static Request make_candidates_request(void* cand, void* cidx, int M, int nms_radius) {
    return make_request(DEC_CAND, cand, cidx, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, M, nms_radius);
}

// the device buffers of one forward (all nullptr when an op is only described)
struct Buffers {
    const void* x;
    void* heat;
    char* ws;
    void* part;
    // with a request the last op (OP_FINAL / OP_TONCHW) writes keypoints instead of heat-maps (heat == nullptr), through the
    // scratch behind the forward's workspace, carved as KpScratch lays it out.  kws: the bytes at kpart
    Request req;
    float* kheat = nullptr;
    float2* kpart = nullptr;
    float* kbmax = nullptr;
    size_t kws = 0;
    int* kcidx = nullptr;       // the refined candidates: the pixels of the candidates where the caller keeps none, and the
    void* kat = nullptr;        // workspace of the decoder at those pixels
    // esahrnet_forward_stats_h0: the fused 16-bit head runs in its range form (launch_head_bf_range) and leaves the range of h0
    void* h0_part = nullptr;
    void* h0_rec = nullptr;
};

// What a decoder keeps behind the forward's workspace (at ShapePlan::bytes, a multiple of 256), one row per decoder: heat,
// then part, then bmax.
//   get_final, Gaussian fit   the per-tile maxima of the output layer (part) and, where that is the matrix-core kernel, its
//                             heat-maps (that kernel writes them in any case)
//   get_final2                seg_hrnet3, get_final2's per-tile raw and blurred maxima of the NHWC heat-maps (part:
//                             esa::final2_workspace_bytes); the matrix-core output layer, its heat-maps and the same; the VALU
//                             output layer, the raw (part) and blurred (bmax) maxima of its 22 x 22 tiles
//   candidates                the heat-maps, for every network and precision: the runner-up rule needs whole planes
//   refined candidates        behind those heat-maps: cidx, the pixels of ESAHRNET_MAX_CANDIDATES candidates per plane (the
//                             query knows no M), then at, the workspace of keypoints_at.hip's decoder (get_final2 only)
// No N*K*H*W term but the matrix-core one and the candidates'.
struct KpScratch {
    int ntiles = 0;
    size_t heat = 0, part = 0, bmax = 0, cidx = 0, at = 0;
    size_t part_off() const { return heat; }
    size_t bmax_off() const { return heat + part; }
    size_t cidx_off() const { return heat + part + bmax; }
    size_t at_off() const { return heat + part + bmax + cidx; }
    size_t total() const { return heat + part + bmax + cidx + at; }
};
static KpScratch kp_scratch(const esahrnet_ctx& c, int n, int height, int width, Decoder d, int refine = -1) {
    KpScratch s;
    const int K = c.cfg.num_keypoints;
    const long long planes = (long long)n * K;
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    if (d == DEC_NONE) return s;
    if (d == DEC_CAND) {
        s.heat = pad((size_t)planes * height * width * 4);
        if (refine >= 0) {
            s.cidx = pad((size_t)planes * ESAHRNET_MAX_CANDIDATES * 4);
            s.at = esa::at_workspace_bytes(planes, height, width, refine);
        }
        return s;
    }
    if (c.cfg.variant != 1 && c.opt.final_mfma) s.heat = pad((size_t)planes * height * width * 4);
    if (d == DEC_FINAL2) {
        if (c.cfg.variant == 1 || c.opt.final_mfma) {
            s.ntiles = esa::final2_tiles(height, width);
            s.part = esa::final2_workspace_bytes(planes, height, width);
        } else {
            s.ntiles = esa::final2_valu_tiles(height, width);
            s.part = pad((size_t)planes * s.ntiles * 8);
            s.bmax = pad((size_t)planes * s.ntiles * 4);
        }
        return s;
    }
    s.ntiles = c.cfg.variant == 1 ? esa::to_nchw_part_tiles(height, width)
             : c.opt.final_mfma ? esa::final_part_tiles(K, c.cfg.cin, height, width)
                                : esa::final_kp_tiles(K, c.cfg.cin, height, width);
    s.part = pad((size_t)planes * s.ntiles * 8);
    return s;
}

// The decode step of a forward with a request: decoder x source of the maps.  The sources: fp == nullptr, seg_hrnet3's NHWC
// maps (`maps`, in format `fmt` with Cp channels per pixel); otherwise the output layer with the parameters *fp, the VALU
// kernel (it decodes behind its own tiles: no heat-maps at all) or the matrix-core one (heat-maps into the scratch, then the
// stand-alone decoder's kernels on them).  Returns what the failing launch returned, or 0.
static int run_decode(const esahrnet_ctx& c, const Buffers& b, const esa::FinalParams* fp, const char* maps, int fmt, int Cp, int n,
                      int height, int width, hipStream_t stream) {
    const Request& r = b.req;
    const int K = c.cfg.num_keypoints;
    const bool final2 = r.decoder == DEC_FINAL2, gaussfit = r.decoder == DEC_GAUSSFIT;
    esa::FinalParams p = fp ? *fp : esa::FinalParams{};
    if (r.decoder == DEC_CAND) {                    // whole planes into the scratch (the output layer, either kernel, or
        int rc;                                     // seg_hrnet3's conversion, with another destination), then the decoder
        if (fp) {
            p.out = b.kheat;
            p.part = nullptr;
            rc = esa::launch_final(p, stream);
        } else rc = esa::launch_fmt_to_nchw(fmt, maps, n, K, height, width, Cp, b.kheat, stream);
        if (rc) return rc;
        // refined: the decoder at every candidate's pixel behind the search (decoder 0 refines nothing: the search's rows are
        // its rows, and only a status asked for is left to write); the pixels go to the scratch where the caller keeps none
        const bool at = r.refine > 0 || (r.refine == 0 && r.status);
        int* const cidx = at && !r.cidx ? b.kcidx : r.cidx;
        rc = esa::launch_keypoints_candidates_auto(b.kheat, n * K, height, width, r.M, r.r, r.cand, cidx, stream);
        if (rc || !at) return rc;
        return esa::launch_keypoints_at(b.kheat, n * K, height, width, cidx, r.M, r.refine, r.cand, r.hess, r.fit, r.status, r.cov,
                                        r.info, r.cov_floor, b.kat, stream);
    }
    if (fp && !c.final_wpk) {
        p.out = nullptr;
        p.part = b.kpart;
        return final2 ? esa::launch_final2_kp(p, b.kbmax, r.kp, r.idx, stream, r.hess)
             : gaussfit ? esa::launch_final_gf_cov(p, r.kp, r.idx, r.fit, r.status, r.hess, r.cov, r.info, r.cov_floor, stream)
             : esa::launch_final_kp(p, r.kp, r.idx, stream);
    }
    int rc = 0;
    if (fp) {
        p.out = b.kheat;
        p.part = final2 ? nullptr : b.kpart;        // get_final2 takes its own tile maxima
        rc = esa::launch_final(p, stream);
        if (rc) return rc;
    }
    if (final2)
        return fp ? esa::launch_keypoints_final2(p.out, n * K, height, width, r.kp, r.idx, b.kpart, b.kws, stream, r.hess)
                  : esa::launch_keypoints_final2_nhwc(fmt, maps, n, K, height, width, Cp, r.kp, r.idx, b.kpart, b.kws, stream, r.hess);
    // get_final, and the Gaussian fit behind it: tile maxima, then the finish.  The fit reads the arg-max index: without idx it
    // passes through status
    int* const idx = gaussfit && !r.idx ? r.status : r.idx;
    if (fp)
        rc = esa::launch_keypoints_finish(p.out, p.part, esa::final_part_tiles(p.K, p.cin, height, width), n * K, height, width,
                                          r.kp, idx, stream);
    else {
        rc = esa::launch_tile_max(fmt, maps, n, K, height, width, Cp, b.kpart, stream);
        if (!rc)
            rc = esa::launch_keypoints_finish_nhwc(fmt, maps, n, K, height, width, Cp, b.kpart,
                                                   esa::to_nchw_part_tiles(height, width), r.kp, idx, stream);
    }
    if (rc || !gaussfit) return rc;
    return fp ? esa::launch_gaussfit_fit_cov(p.out, idx, n * K, height, width, r.kp, r.fit, r.status, r.hess, r.cov, r.info,
                                             r.cov_floor, stream)
              : esa::launch_gaussfit_fit_nhwc_cov(fmt, maps, n, K, height, width, Cp, idx, r.kp, r.fit, r.status, r.hess, r.cov,
                                                  r.info, r.cov_floor, stream);
}

// Op `o` at the shape `sp` decided: every dispatch decision is made here, once, and the launch parameters are built once.
// desc == nullptr: the op is launched on `stream`.  Otherwise nothing is launched and `desc` (zeroed by the caller) names
// that launch and counts its algorithmic FLOPs and compulsory HBM bytes; kernel "" when the op launches nothing of its own.
static int run_op(const esahrnet_ctx& c, const Op& o, const ShapePlan& sp, const Buffers& b, hipStream_t stream,
                  esahrnet_op_desc* desc) {
    const int n = sp.n, height = sp.h, width = sp.w;
    const std::vector<int>& lh = sp.lh;
    const std::vector<int>& lw = sp.lw;
    if (o.alt != 0 && o.alt != (sp.head2 ? 2 : 1)) {        // the head alternative not used at this shape
        if (desc) describe(desc, "", "(not used at this shape)");
        return 0;
    }
    auto T = [&](int t) { return tensor_ptr(c, b.ws, t); };
    auto tbytes = [&](int t) {
        const Tensor& x = c.tensors[t];
        const double wpix = x.tlayout ? (double)esa::head_t_xp(lw[x.level]) : (double)lw[x.level];
        return x.flat ? (double)n * x.flat * 4.0 : (double)n * lh[x.level] * wpix * x.Cp * (double)(x.f32 ? 4 : c.eb());
    };
    auto plain = [&](const char* kernel) {      // the seg_hrnet3 plumbing launches: what they read and write
        describe(desc, kernel, "seg_hrnet3");
        desc->bytes = (o.in >= 0 ? tbytes(o.in) : 0.0) + (o.out >= 0 ? tbytes(o.out) : 0.0);
    };
    int rc = 0;
    switch (o.kind) {
        case OP_STEM: {
            const ConvSpec& s = c.specs[c.spec_stem];
            esa::StemParams p{static_cast<const float*>(b.x), T(o.out), c.stem_w, c.stem_b,
                              n, height, width, c.cfg.cin, c.tensors[o.out].Cp, 1, c.opt.fmt};
            if (desc) {
                describe(desc, c.hf() ? "stem_kernel<fp16>" : "stem_kernel", "%s", s.name.c_str());
                desc->flops = 2.0 * n * height * width * s.cout * s.cin * 9;
                desc->bytes = (double)n * height * width * s.cin * 4 + tbytes(o.out);
            } else rc = esa::launch_stem(p, stream);
            break;
        }
        case OP_STEMRAW: {
            esa::StemParams p{static_cast<const float*>(b.x), T(o.out), c.stemraw_w, c.stemraw_b,
                              n, height, width, c.cfg.cin, c.tensors[o.out].Cp, 0, c.opt.fmt};
            if (desc) plain("stem_kernel(raw)");
            else rc = stem_pools(c, height, width) ? esa::launch_stem_pool(p, reinterpret_cast<float*>(T(o.out2)), stream)
                                                   : esa::launch_stem(p, stream);
            break;
        }
        case OP_POOL: case OP_MLP: case OP_MAPS: case OP_APPLY: {
            if (o.job >= 0 && sp.job_on[o.job]) {           // the same step of every branch of the module in one launch
                if (o.jpos > 0 && !desc) break;             // evaluated by the group's leader
                const JobGroup& g = c.jobs[o.job];
                esa::CbamJob js[esa::CBAM_MAXJOBS];
                int nj = 0;
                double bytes = 0.0;
                for (int k = 0; k < g.n; ++k) {
                    const Op& ok = c.ops[g.op[k]];
                    const esa::CbamJob q = cbam_job(c, ok, sp, b.ws);
                    if (q.kind < 0) continue;
                    js[nj++] = q;
                    if (desc) bytes += (ok.in >= 0 ? tbytes(ok.in) : 0.0) + (ok.out >= 0 ? tbytes(ok.out) : 0.0);
                }
                if (!desc) {
                    if (nj) rc = esa::launch_cbam_jobs(js, nj, stream);
                } else if (o.jpos > 0 || !nj) {
                    describe(desc, "", "seg_hrnet3 (%s)", nj ? "in the merged launch" : "inside cbam_spatial");
                } else {
                    static const char* names[] = {"cbam_jobs(pool)", "cbam_jobs(mlp)", "cbam_jobs(maps)", "cbam_jobs(apply)"};
                    describe(desc, names[o.kind - OP_POOL], "seg_hrnet3: %d branches", nj);
                    desc->bytes = bytes;
                }
                break;
            }
            const esa::CbamJob q = cbam_job(c, o, sp, b.ws);
            if (desc) {
                static const char* names[] = {"pool_partial", "ca_mlp", "cbam_maps", "cbam_apply", "cbam_spatial"};
                if (q.kind >= 0) plain(names[q.kind]);
                else describe(desc, "", "%s", o.kind == OP_POOL ? "seg_hrnet3 (inside stem_kernel(raw))" : "(inside cbam_spatial)");
                break;
            }
            switch (q.kind) {
                case esa::CBAM_POOL: rc = esa::launch_pool_partial(q.ap.x, q.partial, n, q.HW, q.ap.Cp, q.P, stream, c.opt.fmt); break;
                case esa::CBAM_MLP:
                    rc = esa::launch_ca_mlp(q.partial, q.w0, q.w2, q.ca, n, q.HW, q.ap.C, q.ap.Cp, q.Cr, q.P, stream);
                    break;
                case esa::CBAM_MAPS: rc = esa::launch_cbam_maps(q.ap.x, q.ap.ca, q.maps, n, q.HW, q.ap.C, q.ap.Cp, stream, c.opt.fmt); break;
                case esa::CBAM_APPLY: rc = esa::launch_cbam_apply(q.ap, stream); break;
                case esa::CBAM_SPATIAL: rc = esa::launch_cbam_spatial(q.ap, stream); break;
                default: break;
            }
            break;
        }
        case OP_RESAMPLE: {
            const Tensor& ti = c.tensors[o.in];
            const Tensor& to = c.tensors[o.out];
            esa::ResampleParams p{};
            p.x = T(o.in); p.y = T(o.out); p.N = n;
            p.h = lh[ti.level]; p.w = lw[ti.level]; p.H = lh[to.level]; p.W = lw[to.level];
            p.C = o.nchan; p.Cp_src = ti.Cp; p.y_pix_bytes = to.Cp * c.eb(); p.y_c0 = o.c0; p.align = o.align; p.fmt = c.opt.fmt;
            if (desc) plain("resample_slice");
            else rc = esa::launch_resample_slice(p, stream);
            break;
        }
        case OP_GATHER: {
            const Tensor& to = c.tensors[o.out];
            esa::GatherParams p{};
            const int zt[2] = {o.in, o.terms[0]};
            for (int k = 0; k < 2; ++k) {
                const Tensor& tz = c.tensors[zt[k]];
                p.z[k] = T(zt[k]); p.h[k] = lh[tz.level]; p.w[k] = lw[tz.level]; p.zpix[k] = tz.Cp * 4;
            }
            p.y = T(o.out); p.N = n; p.H = lh[to.level]; p.W = lw[to.level]; p.C = to.C; p.Cp = to.Cp;
            if (desc) {
                plain("head_gather");
                desc->bytes += tbytes(o.terms[0]);
            } else rc = esa::launch_head_gather(p, stream, c.opt.fmt);
            break;
        }
        case OP_ZERO: {
            const Tensor& to = c.tensors[o.out];
            if (desc) plain("zero_slice");
            else rc = esa::launch_zero_slice(T(o.out), (long long)n * lh[to.level] * lw[to.level], to.Cp * c.eb(), o.c0, o.nchan, stream, c.opt.fmt);
            break;
        }
        case OP_TONCHW: {
            const bool f32 = c.tensors[o.in].f32;       // (bf16 mode: the output layer's f32 heat-maps)
            const int fmt = f32 ? esa::FMT_F32 : c.opt.fmt;
            if (desc) plain(f32 ? "f32_to_nchw" : "sb_to_nchw");
            else if (b.req.decoder != DEC_NONE)         // keypoints instead of heat-maps: the decoder on the NHWC maps
                rc = run_decode(c, b, nullptr, T(o.in), fmt, c.tensors[o.in].Cp, n, height, width, stream);
            else if (b.part)                              // esahrnet_forward_partials: the same maps plus each tile's maximum
                rc = esa::launch_to_nchw_part(fmt, T(o.in), n, c.cfg.num_keypoints, height, width, c.tensors[o.in].Cp,
                                              static_cast<float*>(b.heat), static_cast<float2*>(b.part), stream);
            else rc = esa::launch_fmt_to_nchw(fmt, T(o.in), n, c.cfg.num_keypoints, height, width, c.tensors[o.in].Cp,
                                              static_cast<float*>(b.heat), stream);
            break;
        }
        case OP_STEMF: {
            const bool x6 = c.opt.stem == STEM_FUSED_X6;
            const DevConv& d = c.dconvs[o.dconv];
            const Tensor& to = c.tensors[o.out];
            esa::StemFusedParams p{};
            p.x = static_cast<const float*>(b.x); p.y = T(o.out);
            p.w1 = c.stem_w; p.bias1 = c.stem_b;
            p.w2 = static_cast<const uint4*>(d.w); p.bias2 = d.bias;
            p.N = n; p.H = height; p.W = width; p.OH = lh[to.level]; p.OW = lw[to.level];
            p.cin = c.cfg.cin; p.Cmid = d.cinp; p.Coutp = d.coutp;
            if (desc) {
                const ConvSpec& s1 = c.specs[c.spec_stem];
                const ConvSpec& s2 = c.specs[d.spec];
                describe(desc, x6 ? "stem_x6_kernel" : "stem_fused", "conv1 + conv2");
                desc->flops = 2.0 * n * height * width * s1.cout * s1.cin * 9 +
                              2.0 * n * lh[to.level] * lw[to.level] * s2.cout * s2.cin * 9;
                desc->bytes = (double)n * height * width * s1.cin * 4 + tbytes(o.out) +
                              (double)c.wbytes(pad32(s2.cout), pad32(s2.cin), 3);
            } else rc = x6 ? esa::launch_stem_fused_x6(p, stream) : esa::launch_stem_fused(p, stream);
            break;
        }
        case OP_CONV: {
            const DevConv& d = c.dconvs[o.dconv];
            const ConvSpec& s = c.specs[d.spec];
            const Tensor& ti = c.tensors[o.in];
            const Tensor& to = c.tensors[o.out];
            if (ti.Cp != d.cinp || to.Cp != d.coutp) return fail("plan bug: channel mismatch at %s", s.name.c_str());
            if (o.multi >= 0 && sp.multi_on[o.multi]) {
                if (o.mpos > 0) {                           // evaluated by the group's leader
                    if (desc) describe(desc, "", "%s (in the multi-head launch above)", s.name.c_str());
                    break;
                }
                const Multi& m = c.multis[o.multi];
                const esa::ConvParams p = multi_params(c, m, sp, b.ws);
                if (!desc) {
                    rc = esa::launch_conv_s2c32_multi(p, stream);
                    break;
                }
                std::string lab;
                desc->bytes = tbytes(o.in);
                for (int k = 0; k < m.n; ++k) {
                    const Op& ok = c.ops[m.op[k]];
                    const DevConv& dk = c.dconvs[ok.dconv];
                    const ConvSpec& sk = c.specs[dk.spec];
                    const Tensor& tk = c.tensors[ok.out];
                    lab += (k ? " + " : "") + sk.name;
                    desc->flops += 2.0 * n * lh[tk.level] * lw[tk.level] * sk.cout * sk.cin * 9.0;
                    desc->bytes += tbytes(ok.out) + (double)esa::packed_weight_bytes(dk.coutp, dk.cinp, 3);
                }
                describe(desc, m.coutp % 64 == 0 ? "conv_s2c32_kernel<2, 4, 4, true>" : "conv_s2c32_kernel<2, 4, 2, true>",
                         "%s", lab.c_str());
                break;
            }
            if (o.job >= 0 && sp.job_on[o.job]) {
                if (o.jpos > 0) {                           // evaluated by the group's leader
                    if (desc) describe(desc, "", "%s (in the merged launch above)", s.name.c_str());
                    break;
                }
                const JobGroup& g = c.jobs[o.job];
                esa::ConvParams ps[6];
                for (int k = 0; k < g.n; ++k) ps[k] = conv_params_of(c, c.ops[g.op[k]], sp, b.ws);
                if (!desc) {
                    rc = c.x6() ? esa::launch_conv_x6_jobs(ps, g.n, s.k, s.stride, stream)
                       : s.k == 1 ? esa::launch_conv1x1_jobs(ps, g.n, stream) : esa::launch_conv_jobs(ps, g.n, s.stride, stream);
                    break;
                }
                char kernel[sizeof desc->kernel];
                esa::conv_group_kernel_name(kernel, sizeof kernel, c.opt.fmt, ps, g.n, s.k, s.stride);
                std::string lab;
                for (int k = 0; k < g.n; ++k) {
                    const Op& ok = c.ops[g.op[k]];
                    const DevConv& dk = c.dconvs[ok.dconv];
                    const ConvSpec& sk = c.specs[dk.spec];
                    const Tensor& tk = c.tensors[ok.out];
                    lab += (k ? " + " : "") + sk.name;
                    desc->flops += 2.0 * n * lh[tk.level] * lw[tk.level] * sk.cout * sk.cin * (double)(sk.k * sk.k);
                    desc->bytes += tbytes(ok.in) + tbytes(ok.out) + (ok.res >= 0 ? tbytes(ok.res) : 0.0) +
                                   (double)c.wbytes(dk.coutp, dk.cinp, sk.k);
                }
                describe(desc, kernel, "%s", lab.c_str());
                break;
            }
            const esa::ConvParams p = conv_params_of(c, o, sp, b.ws);
            if (!desc) {
                rc = esa::launch_conv(p, s.k, s.stride, stream);
                break;
            }
            if (d.c0 != 0 || d.c1 != s.cin) describe(desc, esa::conv_kernel_name(p, s.k, s.stride), "%s[:, %d:%d]", s.name.c_str(), d.c0, d.c1);
            else describe(desc, esa::conv_kernel_name(p, s.k, s.stride), "%s", s.name.c_str());
            desc->flops = 2.0 * n * lh[to.level] * lw[to.level] * s.cout * (d.c1 - d.c0) * s.k * s.k;
            desc->bytes = tbytes(o.in) + tbytes(o.out) + (o.res >= 0 ? tbytes(o.res) : 0.0) +
                          (double)c.wbytes(d.coutp, d.cinp, s.k);
            break;
        }
        case OP_BLOCK: {
            const DevConv& d1 = c.dconvs[o.dconv];
            const DevConv& d2 = c.dconvs[o.dconv2];
            const Tensor& ti = c.tensors[o.in];
            const Tensor& to = c.tensors[o.out];
            if (ti.Cp != 32 || to.Cp != 32) return fail("plan bug: bblock32 on a non-32-channel tensor");
            esa::BlockParams p{};
            p.x = T(o.in); p.y = T(o.out);
            p.w1 = static_cast<const uint4*>(d1.w); p.w2 = static_cast<const uint4*>(d2.w);
            p.bias1 = d1.bias; p.bias2 = d2.bias;
            p.N = n; p.H = lh[ti.level]; p.W = lw[ti.level];
            if (desc) {
                const ConvSpec& s1 = c.specs[d1.spec];
                const ConvSpec& s2 = c.specs[d2.spec];
                describe(desc, "bblock32", "%s + conv2", s1.name.c_str());
                desc->flops = 2.0 * n * lh[to.level] * lw[to.level] * 9.0 * ((double)s1.cout * s1.cin + (double)s2.cout * s2.cin);
                desc->bytes = tbytes(o.in) + tbytes(o.out) + 2.0 * (double)esa::packed_weight_bytes(32, 32, 3);
            } else rc = esa::launch_bblock32(p, stream);
            break;
        }
        case OP_HEAD: case OP_HEADBF: {
            const Tensor& ti = c.tensors[o.in];
            const Tensor& to = c.tensors[o.out];
            esa::HeadParams p{};
            p.x0 = T(o.in); p.y = T(o.out);
            p.w0 = static_cast<const uint4*>(c.head_w0); p.w3 = static_cast<const uint4*>(c.head_w3);
            p.bias0 = c.head_b0; p.bias3 = c.head_b3;
            p.N = n; p.H = lh[ti.level]; p.W = lw[ti.level];
            for (int i = 0; i < 3; ++i) {
                const Tensor& tt = c.tensors[o.terms[i]];
                p.t[i] = T(o.terms[i]); p.th[i] = lh[tt.level]; p.tw[i] = lw[tt.level];
                p.Ctp = tt.Cp;
            }
            p.C0p = ti.Cp; p.C3p = to.Cp; p.K = c.cfg.num_keypoints; p.valu = c.opt.bf_head_valu && !c.hf(); p.hf = c.hf();
            if (desc) {
                const ConvSpec& s0 = c.specs[c.spec_l0];
                const ConvSpec& s3 = c.specs[c.spec_l3];
                describe(desc, o.kind == OP_HEAD ? "head_fused" : c.x6() ? "head_x6" : c.hf() ? "head_fused_bf<fp16>" : "head_fused_bf",
                         "last_layer.0[:, 0:%d] + up + last_layer.3", c.head_c0);
                desc->flops = 2.0 * n * lh[to.level] * lw[to.level] * ((double)s0.cout * c.head_c0 + (double)s3.cout * s3.cin);
                desc->bytes = tbytes(o.in) + tbytes(o.out);
                for (int i = 0; i < 3; ++i) desc->bytes += tbytes(o.terms[i]);
            } else if (o.kind == OP_HEADBF) {
                rc = c.x6() ? esa::launch_head_x6(p, stream)
                   : b.h0_rec ? esa::launch_head_bf_range(p, b.h0_part, b.h0_rec, stream) : esa::launch_head_bf(p, stream);
            } else {
                if (!esa::head_fused_supported(p.H, p.W, p.th, p.tw, p.C0p, p.K))
                    return fail("forward: fused head does not support this shape (%dx%d)", p.H, p.W);
                rc = esa::launch_head(p, stream);
            }
            break;
        }
        case OP_HEADT: {
            const Tensor& ti = c.tensors[o.in];
            const Tensor& to = c.tensors[o.out];
            const DevConv& d = c.dconvs[o.dconv];
            esa::HeadTParams p{};
            p.x = T(o.in); p.t = T(o.out); p.wt = static_cast<const uint4*>(d.w);
            p.N = n; p.h = lh[ti.level]; p.w = lw[ti.level];
            p.Cinp = ti.Cp; p.Ctp = to.Cp; p.XP = esa::head_t_xp(p.w);
            if (desc) {
                const ConvSpec& s = c.specs[d.spec];
                describe(desc, "head_t", "%s[:, %d:%d] (T layout)", s.name.c_str(), d.c0, d.c1);
                desc->flops = 2.0 * n * lh[ti.level] * lw[ti.level] * s.cout * (d.c1 - d.c0);
                desc->bytes = tbytes(o.in) + tbytes(o.out) + (double)esa::packed_weight_bytes(d.coutp, d.cinp, 1);
            } else rc = esa::launch_head_t(p, stream);
            break;
        }
        case OP_HEAD2: {
            const Tensor& ti = c.tensors[o.in];
            const Tensor& to = c.tensors[o.out];
            const DevConv& d1 = c.dconvs[o.dconv];
            esa::Head2Params p{};
            p.x0 = T(o.in); p.x1 = T(o.terms[0]); p.t2 = T(o.terms[1]); p.t3 = T(o.terms[2]); p.y = T(o.out);
            p.w0 = static_cast<const uint4*>(c.head_w0); p.w3 = static_cast<const uint4*>(c.head_w3);
            p.w1 = static_cast<const uint4*>(d1.w);
            p.bias0 = c.head_b0; p.bias3 = c.head_b3;
            p.N = n; p.H = lh[ti.level]; p.W = lw[ti.level];
            for (int i = 0; i < 3; ++i) {
                const Tensor& tt = c.tensors[o.terms[i]];
                p.th[i] = lh[tt.level]; p.tw[i] = lw[tt.level];
            }
            p.xp2 = esa::head_t_xp(p.tw[1]); p.xp3 = esa::head_t_xp(p.tw[2]);
            p.C0p = ti.Cp; p.C1p = c.tensors[o.terms[0]].Cp; p.Ctp = c.tensors[o.terms[1]].Cp;
            p.C3p = to.Cp; p.K = c.cfg.num_keypoints;
            if (desc) {
                const ConvSpec& s0 = c.specs[c.spec_l0];
                const ConvSpec& s3 = c.specs[c.spec_l3];
                const Tensor& t1 = c.tensors[o.terms[0]];
                describe(desc, "head_fused2", "last_layer.0[:, 0:%d] + up (MFMA) + last_layer.3", d1.c1);
                desc->flops = 2.0 * n * lh[to.level] * lw[to.level] * ((double)s0.cout * c.head_c0 + (double)s3.cout * s3.cin) +
                              2.0 * n * lh[t1.level] * lw[t1.level] * (double)s0.cout * (d1.c1 - d1.c0);
                desc->bytes = tbytes(o.in) + tbytes(o.out);
                for (int i = 0; i < 3; ++i) desc->bytes += tbytes(o.terms[i]);
            } else rc = esa::launch_head2(p, sp.head2_ulo, stream);
            break;
        }
        case OP_FUSE: {
            const Tensor& to = c.tensors[o.out];
            esa::FuseParams p{};
            p.nterms = o.nterms;
            for (int i = 0; i < o.nterms; ++i) {
                const Tensor& ti = c.tensors[o.terms[i]];
                if (ti.Cp != to.Cp) return fail("plan bug: fuse channel mismatch");
                p.x[i] = T(o.terms[i]); p.h[i] = lh[ti.level]; p.w[i] = lw[ti.level];
            }
            p.y = T(o.out); p.N = n; p.H = lh[to.level]; p.W = lw[to.level]; p.Cp = to.Cp;
            p.relu = o.relu; p.fmt = c.opt.fmt;
            if (desc) {
                describe(desc, c.hf() ? "fuse_kernel<fp16>" : "fuse_kernel", "fuse -> %s", to.tap.c_str());
                desc->bytes = tbytes(o.out);
                for (int i = 0; i < o.nterms; ++i) desc->bytes += tbytes(o.terms[i]);
            } else rc = esa::launch_fuse(p, stream);
            break;
        }
        case OP_FINAL: {
            const Tensor& ti = c.tensors[o.in];
            esa::FinalParams p{};
            p.h3 = T(o.in); p.x0 = static_cast<const float*>(b.x); p.out = static_cast<float*>(b.heat);
            p.w = c.final_w; p.bias = c.final_b; p.wpk = static_cast<const uint4*>(c.final_wpk);
            p.N = n; p.H = height; p.W = width; p.h = lh[ti.level]; p.wd = lw[ti.level];
            p.K = c.cfg.num_keypoints; p.cin = c.cfg.cin; p.Cp = ti.Cp; p.fmt = c.opt.fmt;
            p.part = static_cast<float2*>(b.part);
            if (desc) {
                const ConvSpec& s = c.specs[c.spec_final];
                describe(desc, c.hf() ? "final_kernel<fp16>" : "final_kernel", "%s", s.name.c_str());
                desc->flops = 2.0 * n * height * width * s.cout * s.cin * 9;
                desc->bytes = tbytes(o.in) + (double)n * height * width * (c.cfg.cin + s.cout) * 4;
            } else if (b.req.decoder != DEC_NONE)       // keypoints instead of heat-maps: the decoder in or behind the output layer
                rc = run_decode(c, b, &p, nullptr, 0, 0, n, height, width, stream);
            else rc = esa::launch_final(p, stream);
            break;
        }
    }
    if (rc) return fail("forward: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

// req == nullptr: heat-maps into heat_dev (and, with part_dev, their per-tile maxima).  Otherwise the decoder of *req runs in
// place of the last launch and nothing but its outputs reaches caller memory (heat_dev and part_dev unused, req->kp never null)
static int run_forward(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* part_dev,
                       void* ws_dev, size_t ws_bytes, esahrnet_stream stream_, hipEvent_t* events, const Request* req,
                       void* h0_part = nullptr, void* h0_rec = nullptr) {
    if (!h || !x_dev || !(heat_dev || req) || !ws_dev) return fail("forward: null argument");
    if (!h->committed) return fail("forward: esahrnet_commit has not been called");
    if (plan_shape(*h, n, height, width)) return 1;
    const KpScratch ks = kp_scratch(*h, n, height, width, req ? req->decoder : DEC_NONE, req ? req->refine : -1);
    const size_t need = h->sp.bytes + ks.total();
    if (ws_bytes < need) return fail("forward: workspace too small (%zu < %zu)", ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(ws_dev) & 255) return fail("forward: workspace must be 256-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Buffers bufs{x_dev, heat_dev, static_cast<char*>(ws_dev), part_dev};
    bufs.h0_part = h0_part; bufs.h0_rec = h0_rec;
    if (req) {
        char* const scratch = bufs.ws + h->sp.bytes;
        bufs.req = *req;
        bufs.kheat = reinterpret_cast<float*>(scratch);
        bufs.kpart = reinterpret_cast<float2*>(scratch + ks.part_off());
        bufs.kbmax = reinterpret_cast<float*>(scratch + ks.bmax_off());
        bufs.kws = ks.part;
        bufs.kcidx = reinterpret_cast<int*>(scratch + ks.cidx_off());
        bufs.kat = scratch + ks.at_off();
    }
    int op_index = 0;
    if (events && hipEventRecord(events[0], stream) != hipSuccess) return fail("forward: hipEventRecord failed");
    // wave executor: lane 0 is the caller's stream; the other lanes of a wave are side streams that fork from and join
    // into it (also valid under stream capture: the graph gets parallel branches).  The timed and the
    // keep-intermediates modes stay on one stream.
    const bool multi = !events && !h->keep && h->opt.nlanes > 1 && h->side[0] != nullptr;
    const hipStream_t caller = stream;
    bool lane_used[4] = {true, false, false, false};
    int cur_wave = -1;
    auto join = [&](size_t slot, unsigned lanes) -> int {      // the caller's stream continues behind those side lanes
        for (int l = 1; l < 4; ++l)
            if ((lanes >> l & 1) && lane_used[l]) {
                hipEvent_t e = h->wave_end[slot * 3 + l - 1];
                if (hipEventRecord(e, h->side[l - 1]) != hipSuccess || hipStreamWaitEvent(caller, e, 0) != hipSuccess) return 1;
                lane_used[l] = false;
            }
        return 0;
    };
    for (const Op& o : h->ops) {
        if (multi) {
            if (o.join && join((size_t)op_index, o.join)) return fail("forward: joining side lanes failed");
            if (o.wave != cur_wave) {
                cur_wave = o.wave;
                if (h->wave_mask[cur_wave] & ~1u) HIP_OK(hipEventRecord(h->wave_entry[cur_wave], caller));
            }
            stream = o.lane == 0 ? caller : h->side[o.lane - 1];
            lane_used[o.lane] = true;
            if (o.wait_entry) HIP_OK(hipStreamWaitEvent(stream, h->wave_entry[cur_wave], 0));
            if (o.wait0 >= 0) HIP_OK(hipStreamWaitEvent(stream, h->op_event[o.wait0], 0));
        }
        if (run_op(*h, o, h->sp, bufs, stream, nullptr)) return 1;
        if (multi && o.record) HIP_OK(hipEventRecord(h->op_event[op_index], caller));
        ++op_index;
        if (events && hipEventRecord(events[op_index], stream) != hipSuccess) return fail("forward: hipEventRecord failed");
    }
    if (multi && join(h->ops.size(), 0xeu)) return fail("forward: joining the side lanes failed");
    return 0;
}

int esahrnet_forward(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                     void* heat_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    return run_forward(h, x_dev, n, height, width, heat_dev, nullptr, ws_dev, ws_bytes, stream, nullptr, nullptr);
}

int esahrnet_forward_timed(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                           void* heat_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream,
                           float* ms_out) {
    if (!h || !ms_out) return fail("forward_timed: null argument");
    const size_t nops = h->ops.size();
    std::vector<hipEvent_t> ev(nops + 1, nullptr);
    hipEvent_t nul[2] = {nullptr, nullptr};
    int rc = 0;
    for (size_t i = 0; i <= nops && !rc; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = fail("forward_timed: hipEventCreate failed");
    for (int i = 0; i < 2 && !rc; ++i)
        if (hipEventCreate(&nul[i]) != hipSuccess) rc = fail("forward_timed: hipEventCreate failed");
    // the cost of an empty event bracket on this stream is measured and subtracted, so that the
    // per-launch figures are kernel time (comparable with rocprofv3 --kernel-trace), not kernel + marker
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!rc && (hipEventRecord(nul[0], st) != hipSuccess || hipEventRecord(nul[1], st) != hipSuccess))
        rc = fail("forward_timed: hipEventRecord failed");
    if (!rc) rc = run_forward(h, x_dev, n, height, width, heat_dev, nullptr, ws_dev, ws_bytes, stream, ev.data(), nullptr);
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail("forward_timed: stream sync failed");
    float null_ms = 0.f;
    if (!rc && hipEventElapsedTime(&null_ms, nul[0], nul[1]) != hipSuccess) rc = fail("forward_timed: hipEventElapsedTime failed");
    for (size_t i = 0; i < nops && !rc; ++i) {
        if (hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]) != hipSuccess) rc = fail("forward_timed: hipEventElapsedTime failed");
        ms_out[i] = ms_out[i] > null_ms ? ms_out[i] - null_ms : 0.f;
    }
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : nul) if (e) (void)hipEventDestroy(e);
    return rc;
}

int esahrnet_op_desc_get(esahrnet_handle h, int index, int n, int height, int width, esahrnet_op_desc* out) {
    if (!h || !out || index < 0 || index >= (int)h->ops.size()) return fail("op_desc_get: bad argument");
    if (check_shape(n, height, width)) return 1;
    memset(out, 0, sizeof *out);
    return run_op(*h, h->ops[index], shape_decisions(*h, n, height, width), Buffers{}, nullptr, out);
}

int esahrnet_partial_tiles(esahrnet_handle h, int height, int width, int* ntiles) {
    if (!h || !ntiles) return fail("partial_tiles: null argument");
    if (!h->committed) return fail("partial_tiles: esahrnet_commit has not been called");
    *ntiles = 0;
    // seg_hrnet / seg_hrnet2: the matrix-core output-layer kernel reports per-tile maxima, the VALU one none;
    // seg_hrnet3: the conversion of its heat-maps to NCHW does, in every precision
    if (h->cfg.variant == 0 && h->final_wpk)
        *ntiles = esa::final_part_tiles(h->cfg.num_keypoints, h->cfg.cin, height, width);
    else if (h->cfg.variant == 1)
        *ntiles = esa::to_nchw_part_tiles(height, width);
    return 0;
}

int esahrnet_forward_partials(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev,
                              void* part_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    int nt = 0;
    if (part_dev) {
        if (esahrnet_partial_tiles(h, height, width, &nt)) return 1;
        if (nt <= 0) return fail("forward_partials: this handle's output layer does not report per-tile maxima (esahrnet_partial_tiles = 0)");
    }
    return run_forward(h, x_dev, n, height, width, heat_dev, part_dev, ws_dev, ws_bytes, stream, nullptr, nullptr);
}

// ---- the workspace of a forward: the plan's tensors, then the decoder's scratch ----------------------------------------
static int forward_workspace_bytes(const char* who, esahrnet_handle h, int n, int height, int width, Decoder d, size_t* bytes,
                                   int refine = -1) {
    if (!h || !bytes) return fail("%s: null argument", who);
    if (plan_shape(*h, n, height, width)) return 1;
    *bytes = h->sp.bytes + kp_scratch(*h, n, height, width, d, refine).total();
    return 0;
}

int esahrnet_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    return forward_workspace_bytes("workspace_bytes", h, n, height, width, DEC_NONE, bytes);
}

int esahrnet_keypoints_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    return forward_workspace_bytes("keypoints_workspace_bytes", h, n, height, width, DEC_FINAL, bytes);
}

int esahrnet_keypoints_final2_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    return forward_workspace_bytes("keypoints_final2_forward_workspace_bytes", h, n, height, width, DEC_FINAL2, bytes);
}

int esahrnet_keypoints_gaussfit_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    return forward_workspace_bytes("keypoints_gaussfit_forward_workspace_bytes", h, n, height, width, DEC_GAUSSFIT, bytes);
}

int esahrnet_keypoints_candidates_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    return forward_workspace_bytes("keypoints_candidates_forward_workspace_bytes", h, n, height, width, DEC_CAND, bytes);
}

// ---- the forward straight to keypoints ----------------------------------------------------------------------------------
static int forward_request(const char* who, esahrnet_handle h, const void* x_dev, int n, int height, int width, const Request& r,
                           void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    if (!h || !r.kp) return fail("%s: null argument", who);
    return run_forward(h, x_dev, n, height, width, nullptr, nullptr, ws_dev, ws_bytes, stream, nullptr, &r);
}

int esahrnet_forward_keypoints(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* kp_dev, void* idx_dev,
                               void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    return forward_request("forward_keypoints", h, x_dev, n, height, width, make_request(DEC_FINAL, kp_dev, idx_dev), ws_dev,
                           ws_bytes, stream);
}

int esahrnet_forward_keypoints_final2(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* kp_dev,
                                      void* idx_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    return forward_request("forward_keypoints_final2", h, x_dev, n, height, width, make_request(DEC_FINAL2, kp_dev, idx_dev), ws_dev,
                           ws_bytes, stream);
}

int esahrnet_forward_keypoints_final2_hess(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* kp_dev,
                                           void* idx_dev, void* hess_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    return forward_request("forward_keypoints_final2_hess", h, x_dev, n, height, width,
                           make_request(DEC_FINAL2, kp_dev, idx_dev, hess_dev), ws_dev, ws_bytes, stream);
}

// what esahrnet_forward_keypoints_gaussfit and the loader in front of it refuse about the decoder's outputs
static int check_gaussfit_outputs(const char* who, const esahrnet_ctx& c, const Request& r) {
    if ((reinterpret_cast<uintptr_t>(r.kp) | reinterpret_cast<uintptr_t>(r.idx) | reinterpret_cast<uintptr_t>(r.status)) & 3)
        return fail("%s: kp_dev, idx_dev and status_dev must be 4-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(r.fit) | reinterpret_cast<uintptr_t>(r.hess)) & 7)
        return fail("%s: fit_dev and hess_dev must be 8-byte aligned", who);
    if (c.cfg.variant != 1 && !c.opt.final_mfma && c.cfg.cin > 8)
        return fail("%s: the VALU output layer's fit stages at most 8 input channels (this handle takes %d)", who, c.cfg.cin);
    return 0;
}

// esahrnet_forward_keypoints_gaussfit and, with_cov, esahrnet_forward_keypoints_gaussfit_cov
static int forward_gaussfit(const char* who, bool with_cov, esahrnet_handle h, const void* x_dev, int n, int height, int width,
                            const Request& r, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    if (!h || !x_dev || !r.kp || !r.status || !ws_dev) return fail("%s: null argument", who);
    if (check_gaussfit_outputs(who, *h, r) || (with_cov && esa::check_cov_args(who, r.cov, r.info, r.cov_floor))) return 1;
    return run_forward(h, x_dev, n, height, width, nullptr, nullptr, ws_dev, ws_bytes, stream, nullptr, &r);
}

int esahrnet_forward_keypoints_gaussfit(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* kp_dev,
                                        void* idx_dev, void* fit_dev, void* status_dev, void* hess_dev, void* ws_dev,
                                        size_t ws_bytes, esahrnet_stream stream) {
    return forward_gaussfit("forward_keypoints_gaussfit", false, h, x_dev, n, height, width,
                            make_request(DEC_GAUSSFIT, kp_dev, idx_dev, hess_dev, fit_dev, status_dev), ws_dev, ws_bytes, stream);
}

int esahrnet_forward_keypoints_gaussfit_cov(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* kp_dev,
                                            void* idx_dev, void* fit_dev, void* status_dev, void* hess_dev, void* cov_dev,
                                            void* info_dev, double cov_floor, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    return forward_gaussfit("forward_keypoints_gaussfit_cov", true, h, x_dev, n, height, width,
                            make_request(DEC_GAUSSFIT, kp_dev, idx_dev, hess_dev, fit_dev, status_dev, cov_dev, info_dev, cov_floor),
                            ws_dev, ws_bytes, stream);
}

// what esahrnet_forward_keypoints_candidates and the loader in front of it refuse about the decoder's arguments
static int check_candidates_request(const char* who, const Request& r) {
    if (r.M < 1 || r.M > ESAHRNET_MAX_CANDIDATES)
        return fail("%s: %d candidates per heat-map unsupported (1..%d)", who, r.M, ESAHRNET_MAX_CANDIDATES);
    if (r.r < 0) return fail("%s: negative nms_radius %d", who, r.r);
    if ((reinterpret_cast<uintptr_t>(r.cand) | reinterpret_cast<uintptr_t>(r.cidx)) & 3)
        return fail("%s: cand_dev and cidx_dev must be 4-byte aligned", who);
    return 0;
}

int esahrnet_forward_keypoints_candidates(esahrnet_handle h, const void* x_dev, int n, int height, int width, int candidates,
                                          int nms_radius, void* cand_dev, void* cidx_dev, void* ws_dev, size_t ws_bytes,
                                          esahrnet_stream stream) {
    const char* who = "forward_keypoints_candidates";
    const Request r = make_candidates_request(cand_dev, cidx_dev, candidates, nms_radius);
    if (!h || !r.cand) return fail("%s: null argument", who);
    if (check_candidates_request(who, r)) return 1;
    return run_forward(h, x_dev, n, height, width, nullptr, nullptr, ws_dev, ws_bytes, stream, nullptr, &r);
}

// ---- the candidates refined at their own pixels, in the forward (keypoints_at.hip behind the search) -------------------------
// What esahrnet_forward_keypoints_candidates_refined and the loader in front of it refuse about the decoder's arguments, in the
// order include/esahrnet.h gives; `decoder` as the caller passed it.  The texts are those of esahrnet_keypoints_candidates_refined.
static int check_refined_decoder(const char* who, int decoder) {
    if (decoder < 0 || decoder > 2) return fail("%s: decoder=%d unknown (0: get_final, 1: get_final2, 2: gaussfit)", who, decoder);
    return 0;
}
static int check_refined_request(const char* who, const Request& r, int decoder) {
    if (r.M < 1 || r.M > ESAHRNET_MAX_CANDIDATES)
        return fail("%s: %d candidates per heat-map unsupported (1..%d)", who, r.M, ESAHRNET_MAX_CANDIDATES);
    if (r.r < 0) return fail("%s: negative nms_radius %d", who, r.r);
    if (check_refined_decoder(who, decoder)) return 1;
    if (decoder == 0 && (r.hess || r.fit || r.cov || r.info))
        return fail("%s: decoder 0 (get_final) writes no hess_dev, fit_dev, cov_dev or info_dev: pass NULL", who);
    if (decoder == 1 && (r.fit || r.cov || r.info))
        return fail("%s: decoder 1 (get_final2) writes no fit_dev, cov_dev or info_dev: pass NULL", who);
    if (decoder == 2 && !r.status) return fail("%s: decoder 2 (gaussfit) needs status_dev", who);
    if (!(r.cov_floor >= 0.0) || !std::isfinite(r.cov_floor))
        return fail("%s: cov_floor must be a finite number >= 0 (got %g)", who, r.cov_floor);
    if ((reinterpret_cast<uintptr_t>(r.cand) | reinterpret_cast<uintptr_t>(r.cidx) | reinterpret_cast<uintptr_t>(r.status)) & 3)
        return fail("%s: cand_dev, cidx_dev and status_dev must be 4-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(r.hess) | reinterpret_cast<uintptr_t>(r.fit) | reinterpret_cast<uintptr_t>(r.cov) |
         reinterpret_cast<uintptr_t>(r.info)) & 7)
        return fail("%s: hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned", who);
    return 0;
}

int esahrnet_keypoints_candidates_refined_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, int decoder,
                                                                  size_t* bytes) {
    const char* who = "keypoints_candidates_refined_forward_workspace_bytes";
    if (!h || !bytes) return fail("%s: null argument", who);
    if (check_refined_decoder(who, decoder)) return 1;
    return forward_workspace_bytes(who, h, n, height, width, DEC_CAND, bytes, decoder);
}

int esahrnet_forward_keypoints_candidates_refined(esahrnet_handle h, const void* x_dev, int n, int height, int width, int candidates,
                                                  int nms_radius, int decoder, void* cand_dev, void* cidx_dev, void* hess_dev,
                                                  void* fit_dev, void* status_dev, void* cov_dev, void* info_dev, double cov_floor,
                                                  void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    const char* who = "forward_keypoints_candidates_refined";
    const Request r = make_request(DEC_CAND, cand_dev, cidx_dev, hess_dev, fit_dev, status_dev, cov_dev, info_dev, cov_floor,
                                   candidates, nms_radius, decoder);
    if (!h || !r.cand) return fail("%s: null argument", who);
    if (check_refined_request(who, r, decoder)) return 1;
    return run_forward(h, x_dev, n, height, width, nullptr, nullptr, ws_dev, ws_bytes, stream, nullptr, &r);
}

// ---- the loader on the device: detector boxes + frames -> crops -> keypoints (frontend.hip) ----------------------------
// what the loader entries take besides the handle and the decoder's outputs
struct FramesArgs {
    const void* frames;
    int nframes, frame_h, frame_w, pixel_format;
    const void* det_boxes;
    const void* frame_idx;
    int m, scale, rule;
    float mean, stdv;
    void *crop_boxes, *rates, *valid;
    void* ws;
    size_t ws_bytes;
    esahrnet_stream stream;
};

static size_t frontend_crop_bytes(int m, int scale) { return ((size_t)m * scale * scale * sizeof(float) + 255) & ~(size_t)255; }

// the loader's workspace: its crops, then the workspace of the forward with decoder `d` on them
static int frames_workspace_bytes(const char* who, esahrnet_handle h, int m, int scale, Decoder d, size_t* bytes, int refine = -1) {
    if (h->cfg.cin != 1)
        return fail("%s: the loader makes 1-channel crops (data_load_val.py / data_load4.py); this handle takes %d channels", who,
                    h->cfg.cin);
    if (m <= 0 || scale <= 0 || (long long)m * scale > esa::kFrontendMaxRows)
        return fail("%s: scale %d with %d boxes (both positive, boxes * scale at most %d)", who, scale, m, esa::kFrontendMaxRows);
    size_t fw = 0;
    if (forward_workspace_bytes(who, h, m, scale, scale, d, &fw, refine)) return 1;
    *bytes = frontend_crop_bytes(m, scale) + fw;
    return 0;
}

int esahrnet_frames_keypoints_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, size_t* bytes) {
    if (!h || !bytes) return fail("frames_keypoints_workspace_bytes: null argument");
    if (decoder != 0 && decoder != 1) return fail("frames_keypoints: decoder=%d unknown (0: get_final, 1: get_final2)", decoder);
    return frames_workspace_bytes("frames_keypoints", h, m, scale, decoder ? DEC_FINAL2 : DEC_FINAL, bytes);
}

int esahrnet_frames_keypoints_gaussfit_workspace_bytes(esahrnet_handle h, int m, int scale, size_t* bytes) {
    if (!h || !bytes) return fail("frames_keypoints_gaussfit_workspace_bytes: null argument");
    return frames_workspace_bytes("frames_keypoints_gaussfit", h, m, scale, DEC_GAUSSFIT, bytes);
}

int esahrnet_frames_keypoints_candidates_workspace_bytes(esahrnet_handle h, int m, int scale, size_t* bytes) {
    if (!h || !bytes) return fail("frames_keypoints_candidates_workspace_bytes: null argument");
    return frames_workspace_bytes("frames_keypoints_candidates", h, m, scale, DEC_CAND, bytes);
}

int esahrnet_frames_keypoints_candidates_refined_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, size_t* bytes) {
    if (!h || !bytes) return fail("frames_keypoints_candidates_refined_workspace_bytes: null argument");
    if (check_refined_decoder("frames_keypoints_candidates_refined", decoder)) return 1;
    return frames_workspace_bytes("frames_keypoints_candidates_refined", h, m, scale, DEC_CAND, bytes, decoder);
}

// what every loader entry refuses about the frames and the boxes
static int check_frames_args(const char* who, const FramesArgs& a) {
    if (esa::check_boxes_args(who, a.m, a.frame_h, a.frame_w, a.scale, a.rule) ||
        esa::check_crops_args(who, a.nframes, a.pixel_format, a.stdv))
        return 1;
    if (!a.frame_idx && a.m != a.nframes)
        return fail("%s: %d boxes on %d frames need a frame index (NULL is the identity: box i lies on frame i)", who, a.m, a.nframes);
    return 0;
}

// The loader entries after their argument checks (`who` names the caller in the messages): boxes -> crops at the head of the
// workspace -> forward + the decoder of `r` -> NaN rows for invalid crops.
static int frames_run(const char* who, esahrnet_handle h, const FramesArgs& a, const Request& r) {
    const hipStream_t st = static_cast<hipStream_t>(a.stream);
    const int* const frame_idx = static_cast<const int*>(a.frame_idx);
    int* const crop_boxes = static_cast<int*>(a.crop_boxes);
    int* const valid = static_cast<int*>(a.valid);
    int rc = esa::launch_boxes(static_cast<const int*>(a.det_boxes), frame_idx, a.nframes, a.m, a.frame_h, a.frame_w, a.scale, a.rule,
                               crop_boxes, static_cast<double*>(a.rates), valid, st);
    if (!rc)
        rc = esa::launch_crops_ex(static_cast<const unsigned char*>(a.frames), a.nframes, a.frame_h, a.frame_w, a.pixel_format,
                                  frame_idx, crop_boxes, valid, static_cast<float*>(a.ws), a.m, a.scale, a.mean, a.stdv, st);
    if (rc) return fail("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    const size_t head = frontend_crop_bytes(a.m, a.scale);
    if (run_forward(h, a.ws, a.m, a.scale, a.scale, nullptr, nullptr, static_cast<char*>(a.ws) + head, a.ws_bytes - head, a.stream,
                    nullptr, &r))
        return 1;
    if (r.decoder == DEC_CAND && r.refine >= 0)     // every output of the refined candidates has K * M rows per crop
        rc = esa::launch_mark_invalid_refined(valid, a.m, h->cfg.num_keypoints * r.M, r.cand, r.cidx, r.status, r.hess, r.fit, r.cov,
                                              r.info, st);
    else if (r.decoder == DEC_CAND)                 // a crop's K * M candidate rows: the kp / idx rows of K * M keypoints
        rc = esa::launch_mark_invalid(valid, a.m, h->cfg.num_keypoints * r.M, r.cand, r.cidx, st);
    else if (r.decoder == DEC_GAUSSFIT)
        rc = esa::launch_mark_invalid_gaussfit_cov(valid, a.m, h->cfg.num_keypoints, r.kp, r.idx, r.fit, r.status, r.hess, r.cov,
                                                   r.info, st);
    else rc = esa::launch_mark_invalid(valid, a.m, h->cfg.num_keypoints, r.kp, r.idx, st);
    if (rc) return fail("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    return 0;
}

// The four esahrnet_frames_keypoints* entries: everything that can be refused is refused here, before the first launch.
// abi_decoder: the `decoder` argument of esahrnet_frames_keypoints as given (refused by its workspace query when unknown);
// unused by the Gaussian-fit entries.  Each entry keeps the order of its refusals: the _cov form checks its three additions
// before the handle's commit, and so does the candidates' form with M, r and the alignment of its outputs.
static int frames_keypoints(const char* who, bool with_cov, esahrnet_handle h, const FramesArgs& a, int abi_decoder,
                            const Request& r) {
    const bool gaussfit = r.decoder == DEC_GAUSSFIT;
    if (!h || !a.frames || !a.det_boxes || !r.kp || (gaussfit && !r.status) || !a.crop_boxes || !a.rates || !a.valid || !a.ws)
        return fail("%s: null argument", who);
    if (check_frames_args(who, a)) return 1;
    if (with_cov && esa::check_cov_args(who, r.cov, r.info, r.cov_floor)) return 1;
    if (r.decoder == DEC_CAND && check_candidates_request(who, r)) return 1;
    if (!h->committed) return fail("%s: esahrnet_commit has not been called", who);
    if (gaussfit && check_gaussfit_outputs(who, *h, r)) return 1;
    size_t need = 0;
    if (r.decoder == DEC_CAND ? esahrnet_frames_keypoints_candidates_workspace_bytes(h, a.m, a.scale, &need)
        : gaussfit ? esahrnet_frames_keypoints_gaussfit_workspace_bytes(h, a.m, a.scale, &need)
                 : esahrnet_frames_keypoints_workspace_bytes(h, a.m, a.scale, abi_decoder, &need))
        return 1;
    if (a.ws_bytes < need) return fail("%s: workspace too small (%zu < %zu)", who, a.ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(a.ws) & 255) return fail("%s: workspace must be 256-byte aligned", who);
    return frames_run(who, h, a, r);
}

int esahrnet_frames_keypoints(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w, int pixel_format,
                              const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale, int rule, float mean,
                              float stdv, int decoder, void* kp_dev, void* idx_dev, void* crop_boxes_dev, void* rates_dev,
                              void* valid_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints", false, h, a, decoder,
                            make_request(decoder == 1 ? DEC_FINAL2 : DEC_FINAL, kp_dev, idx_dev));
}

int esahrnet_frames_keypoints_gaussfit(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                       int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                       int rule, float mean, float stdv, void* kp_dev, void* idx_dev, void* fit_dev, void* status_dev,
                                       void* hess_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* ws_dev,
                                       size_t ws_bytes, esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints_gaussfit", false, h, a, 0,
                            make_request(DEC_GAUSSFIT, kp_dev, idx_dev, hess_dev, fit_dev, status_dev));
}

int esahrnet_frames_keypoints_gaussfit_cov(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                           int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                           int rule, float mean, float stdv, void* kp_dev, void* idx_dev, void* fit_dev,
                                           void* status_dev, void* hess_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev,
                                           void* cov_dev, void* info_dev, double cov_floor, void* ws_dev, size_t ws_bytes,
                                           esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints_gaussfit_cov", true, h, a, 0,
                            make_request(DEC_GAUSSFIT, kp_dev, idx_dev, hess_dev, fit_dev, status_dev, cov_dev, info_dev, cov_floor));
}

int esahrnet_frames_keypoints_candidates(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                         int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                         int rule, float mean, float stdv, int candidates, int nms_radius, void* cand_dev,
                                         void* cidx_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* ws_dev,
                                         size_t ws_bytes, esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints_candidates", false, h, a, 0,
                            make_candidates_request(cand_dev, cidx_dev, candidates, nms_radius));
}

// esahrnet_frames_keypoints_candidates with the refined candidates' forward in the place of the plain one.  The refusals sit
// where that entry has them: the frames' and boxes' arguments, then the decoder's own, then the handle's commit
int esahrnet_frames_keypoints_candidates_refined(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                                 int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m,
                                                 int scale, int rule, float mean, float stdv, int candidates, int nms_radius,
                                                 int decoder, void* cand_dev, void* cidx_dev, void* hess_dev, void* fit_dev,
                                                 void* status_dev, void* cov_dev, void* info_dev, double cov_floor,
                                                 void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* ws_dev, size_t ws_bytes,
                                                 esahrnet_stream stream) {
    const char* who = "frames_keypoints_candidates_refined";
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    const Request r = make_request(DEC_CAND, cand_dev, cidx_dev, hess_dev, fit_dev, status_dev, cov_dev, info_dev, cov_floor,
                                   candidates, nms_radius, decoder);
    if (!h || !a.frames || !a.det_boxes || !r.cand || !a.crop_boxes || !a.rates || !a.valid || !a.ws)
        return fail("%s: null argument", who);
    if (check_frames_args(who, a)) return 1;
    if (check_refined_request(who, r, decoder)) return 1;
    if (!h->committed) return fail("%s: esahrnet_commit has not been called", who);
    size_t need = 0;
    if (esahrnet_frames_keypoints_candidates_refined_workspace_bytes(h, a.m, a.scale, decoder, &need)) return 1;
    if (a.ws_bytes < need) return fail("%s: workspace too small (%zu < %zu)", who, a.ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(a.ws) & 255) return fail("%s: workspace must be 256-byte aligned", who);
    return frames_run(who, h, a, r);
}

// ---- keypoints -> correspondences for the pose solver (correspond.hip) --------------------------------------------------
static size_t frontend_hess_bytes(int m, int k) { return ((size_t)m * k * 3 * sizeof(double) + 255) & ~(size_t)255; }

int esahrnet_frames_correspondences_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, int mode, size_t* bytes) {
    if (!h || !bytes) return fail("frames_correspondences_workspace_bytes: null argument");
    if (esa::check_corr_args("frames_correspondences", m, h->cfg.num_keypoints, mode)) return 1;
    if (mode == 1 && decoder == 0)
        return fail("frames_correspondences: mode 1 (Hessian weights) needs decoder 1: get_final (decoder 0) computes no Hessian");
    size_t fk = 0;
    if (esahrnet_frames_keypoints_workspace_bytes(h, m, scale, decoder, &fk)) return 1;
    *bytes = ((fk + 255) & ~(size_t)255) + (mode == 1 ? frontend_hess_bytes(m, h->cfg.num_keypoints) : 0);
    return 0;
}

int esahrnet_frames_correspondences(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                    int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                    int rule, float mean, float stdv, int decoder, double thresh, int min_k, int mode, void* kp_dev,
                                    void* idx_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* count_dev,
                                    void* order_dev, void* pts_dev, void* w_dev, void* ws_dev, size_t ws_bytes,
                                    esahrnet_stream stream) {
    const char* who = "frames_correspondences";
    if (!h || !frames_dev || !det_boxes_dev || !kp_dev || !crop_boxes_dev || !rates_dev || !valid_dev || !count_dev || !order_dev ||
        !pts_dev || !w_dev || !ws_dev)
        return fail("%s: null argument", who);
    // everything that can be refused is refused here, before the first launch
    FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                 crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    if (check_frames_args(who, a)) return 1;
    if (!h->committed) return fail("%s: esahrnet_commit has not been called", who);
    size_t need = 0, fk = 0;
    if (esahrnet_frames_correspondences_workspace_bytes(h, m, scale, decoder, mode, &need) ||
        esahrnet_frames_keypoints_workspace_bytes(h, m, scale, decoder, &fk))
        return 1;
    if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(ws_dev) & 255) return fail("%s: workspace must be 256-byte aligned", who);
    a.ws_bytes = (fk + 255) & ~(size_t)255;         // the loader's share; the Hessians of mode 1 lie behind it
    void* hess = mode == 1 ? static_cast<char*>(ws_dev) + a.ws_bytes : nullptr;
    if (frames_run(who, h, a, make_request(decoder == 1 ? DEC_FINAL2 : DEC_FINAL, kp_dev, idx_dev, hess))) return 1;
    const int rc = esa::launch_correspond(static_cast<const float*>(kp_dev), static_cast<const double*>(hess),
                                          static_cast<const int*>(crop_boxes_dev), static_cast<const double*>(rates_dev),
                                          static_cast<const int*>(valid_dev), m, h->cfg.num_keypoints, thresh, min_k, mode,
                                          static_cast<int*>(count_dev), static_cast<int*>(order_dev), static_cast<double*>(pts_dev),
                                          static_cast<double*>(w_dev), static_cast<hipStream_t>(stream));
    if (rc) return fail("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    return 0;
}

int esahrnet_flops_per_crop(esahrnet_handle h, int height, int width, double* flops) {
    if (!h || !flops) return fail("flops_per_crop: null argument");
    std::vector<int> lh, lw;
    level_dims(*h, height, width, lh, lw);
    double f = 0;
    for (const ConvSpec& s : h->specs)        // the reference's direct form: derived specs restate work already counted
        if (s.parent < 0) f += 2.0 * lh[s.level] * lw[s.level] * s.cout * s.cin * s.k * s.k;
    *flops = f;
    return 0;
}

int esahrnet_launch_count(esahrnet_handle h) { return h ? (int)h->ops.size() : -1; }

int esahrnet_tap_count(esahrnet_handle h) {
    if (!h) return -1;
    int n = 0;
    for (const Tensor& t : h->tensors) n += !t.tap.empty();
    return n;
}

int esahrnet_tap_name(esahrnet_handle h, int index, char* out, size_t cap) {
    if (!h || !out) return fail("tap_name: null argument");
    int n = 0;
    for (const Tensor& t : h->tensors)
        if (!t.tap.empty() && n++ == index) { snprintf(out, cap, "%s", t.tap.c_str()); return 0; }
    return fail("tap_name: index %d out of range", index);
}

static const Tensor* find_tap(esahrnet_handle h, const char* name) {
    for (const Tensor& t : h->tensors)
        if (t.tap == name) return &t;
    return nullptr;
}

int esahrnet_tap_shape(esahrnet_handle h, const char* name, int height, int width, int* c, int* th, int* tw) {
    if (!h || !name || !c || !th || !tw) return fail("tap_shape: null argument");
    const Tensor* t = find_tap(h, name);
    if (!t) return fail("tap_shape: no tensor named '%s'", name);
    std::vector<int> lh, lw;
    level_dims(*h, height, width, lh, lw);
    *c = t->C; *th = lh[t->level]; *tw = lw[t->level];
    return 0;
}

int esahrnet_tap_read(esahrnet_handle h, const char* name, int n, int height, int width,
                      const void* ws_dev, void* out_dev, esahrnet_stream stream) {
    if (!h || !name || !ws_dev || !out_dev) return fail("tap_read: null argument");
    if (!h->keep) return fail("tap_read: call esahrnet_set_debug_keep(h, 1) before the forward (buffers are recycled otherwise)");
    const Tensor* t = find_tap(h, name);
    if (!t) return fail("tap_read: no tensor named '%s'", name);
    if (plan_shape(*h, n, height, width)) return 1;
    if (t->alt != 0 && t->alt != (h->sp.head2 ? 2 : 1))
        return fail("tap_read: '%s' belongs to the head alternative that does not run at this shape", name);
    // a tensor stored as T * 2^-e (fp16 scale exponents) comes back as T: the conversion takes the factor
    const int e = h->gexp(h->tgroup[t - h->tensors.data()]);
    const int rc = e ? esa::launch_hf_to_nchw_scaled(static_cast<const char*>(ws_dev) + t->off, n, t->C, h->sp.lh[t->level],
                                                     h->sp.lw[t->level], t->Cp, static_cast<float*>(out_dev), ldexpf(1.f, e),
                                                     static_cast<hipStream_t>(stream))
                     : esa::launch_fmt_to_nchw(t->f32 ? esa::FMT_F32 : h->opt.fmt,
        static_cast<const char*>(ws_dev) + t->off, n, t->C, h->sp.lh[t->level], h->sp.lw[t->level], t->Cp,
        static_cast<float*>(out_dev), static_cast<hipStream_t>(stream));
    if (rc) return fail("tap_read: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

// ---- activation range report (stats.hip) -------------------------------------------------------------------------------
// Rows: the plan's tensors in plan order, then "heatmaps".  The storage format of a tensor, as esahrnet_tap_read takes it:
static int stats_fmt(const esahrnet_ctx& c, const Tensor& t) { return t.f32 ? (int)esa::FMT_F32 : c.opt.fmt; }

// Does the scan read tensor `t` at this shape?  Not the flat scratch, the T layout or the head alternative that does not run,
// and no tensor without the padded-channel layout of its format (CBAM's two-plane maps): stats_parts refuses those.
static bool stats_scanned(const esahrnet_ctx& c, const ShapePlan& sp, const Tensor& t) {
    if (t.flat || t.tlayout || t.def < 0) return false;
    if (t.alt != 0 && t.alt != (sp.head2 ? 2 : 1)) return false;
    const long long hw = (long long)sp.lh[t.level] * sp.lw[t.level];
    return hw <= 0x7fffffffLL && esa::stats_parts(stats_fmt(c, t), t.C, t.Cp, (int)hw) > 0;
}

// partial records of one image over all scanned rows, heat-maps included; -1: the heat-maps are beyond the scan
static long long stats_partials_per_image(const esahrnet_ctx& c, const ShapePlan& sp) {
    const int hp = esa::stats_parts(esa::STATS_NCHW, c.cfg.num_keypoints, 0, sp.h * sp.w);
    if (hp <= 0) return -1;
    long long parts = hp;
    for (const Tensor& t : c.tensors)
        if (stats_scanned(c, sp, t)) parts += esa::stats_parts(stats_fmt(c, t), t.C, t.Cp, sp.lh[t.level] * sp.lw[t.level]);
    return parts;
}

int esahrnet_stats_rows(esahrnet_handle h, int* rows) {
    if (!h || !rows) return fail("stats_rows: null argument");
    *rows = (int)h->tensors.size() + 1;
    return 0;
}

int esahrnet_stats_row_get(esahrnet_handle h, int row, int n, int height, int width, esahrnet_stats_row_desc* out) {
    if (!h || !out) return fail("stats_row_get: null argument");
    const int nt = (int)h->tensors.size();
    if (row < 0 || row > nt) return fail("stats_row_get: row %d out of range (0..%d)", row, nt);
    if (check_shape(n, height, width)) return 1;
    memset(out, 0, sizeof *out);
    if (row == nt) {
        snprintf(out->name, sizeof out->name, "heatmaps");
        out->def_op = (int)h->ops.size() - 1;
        out->c = h->cfg.num_keypoints; out->h = height; out->w = width;
        out->fmt = esa::STATS_NCHW;
        out->scanned = 1;
        return 0;
    }
    const Tensor& t = h->tensors[row];
    const ShapePlan sp = shape_decisions(*h, n, height, width);
    out->def_op = t.def;
    out->fmt = t.flat ? (int)esa::FMT_F32 : stats_fmt(*h, t);
    if (!t.flat) { out->c = t.C; out->h = sp.lh[t.level]; out->w = sp.lw[t.level]; }
    out->scanned = stats_scanned(*h, sp, t) ? 1 : 0;
    if (!t.tap.empty()) snprintf(out->name, sizeof out->name, "%s", t.tap.c_str());
    else if (t.def >= 0) {
        esahrnet_op_desc d;
        memset(&d, 0, sizeof d);
        if (run_op(*h, h->ops[t.def], sp, Buffers{}, nullptr, &d)) return 1;
        snprintf(out->name, sizeof out->name, "%s", d.label);
    } else snprintf(out->name, sizeof out->name, "(tensor %d)", row);
    return 0;
}

static size_t stats_pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// the keep-mode plan of the shape, then the partials behind it; the handle's keep state is put back by the caller
static int stats_plan(const char* who, esahrnet_ctx& c, int n, int height, int width, size_t* bytes) {
    if (plan_shape(c, n, height, width)) return 1;
    const long long parts = stats_partials_per_image(c, c.sp);
    if (parts < 0) return fail("%s: crop %dx%d is beyond the scan of the heat-maps", who, height, width);
    *bytes = stats_pad256(stats_pad256(c.sp.bytes) + (size_t)parts * n * sizeof(esahrnet_stats_record));
    return 0;
}

int esahrnet_forward_stats_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    if (!h || !bytes) return fail("forward_stats_workspace_bytes: null argument");
    const bool keep = h->keep;
    h->keep = true;
    const int rc = stats_plan("forward_stats_workspace_bytes", *h, n, height, width, bytes);
    h->keep = keep;
    return rc;
}

// the partials of the fused head's range form behind the scan's (esahrnet_forward_stats_h0); 0 where that head does not run
static size_t stats_h0_bytes(const esahrnet_ctx& c, const ShapePlan& sp) {
    if (c.head2_op < 0 || c.ops[c.head2_op].kind != OP_HEADBF || c.x6() || !sp.head2) return 0;
    const Tensor& t0 = c.tensors[c.ops[c.head2_op].in];
    return stats_pad256((size_t)esa::head_bf_range_tiles(sp.lh[t0.level], sp.lw[t0.level]) * sp.n * 8);
}

// esahrnet_forward_stats (h0_dev == nullptr, with_h0 false) and esahrnet_forward_stats_h0
static int forward_stats(const char* who, bool with_h0, esahrnet_handle h, const void* x_dev, int n, int height, int width,
                         void* heat_dev, void* ws_dev, size_t ws_bytes, void* stats_dev, void* h0_dev, esahrnet_stream stream_) {
    if (!h || !x_dev || !heat_dev || !ws_dev || !stats_dev || (with_h0 && !h0_dev)) return fail("%s: null argument", who);
    if (!h->committed) return fail("%s: esahrnet_commit has not been called", who);
    if (with_h0 && h->gnames.empty()) return fail("%s: variant 0 with precision 1 or 3 only (the head that rounds h0 in registers)", who);
    if (with_h0 && h->opt.bf_head_valu && !h->hf()) return fail("%s: the range form is the matrix-core head's: unset ESAHRNET_BF_HEAD_VALU", who);
    const bool keep = h->keep;
    h->keep = true;
    auto body = [&]() -> int {
        size_t need = 0;
        if (stats_plan(who, *h, n, height, width, &need)) return 1;
        const size_t h0_off = need, h0_bytes = with_h0 ? stats_h0_bytes(*h, h->sp) : 0;
        need += h0_bytes;
        if (ws_bytes < need) return fail("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
        if (reinterpret_cast<uintptr_t>(ws_dev) & 255) return fail("%s: workspace must be 256-byte aligned", who);
        if (reinterpret_cast<uintptr_t>(stats_dev) & 7) return fail("%s: stats_dev must be 8-byte aligned", who);
        if (with_h0 && (reinterpret_cast<uintptr_t>(h0_dev) & 7)) return fail("%s: h0_dev must be 8-byte aligned", who);
        hipStream_t stream = static_cast<hipStream_t>(stream_);
        const size_t rows = h->tensors.size() + 1;
        HIP_OK(hipMemsetAsync(stats_dev, 0, rows * n * sizeof(esahrnet_stats_record), stream));   // the rows not scanned
        if (run_forward(h, x_dev, n, height, width, heat_dev, nullptr, ws_dev, ws_bytes, stream_, nullptr, nullptr,
                        h0_bytes ? static_cast<char*>(ws_dev) + h0_off : nullptr, h0_bytes ? h0_dev : nullptr)) return 1;
        const ShapePlan& sp = h->sp;
        char* const ws = static_cast<char*>(ws_dev);
        std::vector<esa::StatsJob> jobs;
        for (size_t ti = 0; ti < h->tensors.size(); ++ti) {
            const Tensor& t = h->tensors[ti];
            if (stats_scanned(*h, sp, t))
                jobs.push_back({ws + t.off, stats_fmt(*h, t), t.C, t.Cp, sp.lh[t.level] * sp.lw[t.level], (int)ti});
        }
        jobs.push_back({heat_dev, esa::STATS_NCHW, h->cfg.num_keypoints, 0, height * width, (int)rows - 1});
        const int rc = esa::launch_stats(jobs.data(), (int)jobs.size(), n, ws + stats_pad256(sp.bytes), stats_dev, stream);
        if (rc) return fail("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
        if (with_h0 && !h0_bytes) {     // the materialised head ran: h0 is the stored row "head0"
            int row = -1;
            for (size_t ti = 0; ti < h->tensors.size(); ++ti)
                if (h->tensors[ti].tap == "head0" && stats_scanned(*h, sp, h->tensors[ti])) row = (int)ti;
            if (row < 0) return fail("%s: no head0 tensor at this shape", who);
            HIP_OK(hipMemcpyAsync(h0_dev, static_cast<const esahrnet_stats_record*>(stats_dev) + (size_t)row * n,
                                  (size_t)n * sizeof(esahrnet_stats_record), hipMemcpyDeviceToDevice, stream));
        }
        return 0;
    };
    const int rc = body();
    h->keep = keep;
    return rc;
}

int esahrnet_forward_stats(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* ws_dev,
                           size_t ws_bytes, void* stats_dev, esahrnet_stream stream) {
    return forward_stats("forward_stats", false, h, x_dev, n, height, width, heat_dev, ws_dev, ws_bytes, stats_dev, nullptr, stream);
}

int esahrnet_forward_stats_h0_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    if (!h || !bytes) return fail("forward_stats_h0_workspace_bytes: null argument");
    const bool keep = h->keep;
    h->keep = true;
    int rc = stats_plan("forward_stats_h0_workspace_bytes", *h, n, height, width, bytes);
    if (!rc) *bytes += stats_h0_bytes(*h, h->sp);
    h->keep = keep;
    return rc;
}

int esahrnet_forward_stats_h0(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* ws_dev,
                              size_t ws_bytes, void* stats_dev, void* h0_dev, esahrnet_stream stream) {
    return forward_stats("forward_stats_h0", true, h, x_dev, n, height, width, heat_dev, ws_dev, ws_bytes, stats_dev, h0_dev, stream);
}

static int stats_row_name(esahrnet_handle h, int row, char* out, size_t cap) {
    esahrnet_stats_row_desc d;
    if (esahrnet_stats_row_get(h, row, 1, 64, 64, &d)) return 1;
    snprintf(out, cap, "%s", d.name);
    return 0;
}

static int tensor_stats_parts(const char* who, int fmt, int n, int c, int cp, int h, int w, int* parts) {
    if (n < 1) return fail("%s: batch must be positive (got %d)", who, n);
    const long long hw = (long long)h * w;
    *parts = h > 0 && w > 0 && hw <= 0x7fffffffLL && fmt >= esa::STATS_NCHW && fmt <= esa::FMT_HF
                 ? esa::stats_parts(fmt, c, cp, (int)hw) : 0;
    if (*parts <= 0)
        return fail("%s: no scan for format %d, %d channels (%d padded), %dx%d (formats -1..3; SB: padded channels a multiple "
                    "of 8, BF / HF of 8, F32 of 4; an image below 2 GiB)", who, fmt, c, cp, h, w);
    return 0;
}

int esahrnet_tensor_stats_workspace_bytes(int fmt, int n, int c, int cp, int h, int w, size_t* bytes) {
    if (!bytes) return fail("tensor_stats_workspace_bytes: null argument");
    int parts = 0;
    if (tensor_stats_parts("tensor_stats_workspace_bytes", fmt, n, c, cp, h, w, &parts)) return 1;
    *bytes = (size_t)parts * n * sizeof(esahrnet_stats_record);
    return 0;
}

int esahrnet_tensor_stats(const void* t_dev, int fmt, int n, int c, int cp, int h, int w, void* ws_dev, size_t ws_bytes,
                          void* stats_dev, esahrnet_stream stream) {
    if (!t_dev || !ws_dev || !stats_dev) return fail("tensor_stats: null argument");
    int parts = 0;
    if (tensor_stats_parts("tensor_stats", fmt, n, c, cp, h, w, &parts)) return 1;
    const size_t need = (size_t)parts * n * sizeof(esahrnet_stats_record);
    if (ws_bytes < need) return fail("tensor_stats: workspace too small (%zu < %zu)", ws_bytes, need);
    if (fmt != esa::STATS_NCHW && (reinterpret_cast<uintptr_t>(t_dev) & 15)) return fail("tensor_stats: t_dev must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(ws_dev) & 7) return fail("tensor_stats: workspace must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(stats_dev) & 7) return fail("tensor_stats: stats_dev must be 8-byte aligned");
    const esa::StatsJob job{t_dev, fmt, c, cp, h * w, 0};
    const int rc = esa::launch_stats(&job, 1, n, ws_dev, stats_dev, static_cast<hipStream_t>(stream));
    if (rc) return fail("tensor_stats: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

// ---- precision report (diff.hip) -----------------------------------------------------------------------------------------
// Rows are the range report's.  Two rows of two handles hold the same tensor if they carry the same key (Tensor::key, given by
// the builder from what the tensor is: no label is parsed), and the key names one row only in either handle.
static std::string diff_key(const esahrnet_ctx& c, int row) {
    return row == (int)c.tensors.size() ? std::string("heatmaps") : c.tensors[row].key;
}

static int diff_find(const esahrnet_ctx& c, const std::string& key) {       // the one row with this key; -1: none or several
    if (key.empty()) return -1;
    int found = -1;
    for (int r = 0; r <= (int)c.tensors.size(); ++r)
        if (diff_key(c, r) == key) {
            if (found >= 0) return -1;
            found = r;
        }
    return found;
}

// one row of h against href under the two shape plans (shape_decisions, or the handles' own after plan_shape)
static void diff_row(const esahrnet_ctx& a, const ShapePlan& spa, const esahrnet_ctx& b, const ShapePlan& spb, int row,
                     int height, int width, esahrnet_diff_row_desc* out) {
    memset(out, 0, sizeof *out);
    const int nta = (int)a.tensors.size(), ntb = (int)b.tensors.size();
    const std::string key = diff_key(a, row);
    snprintf(out->key, sizeof out->key, "%s", key.c_str());
    out->ref_row = diff_find(a, key) == row ? diff_find(b, key) : -1;
    const int rr = out->ref_row;
    if (row == nta) {
        out->c = a.cfg.num_keypoints; out->h = height; out->w = width; out->fmt = esa::STATS_NCHW;
        if (rr < 0) return;
        out->ref_fmt = esa::STATS_NCHW;
        out->compared = rr == ntb && b.cfg.num_keypoints == out->c &&
                        esa::diff_parts(esa::STATS_NCHW, 0, esa::STATS_NCHW, 0, out->c, height * width) > 0;
        return;
    }
    const Tensor& ta = a.tensors[row];
    out->fmt = ta.flat ? (int)esa::FMT_F32 : stats_fmt(a, ta);
    if (!ta.flat) { out->c = ta.C; out->h = spa.lh[ta.level]; out->w = spa.lw[ta.level]; }
    out->exponent = a.gexp(a.tgroup.empty() ? -1 : a.tgroup[row]);
    if (rr < 0 || rr == ntb) { if (rr == ntb) out->ref_row = -1; return; }
    const Tensor& tb = b.tensors[rr];
    out->ref_fmt = tb.flat ? (int)esa::FMT_F32 : stats_fmt(b, tb);
    if (ta.flat || tb.flat || tb.C != out->c || spb.lh[tb.level] != out->h || spb.lw[tb.level] != out->w) return;
    out->compared = stats_scanned(a, spa, ta) && stats_scanned(b, spb, tb) &&
                    esa::diff_parts(out->fmt, ta.Cp, out->ref_fmt, tb.Cp, ta.C, out->h * out->w) > 0;
}

int esahrnet_diff_row_get(esahrnet_handle h, esahrnet_handle href, int row, int n, int height, int width,
                          esahrnet_diff_row_desc* out) {
    if (!h || !href || !out) return fail("diff_row_get: null argument");
    const int nt = (int)h->tensors.size();
    if (row < 0 || row > nt) return fail("diff_row_get: row %d out of range (0..%d)", row, nt);
    if (check_shape(n, height, width)) return 1;
    const ShapePlan spa = shape_decisions(*h, n, height, width);
    if (h == href) diff_row(*h, spa, *h, spa, row, height, width, out);
    else diff_row(*h, spa, *href, shape_decisions(*href, n, height, width), row, height, width, out);
    return 0;
}

// name of the first configuration field in which the handles differ, `precision` aside; nullptr: none
static const char* diff_cfg_field(const esahrnet_cfg& a, const esahrnet_cfg& b, int* va, int* vb) {
    static thread_local char name[32];
    auto differ = [&](int x, int y, const char* fmt, int i, int j) {
        if (x == y) return false;
        snprintf(name, sizeof name, fmt, i, j);
        *va = x; *vb = y;
        return true;
    };
    if (differ(a.variant, b.variant, "variant", 0, 0) || differ(a.cin, b.cin, "cin", 0, 0) ||
        differ(a.num_keypoints, b.num_keypoints, "num_keypoints", 0, 0) || differ(a.stem_width, b.stem_width, "stem_width", 0, 0))
        return name;
    for (int i = 0; i < ESAHRNET_MAX_BRANCHES; ++i)
        if (differ(a.widths[i], b.widths[i], "widths[%d]", i, 0)) return name;
    for (int s = 0; s < 4; ++s)
        for (int i = 0; i < ESAHRNET_MAX_BRANCHES; ++i)
            if (differ(a.blocks[s][i], b.blocks[s][i], "blocks[%d][%d]", s, i)) return name;
    for (int s = 0; s < 4; ++s)
        if (differ(a.modules[s], b.modules[s], "modules[%d]", s, 0)) return name;
    if (differ(a.final_conv_kernel, b.final_conv_kernel, "final_conv_kernel", 0, 0)) return name;
    return nullptr;
}

struct DiffPlan {
    size_t off_b = 0, off_parts = 0, bytes = 0;       // href's forward and the partials inside the workspace (h's forward at 0)
    std::vector<esahrnet_diff_row_desc> rows;
};

// both keep-mode plans of the shape (the caller has set keep on both handles and puts it back), the rows, the workspace
static int diff_plan(const char* who, esahrnet_ctx& a, esahrnet_ctx& b, int n, int height, int width, DiffPlan* dp) {
    int va = 0, vb = 0;
    if (const char* f = diff_cfg_field(a.cfg, b.cfg, &va, &vb))
        return fail("%s: the handles differ in %s (%d against %d): they may differ in precision only", who, f, va, vb);
    if (plan_shape(a, n, height, width)) return 1;
    if (&a != &b && plan_shape(b, n, height, width)) return 1;
    const int rows = (int)a.tensors.size() + 1;
    dp->rows.resize(rows);
    long long parts = 0;
    for (int r = 0; r < rows; ++r) {
        esahrnet_diff_row_desc& d = dp->rows[r];
        diff_row(a, a.sp, b, b.sp, r, height, width, &d);
        if (!d.compared) continue;
        parts += r == rows - 1 ? esa::diff_parts(esa::STATS_NCHW, 0, esa::STATS_NCHW, 0, d.c, height * width)
                               : esa::diff_parts(d.fmt, a.tensors[r].Cp, d.ref_fmt, b.tensors[d.ref_row].Cp, d.c, d.h * d.w);
    }
    if (!dp->rows[rows - 1].compared) return fail("%s: crop %dx%d is beyond the scan of the heat-maps", who, height, width);
    dp->off_b = stats_pad256(a.sp.bytes);
    dp->off_parts = dp->off_b + stats_pad256(b.sp.bytes);
    dp->bytes = stats_pad256(dp->off_parts + (size_t)parts * n * sizeof(esahrnet_diff_record));
    return 0;
}

int esahrnet_forward_diff_workspace_bytes(esahrnet_handle h, esahrnet_handle href, int n, int height, int width, size_t* bytes) {
    if (!h || !href || !bytes) return fail("forward_diff_workspace_bytes: null argument");
    const bool keep = h->keep, keep_ref = href->keep;
    h->keep = href->keep = true;
    DiffPlan dp;
    const int rc = diff_plan("forward_diff_workspace_bytes", *h, *href, n, height, width, &dp);
    h->keep = keep; href->keep = keep_ref;
    if (!rc) *bytes = dp.bytes;
    return rc;
}

int esahrnet_forward_diff(esahrnet_handle h, esahrnet_handle href, const void* x_dev, int n, int height, int width,
                          void* heat_dev, void* heat_ref_dev, void* ws_dev, size_t ws_bytes, void* diff_dev, esahrnet_stream stream_) {
    const char* who = "forward_diff";
    if (!h || !href || !x_dev || !heat_dev || !heat_ref_dev || !ws_dev || !diff_dev) return fail("%s: null argument", who);
    if (!h->committed || !href->committed)
        return fail("%s: esahrnet_commit has not been called on the %s handle", who, !h->committed ? "tested" : "reference");
    if (h->device != href->device) return fail("%s: the handles live on different devices (%d and %d)", who, h->device, href->device);
    const bool keep = h->keep, keep_ref = href->keep;
    h->keep = href->keep = true;
    auto body = [&]() -> int {
        DiffPlan dp;
        if (diff_plan(who, *h, *href, n, height, width, &dp)) return 1;
        if (ws_bytes < dp.bytes) return fail("%s: workspace too small (%zu < %zu)", who, ws_bytes, dp.bytes);
        if (reinterpret_cast<uintptr_t>(ws_dev) & 255) return fail("%s: workspace must be 256-byte aligned", who);
        if (reinterpret_cast<uintptr_t>(diff_dev) & 7) return fail("%s: diff_dev must be 8-byte aligned", who);
        hipStream_t stream = static_cast<hipStream_t>(stream_);
        const int rows = (int)dp.rows.size();
        char* const ws = static_cast<char*>(ws_dev);
        char* const ws_b = h == href ? ws : ws + dp.off_b;
        HIP_OK(hipMemsetAsync(diff_dev, 0, (size_t)rows * n * sizeof(esahrnet_diff_record), stream));     // the rows not compared
        if (run_forward(h, x_dev, n, height, width, heat_dev, nullptr, ws, dp.off_b, stream_, nullptr, nullptr)) return 1;
        if (h != href) {
            if (run_forward(href, x_dev, n, height, width, heat_ref_dev, nullptr, ws_b, dp.off_parts - dp.off_b, stream_, nullptr, nullptr))
                return 1;
        } else if (heat_ref_dev != heat_dev) {
            HIP_OK(hipMemcpyAsync(heat_ref_dev, heat_dev, (size_t)n * h->cfg.num_keypoints * height * width * sizeof(float),
                                  hipMemcpyDeviceToDevice, stream));
        }
        std::vector<esa::DiffJob> jobs;
        for (int r = 0; r + 1 < rows; ++r) {
            const esahrnet_diff_row_desc& d = dp.rows[r];
            if (!d.compared) continue;
            const Tensor& ta = h->tensors[r];
            const Tensor& tb = href->tensors[d.ref_row];
            jobs.push_back({ws + ta.off, d.fmt, ta.Cp, ws_b + tb.off, d.ref_fmt, tb.Cp, d.c, d.h * d.w, d.exponent, r});
        }
        jobs.push_back({heat_dev, esa::STATS_NCHW, 0, heat_ref_dev, esa::STATS_NCHW, 0, h->cfg.num_keypoints, height * width, 0, rows - 1});
        const int rc = esa::launch_diff(jobs.data(), (int)jobs.size(), n, ws + dp.off_parts, diff_dev, stream);
        if (rc) return fail("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
        return 0;
    };
    const int rc = body();
    h->keep = keep; href->keep = keep_ref;
    return rc;
}

static int tensor_diff_parts(const char* who, int fmt_a, int cp_a, int fmt_b, int cp_b, int exponent, int n, int c, int h, int w,
                             int* parts) {
    if (n < 1) return fail("%s: batch must be positive (got %d)", who, n);
    if (exponent < -ESAHRNET_SCALE_MAX_EXPONENT || exponent > ESAHRNET_SCALE_MAX_EXPONENT)
        return fail("%s: exponent %d outside -%d..%d", who, exponent, ESAHRNET_SCALE_MAX_EXPONENT, ESAHRNET_SCALE_MAX_EXPONENT);
    const bool nchw = fmt_a == esa::STATS_NCHW && fmt_b == esa::STATS_NCHW;
    if (!nchw && (fmt_a < esa::FMT_SB || fmt_a > esa::FMT_HF || fmt_b != esa::FMT_F32))
        return fail("%s: no scan for format %d against format %d (0..3 against 2, or -1 against -1)", who, fmt_a, fmt_b);
    const long long hw = (long long)h * w;
    *parts = h > 0 && w > 0 && hw <= 0x7fffffffLL ? esa::diff_parts(fmt_a, cp_a, fmt_b, cp_b, c, (int)hw) : 0;
    if (*parts <= 0)
        return fail("%s: no scan for %d channels (%d and %d padded), %dx%d (padded channels a multiple of 8 and at least the "
                    "channels; an image below 2 GiB on either side)", who, c, cp_a, cp_b, h, w);
    return 0;
}

int esahrnet_tensor_diff_workspace_bytes(int fmt_a, int cp_a, int fmt_b, int cp_b, int n, int c, int h, int w, size_t* bytes) {
    if (!bytes) return fail("tensor_diff_workspace_bytes: null argument");
    int parts = 0;
    if (tensor_diff_parts("tensor_diff_workspace_bytes", fmt_a, cp_a, fmt_b, cp_b, 0, n, c, h, w, &parts)) return 1;
    *bytes = (size_t)parts * n * sizeof(esahrnet_diff_record);
    return 0;
}

int esahrnet_tensor_diff(const void* a_dev, int fmt_a, int cp_a, const void* b_dev, int fmt_b, int cp_b, int exponent,
                         int n, int c, int h, int w, void* ws_dev, size_t ws_bytes, void* diff_dev, esahrnet_stream stream) {
    if (!a_dev || !b_dev || !ws_dev || !diff_dev) return fail("tensor_diff: null argument");
    int parts = 0;
    if (tensor_diff_parts("tensor_diff", fmt_a, cp_a, fmt_b, cp_b, exponent, n, c, h, w, &parts)) return 1;
    const size_t need = (size_t)parts * n * sizeof(esahrnet_diff_record);
    if (ws_bytes < need) return fail("tensor_diff: workspace too small (%zu < %zu)", ws_bytes, need);
    if (fmt_a != esa::STATS_NCHW && ((reinterpret_cast<uintptr_t>(a_dev) | reinterpret_cast<uintptr_t>(b_dev)) & 15))
        return fail("tensor_diff: a_dev and b_dev must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(a_dev) | reinterpret_cast<uintptr_t>(b_dev)) & 3)
        return fail("tensor_diff: a_dev and b_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(ws_dev) & 7) return fail("tensor_diff: workspace must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(diff_dev) & 7) return fail("tensor_diff: diff_dev must be 8-byte aligned");
    const esa::DiffJob job{a_dev, fmt_a, cp_a, b_dev, fmt_b, cp_b, c, h * w, exponent, 0};
    const int rc = esa::launch_diff(&job, 1, n, ws_dev, diff_dev, static_cast<hipStream_t>(stream));
    if (rc) return fail("tensor_diff: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

}  // extern "C"
