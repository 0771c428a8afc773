// plan.h — what the host units behind the handle entries share (plan_build.hip: configuration -> static plan; plan.hip: handle,
// weights, per-shape plan; forward.hip; loader.hip; report.hip): the plan's types, the handle, a forward's request and buffers,
// and the functions one unit calls in another.  Private to csrc; nothing here is exported.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/esahrnet.h"
#include "host_util.h"

#pragma GCC visibility push(hidden)
namespace esa {

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

struct ScaleRange { int c0, c1, group; };      // scale_conv_info: input channels [c0, c1) of a convolution lie in this scale group

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

}  // namespace esa

struct esahrnet_ctx {
    esahrnet_cfg cfg;
    int device;
    std::vector<esa::ConvSpec> specs;
    std::map<std::string, int> spec_by_name;
    std::vector<esa::DevConv> dconvs;
    std::vector<esa::AuxSpec> aux;
    float *stemraw_w = nullptr, *stemraw_b = nullptr;     // variant 1: un-normalised conv1 for the skip
    std::vector<esa::Tensor> tensors;
    std::vector<esa::Op> ops;
    int spec_stem = -1, spec_final = -1;
    float *stem_w = nullptr, *stem_b = nullptr, *final_w = nullptr, *final_b = nullptr;
    void* final_wpk = nullptr;  // output_layer weights as MFMA fragments (head.hip, final_mfma_kernel)
    int spec_l0 = -1, spec_l3 = -1, head_c0 = 0;     // fused head (OP_HEAD)
    void *head_w0 = nullptr, *head_w3 = nullptr;
    float *head_b0 = nullptr, *head_b3 = nullptr;
    bool committed = false;
    bool keep = false;
    esa::PlanOptions opt;
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
    esa::ShapePlan sp;
    int max_level = 0;
    int nhost_specs = -1;       // specs [nhost_specs, end) are derived (ConvSpec::parent); -1: none
    int stemraw_partial = -1;   // seg_hrnet3: tensor of the pooled partials of the raw stem output when the stem kernel makes them
    std::vector<esa::Multi> multis;
    std::vector<esa::JobGroup> jobs;
    // fp16 scale groups (build_scale_groups; variant 0 in a 16-bit format, else none): the group of every tensor (-1: none), a
    // name per group, and the exponent the host gave each (tensor T of group g is stored as T * 2^-exps[g]; all zero by default)
    std::vector<int> tgroup;
    std::vector<std::string> gnames;
    std::vector<int32_t> exps;
    bool scaled() const { for (int32_t e : exps) if (e) return true; return false; }
    int gexp(int g) const { return g < 0 ? 0 : exps[g]; }
};

namespace esa {

int final_kt(int K);        // head.hip

// plan_build.hip: configuration and switches -> the static plan and its fp16 scale groups
PlanOptions plan_options(const esahrnet_cfg& g, const Format& format);
int build_plan(esahrnet_ctx& c);
int build_scale_groups(esahrnet_ctx& c);
int scale_conv_info(const esahrnet_ctx& c, int index, int* out_group, std::vector<ScaleRange>& ranges);
int scaled_conv(const esahrnet_ctx& c, int index, std::vector<float>& w, std::vector<float>& b, std::vector<int>* shift_at);

// plan.hip: the per-shape plan
void level_dims(const esahrnet_ctx& c, int h, int w, std::vector<int>& lh, std::vector<int>& lw);
int check_shape(int n, int h, int w);
ShapePlan shape_decisions(const esahrnet_ctx& c, int n, int h, int w);
int plan_shape(esahrnet_ctx& c, int n, int h, int w);
ConvParams multi_params(const esahrnet_ctx& c, const Multi& m, const ShapePlan& sp, char* ws);
ConvParams conv_params_of(const esahrnet_ctx& c, const Op& o, const ShapePlan& sp, char* ws);
CbamJob cbam_job(const esahrnet_ctx& c, const Op& o, const ShapePlan& sp, char* ws);
int stem_pools(const esahrnet_ctx& c, int height, int width);

// Device address of tensor `t` in the workspace `ws`.  Without a workspace (the per-shape decisions, op_desc_get) launch
// parameters are built for their shapes and flags only, and every tensor points at one non-null placeholder: the
// *_supported() predicates and conv_kernel_name() test some pointers (res, the multi-head outputs) against nullptr.
inline char* tensor_ptr(const esahrnet_ctx& c, char* ws, int t) {
    static char placeholder;
    return ws ? ws + c.tensors[t].off : &placeholder;
}

// forward.hip: a forward, its request and its workspace; the decoders' argument checks the loader entries repeat
Request make_request(Decoder d, void* kp, void* idx, void* hess = nullptr, void* fit = nullptr, void* status = nullptr,
                     void* cov = nullptr, void* info = nullptr, double cov_floor = 0.0, int M = 0, int nms_radius = 0,
                     int refine = -1);
Request make_candidates_request(void* cand, void* cidx, int M, int nms_radius);
int check_gaussfit_outputs(const char* who, const esahrnet_ctx& c, const Request& r);
int check_candidates_request(const char* who, const Request& r);
int check_refined_decoder(const char* who, int decoder);
int check_refined_request(const char* who, const Request& r, int decoder);
int forward_workspace_bytes(const char* who, esahrnet_handle h, int n, int height, int width, Decoder d, size_t* bytes, int refine = -1);
int run_op(const esahrnet_ctx& c, const Op& o, const ShapePlan& sp, const Buffers& b, hipStream_t stream, esahrnet_op_desc* desc);
int run_forward(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* part_dev, void* ws_dev,
                size_t ws_bytes, esahrnet_stream stream_, hipEvent_t* events, const Request* req, void* h0_part = nullptr,
                void* h0_rec = nullptr);

}  // namespace esa
#pragma GCC visibility pop
