// plan.hip — host runtime behind the C-ABI (include/esahrnet.h): the handle's lifetime, weight packing, the per-shape plan
// (dispatch decisions, workspace planning).  The stage table -> static plan (list of fused kernels over SB tensors) is
// plan_build.hip; the other entries that take a handle are in forward.hip, loader.hip and report.hip (what they share: plan.h);
// the ones that take none are in abi_decode.hip and op_abi.hip (the stand-alone operator entries, esahrnet_op_*).
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
#include <cstdarg>

#include "plan.h"

static thread_local char g_err[512] = "";

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

namespace esa {

void level_dims(const esahrnet_ctx& c, int h, int w, std::vector<int>& lh, std::vector<int>& lw) {
    lh.assign(c.max_level + 1, 0);
    lw.assign(c.max_level + 1, 0);
    lh[0] = h; lw[0] = w;
    for (int l = 1; l <= c.max_level; ++l) { lh[l] = (lh[l - 1] + 1) / 2; lw[l] = (lw[l - 1] + 1) / 2; }
}

int check_shape(int n, int h, int w) {
    if (n <= 0) return set_error("batch must be positive (got %d)", n);
    if (h < 16 || w < 16 || (h & 1) || (w & 1))
        return set_error("crop %dx%d: height and width must be even and >= 16 "
                         "(UpsamplingBilinear2d(x2) output must match the crop, seg_hrnet.py:330,469)", h, w);
    return 0;
}

// does this input shape run the second-generation head (ops with alt == 2)?
static bool head2_for_shape(const esahrnet_ctx& c, const std::vector<int>& lh, const std::vector<int>& lw, bool* ulo) {
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
static bool job_on_for(const esahrnet_ctx& c, const JobGroup& g, const ShapePlan& sp) {
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

static bool cbam_fused(const esahrnet_ctx& c, int Cp, int hh, int ww) {
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
static size_t tensor_bytes(const esahrnet_ctx& c, const ShapePlan& sp, const Tensor& t) {
    const size_t wpix = t.tlayout ? (size_t)esa::head_t_xp(sp.lw[t.level]) : (size_t)sp.lw[t.level];
    size_t b = t.flat ? (size_t)sp.n * t.flat * 4 : (size_t)sp.n * sp.lh[t.level] * wpix * t.Cp * (t.f32 ? 4 : c.eb());
    return pad256(b);
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
                return set_error("crop %dx%d: the interpolation windows of seg_hrnet3's last_layer[0] do not fit the gather kernel's LDS "
                                 "budget (set ESAHRNET_HEAD3_DIRECT=1 before creating the net for the direct 480-channel 3x3)", h, w);
        } else if (o.kind >= OP_POOL && o.kind <= OP_APPLY) {
            // a CBAM step, alone or in a merged launch: cbam_job_blocks holds the predicates of every CBAM launcher, and
            // none of them depends on the batch
            esa::CbamJob q = cbam_job(c, o, sp, nullptr);
            if (q.kind >= 0 && esa::cbam_job_blocks(q) < 1) {
                static const char* steps[] = {"channel pooling", "channel-attention MLP", "spatial maps", "apply", "spatial attention"};
                const std::string& a = c.aux[o.aux[0]].name;        // "<layer>.ca.fc.0.weight"; the stem skip's has no layer
                const std::string layer = a.size() > 15 ? "'" + a.substr(0, a.size() - 15) + "'" : "the stem skip";
                return set_error("seg_hrnet3: no kernel serves the CBAM %s of %s at %d channels (%d padded)", steps[q.kind],
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

static void free_weights(esahrnet_ctx& c) {
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

}  // namespace esa

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

using namespace esa;

// ============================================ C ABI ============================================
extern "C" {

const char* esahrnet_last_error(void) { return g_err; }
int esahrnet_abi_version(void) { return ESAHRNET_ABI_VERSION; }

int esahrnet_create(const esahrnet_cfg* cfg, int device, esahrnet_handle* out) {
    if (!cfg || !out) return set_error("esahrnet_create: null argument");
    if (cfg->final_conv_kernel != 1) return set_error("FINAL_CONV_KERNEL=%d unsupported (reference default 1)", cfg->final_conv_kernel);
    if (cfg->cin < 1 || cfg->cin > 4) return set_error("cin=%d unsupported (1..4)", cfg->cin);
    if (cfg->num_keypoints < 1 || esa::final_kt(cfg->num_keypoints) < 0) return set_error("num_keypoints=%d unsupported (1..32)", cfg->num_keypoints);
    if (cfg->stem_width < 1 || cfg->blocks[0][0] < 1) return set_error("bad stem_width/blocks");
    if (cfg->variant != 0 && cfg->variant != 1) return set_error("variant=%d unsupported (0: seg_hrnet/2, 1: seg_hrnet3)", cfg->variant);
    if (cfg->precision < 0 || cfg->precision > 3)
        return set_error("precision=%d unsupported (0..3 — 0: split-bf16 'bf16x3', 1: bf16, 2: fp32-grade 'bf16x6', 3: fp16)", cfg->precision);
    if (cfg->precision == 3 && cfg->variant == 1)
        return set_error("precision=3 (fp16) is not built for variant 1 (seg_hrnet3): its CBAM kernels have no fp16 form; "
                         "seg_hrnet / seg_hrnet2 take it, seg_hrnet3 takes 0, 1 or 2");
    if (cfg->variant == 1) {
        if (cfg->stem_width % 16) return set_error("variant 1: stem_width must be a multiple of 16 (ChannelAttention ratio)");
        for (int b = 0; b < ESAHRNET_MAX_BRANCHES; ++b)
            if (cfg->blocks[3][b] > 0 && (cfg->widths[b] < 16 || cfg->widths[b] % 8))
                return set_error("variant 1: branch widths must be >= 16 and multiples of 8 (got %d)", cfg->widths[b]);
    }
    for (int s = 1; s < 4; ++s)
        if (cfg->modules[s] < 1) return set_error("NUM_MODULES of stage %d must be >= 1", s + 1);
    for (int b = 0; b < ESAHRNET_MAX_BRANCHES; ++b)
        if (cfg->blocks[3][b] > 0 && cfg->widths[b] < 1) return set_error("width of branch %d must be positive", b);
    // the job keys of group_jobs pack (stage << 4 | module) above an 8-bit depth field in which the branch convolutions take
    // (2 or 6) * block + 0..5, the fuse-up 1x1s 100 and the fuse-down links 128 + k: reject stage tables that overflow either
    for (int s = 0; s < 4; ++s) {
        if (cfg->modules[s] > 15) return set_error("NUM_MODULES of stage %d is %d (at most 15)", s + 1, cfg->modules[s]);
        for (int b = 0; b < ESAHRNET_MAX_BRANCHES; ++b)
            if ((cfg->variant == 1 ? 6 : 2) * cfg->blocks[s][b] + (cfg->variant == 1 ? 5 : 1) >= 100)
                return set_error("NUM_BLOCKS of stage %d branch %d is %d (at most %d)", s + 1, b, cfg->blocks[s][b], cfg->variant == 1 ? 15 : 49);
    }
    esahrnet_ctx* c = new esahrnet_ctx();
    c->cfg = *cfg;
    c->device = device;
    c->format = esa::Format(cfg->precision);
    c->opt = plan_options(*cfg, c->format);
    // fp16 tensors reach the output layer through the matrix-core kernel only (head.hip final_mfma_kernel<.., HF>)
    if (c->hf() && !c->opt.final_mfma) {
        delete c;
        return set_error("precision=3 (fp16) needs the matrix-core output layer: unset ESAHRNET_FINAL_VALU (num_keypoints=%d, cin=%d)",
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

int esahrnet_debug_op_schedule(esahrnet_handle h, int index, int* wave, int* lane) {
    if (!h || !wave || !lane || index < 0 || index >= (int)h->ops.size()) return set_error("debug_op_schedule: bad argument");
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
    if (!h || !count) return set_error("debug_op_count: null argument");
    if (plan_shape(*h, n, height, width)) return 1;
    *count = (int)active_ops(*h).size();
    return 0;
}

int esahrnet_debug_op_regions(esahrnet_handle h, int n, int height, int width, int k, esahrnet_debug_op* out) {
    if (!h || !out) return set_error("debug_op_regions: null argument");
    if (plan_shape(*h, n, height, width)) return 1;
    const std::vector<int> idx = active_ops(*h);
    if (k < 0 || k >= (int)idx.size()) return set_error("debug_op_regions: op %d out of range (%zu run at this shape)", k, idx.size());
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
    if (!h || !out || i < 0 || i >= host_specs(h)) return set_error("conv_desc_get: bad index %d", i);
    const ConvSpec& s = h->specs[i];
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", s.name.c_str());
    snprintf(out->bn, sizeof out->bn, "%s", s.bn.c_str());
    out->cin = s.cin; out->cout = s.cout; out->k = s.k; out->stride = s.stride;
    out->has_bias = s.has_bias; out->relu = s.relu;
    return 0;
}

int esahrnet_set_conv(esahrnet_handle h, int i, const float* w, const float* b) {
    if (!h || !w || !b || i < 0 || i >= host_specs(h)) return set_error("set_conv: bad argument (index %d)", i);
    ConvSpec& s = h->specs[i];
    const size_t nw = (size_t)s.cout * s.cin * s.k * s.k;
    s.w.assign(w, w + nw);
    s.b.assign(b, b + s.cout);
    for (size_t j = 0; j < nw; ++j)
        if (!std::isfinite(s.w[j])) return set_error("set_conv(%s): non-finite weight", s.name.c_str());
    s.set = true;
    return 0;
}

int esahrnet_aux_count(esahrnet_handle h) { return h ? (int)h->aux.size() : -1; }

int esahrnet_aux_desc_get(esahrnet_handle h, int i, esahrnet_aux_desc* out) {
    if (!h || !out || i < 0 || i >= (int)h->aux.size()) return set_error("aux_desc_get: bad index %d", i);
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", h->aux[i].name.c_str());
    for (int k = 0; k < 4; ++k) out->shape[k] = h->aux[i].shape[k];
    return 0;
}

int esahrnet_set_aux(esahrnet_handle h, int i, const float* w) {
    if (!h || !w || i < 0 || i >= (int)h->aux.size()) return set_error("set_aux: bad argument (index %d)", i);
    AuxSpec& a = h->aux[i];
    const size_t n = (size_t)a.shape[0] * a.shape[1] * a.shape[2] * a.shape[3];
    a.data.assign(w, w + n);
    for (float v : a.data) if (!std::isfinite(v)) return set_error("set_aux(%s): non-finite value", a.name.c_str());
    a.set = true;
    return 0;
}

int esahrnet_commit(esahrnet_handle h) {
    if (!h) return set_error("commit: null handle");
    for (ConvSpec& s : h->specs) {
        if (s.parent < 0) continue;
        const ConvSpec& ps = h->specs[s.parent];
        if (!ps.set) return set_error("commit: weights of '%s' were never set", ps.name.c_str());
        s.w.assign((size_t)s.cout * s.cin, 0.f);
        s.b.assign(s.cout, 0.f);
        for (int co = 0; co < ps.cout; ++co)
            for (int t = 0; t < 9; ++t)
                for (int ci = 0; ci < s.cin; ++ci)
                    s.w[(size_t)((co >> 3) * 72 + t * 8 + (co & 7)) * s.cin + ci] = ps.w[((size_t)co * ps.cin + s.pc0 + ci) * 9 + t];
        s.set = true;
    }
    for (const ConvSpec& s : h->specs)
        if (!s.set) return set_error("commit: weights of '%s' were never set", s.name.c_str());
    for (const AuxSpec& a : h->aux)
        if (!a.set) return set_error("commit: tensor '%s' was never set", a.name.c_str());
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
                    return set_error("commit: weight %g of '%s' is not finite in fp16 (|w| must stay below 65520; scale shift 2^%d): precision "
                                     "'fp16' cannot hold this network, use 'bf16'", (double)s.w[j], s.name.c_str(),
                                     shifts[i].empty() ? 0 : shifts[i][(j / ((size_t)s.k * s.k)) % s.cin]);
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error("commit: no HIP device visible — the MI355X kernels cannot run (no CPU fallback exists)");
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
    if (!h || !groups) return set_error("scale_groups: null argument");
    *groups = (int)h->gnames.size();
    return 0;
}

int esahrnet_scale_group_name(esahrnet_handle h, int group, char* out, size_t cap) {
    if (!h || !out || !cap) return set_error("scale_group_name: null argument");
    if (group < 0 || group >= (int)h->gnames.size()) return set_error("scale_group_name: group %d out of range (%zu groups)", group, h->gnames.size());
    snprintf(out, cap, "%s", h->gnames[group].c_str());
    return 0;
}

int esahrnet_scale_conv_get(esahrnet_handle h, int index, esahrnet_scale_conv* out) {
    if (!h || !out) return set_error("scale_conv_get: null argument");
    if (index < 0 || index >= host_specs(h)) return set_error("scale_conv_get: bad index %d", index);
    std::vector<ScaleRange> ranges;
    int og = -1;
    if (scale_conv_info(*h, index, &og, ranges)) return 1;
    if (ranges.size() > ESAHRNET_SCALE_MAX_RANGES) return set_error("scale_conv_get: '%s' reads %zu ranges", h->specs[index].name.c_str(), ranges.size());
    memset(out, 0, sizeof *out);
    out->out_group = og;
    out->nranges = (int)ranges.size();
    for (size_t i = 0; i < ranges.size(); ++i) { out->c0[i] = ranges[i].c0; out->c1[i] = ranges[i].c1; out->in_group[i] = ranges[i].group; }
    return 0;
}

int esahrnet_scale_row_group(esahrnet_handle h, int row, int* group) {
    if (!h || !group) return set_error("scale_row_group: null argument");
    const int nt = (int)h->tensors.size();
    if (row < 0 || row > nt) return set_error("scale_row_group: row %d out of range (0..%d)", row, nt);
    *group = row == nt ? -1 : h->tgroup[row];
    return 0;
}

int esahrnet_set_scale_exponents(esahrnet_handle h, const int32_t* exponents, int count) {
    if (!h || (!exponents && count)) return set_error("set_scale_exponents: null argument");
    if (count != (int)h->gnames.size())
        return set_error("set_scale_exponents: %d exponents for a handle with %zu scale groups", count, h->gnames.size());
    for (int g = 0; g < count; ++g) {
        if (exponents[g] < -ESAHRNET_SCALE_MAX_EXPONENT || exponents[g] > ESAHRNET_SCALE_MAX_EXPONENT)
            return set_error("set_scale_exponents: exponent %d of group %d ('%s') is outside [-%d, %d]", exponents[g], g, h->gnames[g].c_str(),
                             ESAHRNET_SCALE_MAX_EXPONENT, ESAHRNET_SCALE_MAX_EXPONENT);
        if (exponents[g] && h->cfg.precision != 3)
            return set_error("set_scale_exponents: a non-zero exponent (group %d, '%s': %d) needs precision 3 (fp16); this handle has precision %d, "
                             "whose format has f32's exponent range", g, h->gnames[g].c_str(), exponents[g], h->cfg.precision);
    }
    h->exps.assign(exponents, exponents + count);
    h->committed = false;       // the packed weights on the device belong to the old exponents: esahrnet_commit again
    return 0;
}

int esahrnet_get_scale_exponents(esahrnet_handle h, int32_t* exponents, int count) {
    if (!h || (!exponents && count)) return set_error("get_scale_exponents: null argument");
    if (count != (int)h->exps.size()) return set_error("get_scale_exponents: room for %d exponents, the handle has %zu scale groups", count, h->exps.size());
    std::copy(h->exps.begin(), h->exps.end(), exponents);
    return 0;
}

int esahrnet_debug_scaled_conv(esahrnet_handle h, int index, float* w, float* b) {
    if (!h || !w || !b) return set_error("debug_scaled_conv: null argument");
    if (index < 0 || index >= host_specs(h)) return set_error("debug_scaled_conv: bad index %d", index);
    if (!h->specs[index].set) return set_error("debug_scaled_conv: weights of '%s' were never set", h->specs[index].name.c_str());
    std::vector<float> sw, sb;
    if (scaled_conv(*h, index, sw, sb, nullptr)) return 1;
    std::copy(sw.begin(), sw.end(), w);
    std::copy(sb.begin(), sb.end(), b);
    return 0;
}

int esahrnet_scale_exponents_from_stats(esahrnet_handle h, const void* records, int rows, int n_total, const void* h0_records,
                                        int headroom_bits, int32_t* exponents, int count) {
    if (!h || !records || !exponents) return set_error("scale_exponents_from_stats: null argument");
    const int ng = (int)h->gnames.size();
    if (!ng) return set_error("scale_exponents_from_stats: this handle has no scale groups (variant 0 with precision 1 or 3 only)");
    if (count != ng) return set_error("scale_exponents_from_stats: room for %d exponents, the handle has %d scale groups", count, ng);
    if (rows != (int)h->tensors.size() + 1) return set_error("scale_exponents_from_stats: %d rows, the handle's report has %zu", rows, h->tensors.size() + 1);
    if (n_total < 1) return set_error("scale_exponents_from_stats: n_total must be positive (got %d)", n_total);
    if (headroom_bits < 0 || headroom_bits > 14) return set_error("scale_exponents_from_stats: headroom_bits %d outside 0..14", headroom_bits);
    const esahrnet_stats_record* rec = static_cast<const esahrnet_stats_record*>(records);
    const esahrnet_stats_record* h0 = static_cast<const esahrnet_stats_record*>(h0_records);
    std::vector<float> top(ng, 0.f);
    for (int r = 0; r < rows; ++r)
        for (int i = 0; i < n_total; ++i) {
            const esahrnet_stats_record& v = rec[(size_t)r * n_total + i];
            if (v.n_nan || v.n_inf) {
                esahrnet_stats_row_desc d;
                const char* name = esahrnet_stats_row_get(h, r, 1, 64, 64, &d) ? "?" : d.name;
                return set_error("scale_exponents_from_stats: row %d ('%s') holds %u NaN and %u infinite values in crop %d: no exponent cures that",
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
                return set_error("scale_exponents_from_stats: h0 holds %u NaN and %u infinite values in crop %d", h0[i].n_nan, h0[i].n_inf, i);
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
    if (!h) return set_error("null handle");
    h->keep = keep != 0;
    return 0;
}

}  // extern "C"
