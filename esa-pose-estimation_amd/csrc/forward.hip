// forward.hip — the forward of a handle: a request (which decoder, where its results go), the launch of every plan op (run_op: the
// one place a dispatch decision becomes a launch or its description), the wave executor, and the entries built on them: heat-maps,
// keypoints straight from the forward, workspace queries, op descriptions, taps.
#include <cstdarg>

#include "plan.h"

namespace esa {

// kernel and (printf-formatted) label of an op description
__attribute__((format(printf, 3, 4)))
static void describe(esahrnet_op_desc* d, const char* kernel, const char* label, ...) {
    snprintf(d->kernel, sizeof d->kernel, "%s", kernel);
    va_list ap;
    va_start(ap, label);
    vsnprintf(d->label, sizeof d->label, label, ap);
    va_end(ap);
}

// The one place a request is built, for the four forms the entries come in: (kp, idx), + hess, + fit and status, + cov, info and
// cov_floor.  Two rules are stated here and nowhere else: get_final computes no Hessian, so hess is ignored by it; cov and
// info belong to the Gaussian fit, and are ignored without it.  The candidates' form is (cand, cidx) in the place of (kp, idx),
// with M and r, and with `refine` (0..2) the decoder that refines every candidate and may write all of the other outputs.
Request make_request(Decoder d, void* kp, void* idx, void* hess, void* fit, void* status, void* cov, void* info, double cov_floor,
                     int M, int nms_radius, int refine) {
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
Request make_candidates_request(void* cand, void* cidx, int M, int nms_radius) {
    return make_request(DEC_CAND, cand, cidx, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, M, nms_radius);
}

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
    if (d == DEC_NONE) return s;
    if (d == DEC_CAND) {
        s.heat = pad256((size_t)planes * height * width * 4);
        if (refine >= 0) {
            s.cidx = pad256((size_t)planes * ESAHRNET_MAX_CANDIDATES * 4);
            s.at = esa::at_workspace_bytes(planes, height, width, refine);
        }
        return s;
    }
    if (c.cfg.variant != 1 && c.opt.final_mfma) s.heat = pad256((size_t)planes * height * width * 4);
    if (d == DEC_FINAL2) {
        if (c.cfg.variant == 1 || c.opt.final_mfma) {
            s.ntiles = esa::final2_tiles(height, width);
            s.part = esa::final2_workspace_bytes(planes, height, width);
        } else {
            s.ntiles = esa::final2_valu_tiles(height, width);
            s.part = pad256((size_t)planes * s.ntiles * 8);
            s.bmax = pad256((size_t)planes * s.ntiles * 4);
        }
        return s;
    }
    s.ntiles = c.cfg.variant == 1 ? esa::to_nchw_part_tiles(height, width)
             : c.opt.final_mfma ? esa::final_part_tiles(K, c.cfg.cin, height, width)
                                : esa::final_kp_tiles(K, c.cfg.cin, height, width);
    s.part = pad256((size_t)planes * s.ntiles * 8);
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
int run_op(const esahrnet_ctx& c, const Op& o, const ShapePlan& sp, const Buffers& b, hipStream_t stream, esahrnet_op_desc* desc) {
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
            if (ti.Cp != d.cinp || to.Cp != d.coutp) return set_error("plan bug: channel mismatch at %s", s.name.c_str());
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
            if (ti.Cp != 32 || to.Cp != 32) return set_error("plan bug: bblock32 on a non-32-channel tensor");
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
                    return set_error("forward: fused head does not support this shape (%dx%d)", p.H, p.W);
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
                if (ti.Cp != to.Cp) return set_error("plan bug: fuse channel mismatch");
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
    if (rc) return set_error("forward: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

// req == nullptr: heat-maps into heat_dev (and, with part_dev, their per-tile maxima).  Otherwise the decoder of *req runs in
// place of the last launch and nothing but its outputs reaches caller memory (heat_dev and part_dev unused, req->kp never null)
int run_forward(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* part_dev, void* ws_dev,
                size_t ws_bytes, esahrnet_stream stream_, hipEvent_t* events, const Request* req, void* h0_part, void* h0_rec) {
    if (!h || !x_dev || !(heat_dev || req) || !ws_dev) return set_error("forward: null argument");
    if (!h->committed) return set_error("forward: esahrnet_commit has not been called");
    if (plan_shape(*h, n, height, width)) return 1;
    const KpScratch ks = kp_scratch(*h, n, height, width, req ? req->decoder : DEC_NONE, req ? req->refine : -1);
    if (check_workspace("forward", ws_dev, ws_bytes, h->sp.bytes + ks.total())) return 1;
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
    if (events && hipEventRecord(events[0], stream) != hipSuccess) return set_error("forward: hipEventRecord failed");
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
            if (o.join && join((size_t)op_index, o.join)) return set_error("forward: joining side lanes failed");
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
        if (events && hipEventRecord(events[op_index], stream) != hipSuccess) return set_error("forward: hipEventRecord failed");
    }
    if (multi && join(h->ops.size(), 0xeu)) return set_error("forward: joining the side lanes failed");
    return 0;
}

int forward_workspace_bytes(const char* who, esahrnet_handle h, int n, int height, int width, Decoder d, size_t* bytes, int refine) {
    if (!h || !bytes) return set_error("%s: null argument", who);
    if (plan_shape(*h, n, height, width)) return 1;
    *bytes = h->sp.bytes + kp_scratch(*h, n, height, width, d, refine).total();
    return 0;
}

// what esahrnet_forward_keypoints_gaussfit and the loader in front of it refuse about the decoder's outputs
int check_gaussfit_outputs(const char* who, const esahrnet_ctx& c, const Request& r) {
    if ((reinterpret_cast<uintptr_t>(r.kp) | reinterpret_cast<uintptr_t>(r.idx) | reinterpret_cast<uintptr_t>(r.status)) & 3)
        return set_error("%s: kp_dev, idx_dev and status_dev must be 4-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(r.fit) | reinterpret_cast<uintptr_t>(r.hess)) & 7)
        return set_error("%s: fit_dev and hess_dev must be 8-byte aligned", who);
    if (c.cfg.variant != 1 && !c.opt.final_mfma && c.cfg.cin > 8)
        return set_error("%s: the VALU output layer's fit stages at most 8 input channels (this handle takes %d)", who, c.cfg.cin);
    return 0;
}

// what esahrnet_forward_keypoints_candidates and the loader in front of it refuse about the decoder's arguments
int check_candidates_request(const char* who, const Request& r) {
    if (r.M < 1 || r.M > ESAHRNET_MAX_CANDIDATES)
        return set_error("%s: %d candidates per heat-map unsupported (1..%d)", who, r.M, ESAHRNET_MAX_CANDIDATES);
    if (r.r < 0) return set_error("%s: negative nms_radius %d", who, r.r);
    if ((reinterpret_cast<uintptr_t>(r.cand) | reinterpret_cast<uintptr_t>(r.cidx)) & 3)
        return set_error("%s: cand_dev and cidx_dev must be 4-byte aligned", who);
    return 0;
}

// What esahrnet_forward_keypoints_candidates_refined and the loader in front of it refuse about the decoder's arguments, in the
// order include/esahrnet.h gives; `decoder` as the caller passed it.  The texts are those of esahrnet_keypoints_candidates_refined.
int check_refined_decoder(const char* who, int decoder) {
    if (decoder < 0 || decoder > 2) return set_error("%s: decoder=%d unknown (0: get_final, 1: get_final2, 2: gaussfit)", who, decoder);
    return 0;
}
int check_refined_request(const char* who, const Request& r, int decoder) {
    if (r.M < 1 || r.M > ESAHRNET_MAX_CANDIDATES)
        return set_error("%s: %d candidates per heat-map unsupported (1..%d)", who, r.M, ESAHRNET_MAX_CANDIDATES);
    if (r.r < 0) return set_error("%s: negative nms_radius %d", who, r.r);
    if (check_refined_decoder(who, decoder)) return 1;
    if (decoder == 0 && (r.hess || r.fit || r.cov || r.info))
        return set_error("%s: decoder 0 (get_final) writes no hess_dev, fit_dev, cov_dev or info_dev: pass NULL", who);
    if (decoder == 1 && (r.fit || r.cov || r.info))
        return set_error("%s: decoder 1 (get_final2) writes no fit_dev, cov_dev or info_dev: pass NULL", who);
    if (decoder == 2 && !r.status) return set_error("%s: decoder 2 (gaussfit) needs status_dev", who);
    if (!(r.cov_floor >= 0.0) || !std::isfinite(r.cov_floor))
        return set_error("%s: cov_floor must be a finite number >= 0 (got %g)", who, r.cov_floor);
    if ((reinterpret_cast<uintptr_t>(r.cand) | reinterpret_cast<uintptr_t>(r.cidx) | reinterpret_cast<uintptr_t>(r.status)) & 3)
        return set_error("%s: cand_dev, cidx_dev and status_dev must be 4-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(r.hess) | reinterpret_cast<uintptr_t>(r.fit) | reinterpret_cast<uintptr_t>(r.cov) |
         reinterpret_cast<uintptr_t>(r.info)) & 7)
        return set_error("%s: hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned", who);
    return 0;
}

}  // namespace esa

using namespace esa;

extern "C" {

int esahrnet_forward(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                     void* heat_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    return run_forward(h, x_dev, n, height, width, heat_dev, nullptr, ws_dev, ws_bytes, stream, nullptr, nullptr);
}

int esahrnet_forward_timed(esahrnet_handle h, const void* x_dev, int n, int height, int width,
                           void* heat_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream,
                           float* ms_out) {
    if (!h || !ms_out) return set_error("forward_timed: null argument");
    const size_t nops = h->ops.size();
    std::vector<hipEvent_t> ev(nops + 1, nullptr);
    hipEvent_t nul[2] = {nullptr, nullptr};
    int rc = 0;
    for (size_t i = 0; i <= nops && !rc; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = set_error("forward_timed: hipEventCreate failed");
    for (int i = 0; i < 2 && !rc; ++i)
        if (hipEventCreate(&nul[i]) != hipSuccess) rc = set_error("forward_timed: hipEventCreate failed");
    // the cost of an empty event bracket on this stream is measured and subtracted, so that the
    // per-launch figures are kernel time (comparable with rocprofv3 --kernel-trace), not kernel + marker
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!rc && (hipEventRecord(nul[0], st) != hipSuccess || hipEventRecord(nul[1], st) != hipSuccess))
        rc = set_error("forward_timed: hipEventRecord failed");
    if (!rc) rc = run_forward(h, x_dev, n, height, width, heat_dev, nullptr, ws_dev, ws_bytes, stream, ev.data(), nullptr);
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = set_error("forward_timed: stream sync failed");
    float null_ms = 0.f;
    if (!rc && hipEventElapsedTime(&null_ms, nul[0], nul[1]) != hipSuccess) rc = set_error("forward_timed: hipEventElapsedTime failed");
    for (size_t i = 0; i < nops && !rc; ++i) {
        if (hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]) != hipSuccess) rc = set_error("forward_timed: hipEventElapsedTime failed");
        ms_out[i] = ms_out[i] > null_ms ? ms_out[i] - null_ms : 0.f;
    }
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : nul) if (e) (void)hipEventDestroy(e);
    return rc;
}

int esahrnet_op_desc_get(esahrnet_handle h, int index, int n, int height, int width, esahrnet_op_desc* out) {
    if (!h || !out || index < 0 || index >= (int)h->ops.size()) return set_error("op_desc_get: bad argument");
    if (check_shape(n, height, width)) return 1;
    memset(out, 0, sizeof *out);
    return run_op(*h, h->ops[index], shape_decisions(*h, n, height, width), Buffers{}, nullptr, out);
}

int esahrnet_partial_tiles(esahrnet_handle h, int height, int width, int* ntiles) {
    if (!h || !ntiles) return set_error("partial_tiles: null argument");
    if (!h->committed) return set_error("partial_tiles: esahrnet_commit has not been called");
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
        if (nt <= 0) return set_error("forward_partials: this handle's output layer does not report per-tile maxima (esahrnet_partial_tiles = 0)");
    }
    return run_forward(h, x_dev, n, height, width, heat_dev, part_dev, ws_dev, ws_bytes, stream, nullptr, nullptr);
}

// ---- the workspace of a forward: the plan's tensors, then the decoder's scratch ----------------------------------------
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
    if (!h || !r.kp) return set_error("%s: null argument", who);
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

// esahrnet_forward_keypoints_gaussfit and, with_cov, esahrnet_forward_keypoints_gaussfit_cov
static int forward_gaussfit(const char* who, bool with_cov, esahrnet_handle h, const void* x_dev, int n, int height, int width,
                            const Request& r, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    if (!h || !x_dev || !r.kp || !r.status || !ws_dev) return set_error("%s: null argument", who);
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

int esahrnet_forward_keypoints_candidates(esahrnet_handle h, const void* x_dev, int n, int height, int width, int candidates,
                                          int nms_radius, void* cand_dev, void* cidx_dev, void* ws_dev, size_t ws_bytes,
                                          esahrnet_stream stream) {
    const char* who = "forward_keypoints_candidates";
    const Request r = make_candidates_request(cand_dev, cidx_dev, candidates, nms_radius);
    if (!h || !r.cand) return set_error("%s: null argument", who);
    if (check_candidates_request(who, r)) return 1;
    return run_forward(h, x_dev, n, height, width, nullptr, nullptr, ws_dev, ws_bytes, stream, nullptr, &r);
}

// ---- the candidates refined at their own pixels, in the forward (keypoints_at.hip behind the search) -------------------------
int esahrnet_keypoints_candidates_refined_forward_workspace_bytes(esahrnet_handle h, int n, int height, int width, int decoder,
                                                                  size_t* bytes) {
    const char* who = "keypoints_candidates_refined_forward_workspace_bytes";
    if (!h || !bytes) return set_error("%s: null argument", who);
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
    if (!h || !r.cand) return set_error("%s: null argument", who);
    if (check_refined_request(who, r, decoder)) return 1;
    return run_forward(h, x_dev, n, height, width, nullptr, nullptr, ws_dev, ws_bytes, stream, nullptr, &r);
}

int esahrnet_flops_per_crop(esahrnet_handle h, int height, int width, double* flops) {
    if (!h || !flops) return set_error("flops_per_crop: null argument");
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
    if (!h || !out) return set_error("tap_name: null argument");
    int n = 0;
    for (const Tensor& t : h->tensors)
        if (!t.tap.empty() && n++ == index) { snprintf(out, cap, "%s", t.tap.c_str()); return 0; }
    return set_error("tap_name: index %d out of range", index);
}

static const Tensor* find_tap(esahrnet_handle h, const char* name) {
    for (const Tensor& t : h->tensors)
        if (t.tap == name) return &t;
    return nullptr;
}

int esahrnet_tap_shape(esahrnet_handle h, const char* name, int height, int width, int* c, int* th, int* tw) {
    if (!h || !name || !c || !th || !tw) return set_error("tap_shape: null argument");
    const Tensor* t = find_tap(h, name);
    if (!t) return set_error("tap_shape: no tensor named '%s'", name);
    std::vector<int> lh, lw;
    level_dims(*h, height, width, lh, lw);
    *c = t->C; *th = lh[t->level]; *tw = lw[t->level];
    return 0;
}

int esahrnet_tap_read(esahrnet_handle h, const char* name, int n, int height, int width,
                      const void* ws_dev, void* out_dev, esahrnet_stream stream) {
    if (!h || !name || !ws_dev || !out_dev) return set_error("tap_read: null argument");
    if (!h->keep) return set_error("tap_read: call esahrnet_set_debug_keep(h, 1) before the forward (buffers are recycled otherwise)");
    const Tensor* t = find_tap(h, name);
    if (!t) return set_error("tap_read: no tensor named '%s'", name);
    if (plan_shape(*h, n, height, width)) return 1;
    if (t->alt != 0 && t->alt != (h->sp.head2 ? 2 : 1))
        return set_error("tap_read: '%s' belongs to the head alternative that does not run at this shape", name);
    // a tensor stored as T * 2^-e (fp16 scale exponents) comes back as T: the conversion takes the factor
    const int e = h->gexp(h->tgroup[t - h->tensors.data()]);
    const int rc = e ? esa::launch_hf_to_nchw_scaled(static_cast<const char*>(ws_dev) + t->off, n, t->C, h->sp.lh[t->level],
                                                     h->sp.lw[t->level], t->Cp, static_cast<float*>(out_dev), ldexpf(1.f, e),
                                                     static_cast<hipStream_t>(stream))
                     : esa::launch_fmt_to_nchw(t->f32 ? esa::FMT_F32 : h->opt.fmt,
        static_cast<const char*>(ws_dev) + t->off, n, t->C, h->sp.lh[t->level], h->sp.lw[t->level], t->Cp,
        static_cast<float*>(out_dev), static_cast<hipStream_t>(stream));
    if (rc) return set_error("tap_read: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

}  // extern "C"
