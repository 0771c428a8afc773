// op_abi.hip — the stand-alone operator entries of include/esahrnet.h (esahrnet_op_conv .. esahrnet_op_tile_max, test use only):
// one kernel or one launcher on f32 NCHW tensors of the caller.  None takes a handle or knows esahrnet_ctx (esahrnet_op_desc_get
// does, and is in forward.hip).  Each checks its arguments before its first HIP call, reports through esa::set_error, keeps its
// device memory in a DevScope and ends in DevScope::finish (host_util.h); the format of a precision code is esa::Format.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/esahrnet.h"
#include "host_util.h"
#include "kernels.h"

using esa::DevScope;
using esa::Format;
using esa::set_error;

static const float* f32(const void* p) { return static_cast<const float*>(p); }
static float* f32(void* p) { return static_cast<float*>(p); }
static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static bool conv_form_ok(int k, int stride) { return (k == 1 && stride == 1) || (k == 3 && (stride == 1 || stride == 2)); }
static bool op_conv_dims_ok(int n, int cin, int cout, int h, int w, int k, int stride) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || !conv_form_ok(k, stride)) return false;
    return (long long)n * h * w * (long long)((std::max(cin, cout) + 63) & ~63) * 4 <= 0x7fffffffLL;      // (test tensors)
}
// ConvParams of a stand-alone convolution — shapes and flags only; `res` stands for "there is a residual" until op_conv_device
// puts the device tensors in.  (No handle here: the call is its own create, and reads the reload switch itself.)
static esa::ConvParams op_conv_shape(const Format& f, int n, int cin, int cout, int h, int w, int stride, int relu, const void* res) {
    esa::ConvParams p{};
    p.N = n; p.H = h; p.W = w; p.OH = stride == 2 ? (h + 1) / 2 : h; p.OW = stride == 2 ? (w + 1) / 2 : w;
    p.Cinp = f.pad(cin); p.Coutp = f.pad(cout); p.relu = relu; p.fmt = f.fmt;
    p.res = static_cast<const char*>(res);
    p.x6_reload = esa::env_on("ESAHRNET_X6_RELOAD_WEIGHTS");
    return p;
}
// weights packed and uploaded, x and res converted to the format, y allocated, all in `m`; p's pointers set.  Non-zero: an error is
// set.  *rc: the conversions' launch error, for the caller to report in its own words.
static int op_conv_device(DevScope& m, const Format& f, esa::ConvParams& p, int cin, int cout, int k, const float* w, const float* b,
                          const void* x_dev, const void* res_dev, int* rc) {
    std::vector<float> bias(p.Coutp, 0.f);
    std::copy(b, b + cout, bias.begin());
    char *xs = nullptr, *rs = nullptr;
    if (m.upload(f.pack(w, cout, cin, k, p.Coutp, p.Cinp), &p.w) || m.upload(bias, &p.bias)) return 1;
    const size_t xb = (size_t)p.N * p.H * p.W * p.Cinp * f.eb, yb = (size_t)p.N * p.OH * p.OW * p.Coutp * f.eb;
    if (m.alloc(&xs, xb) || m.alloc(&p.y, yb) || (res_dev && m.alloc(&rs, yb))) return 1;
    *rc = esa::launch_nchw_to_fmt(f.fmt, f32(x_dev), p.N, cin, p.H, p.W, xs, p.Cinp, m.stream());
    if (!*rc && res_dev) *rc = esa::launch_nchw_to_fmt(f.fmt, f32(res_dev), p.N, cout, p.OH, p.OW, rs, p.Coutp, m.stream());
    p.x = xs; p.res = rs;
    return 0;
}

extern "C" {

int esahrnet_op_conv(const void* x_dev, int n, int cin, int height, int width, const float* w,
                     const float* b, int cout, int k, int stride, int relu, const void* res_dev,
                     void* y_dev, esahrnet_stream stream_) {
    return esahrnet_op_conv_ex(x_dev, n, cin, height, width, w, b, cout, k, stride, relu, res_dev, y_dev, 0, stream_);
}

int esahrnet_op_conv_ex(const void* x_dev, int n, int cin, int height, int width, const float* w,
                        const float* b, int cout, int k, int stride, int relu, const void* res_dev,
                        void* y_dev, int precision, esahrnet_stream stream_) {
    if (!x_dev || !w || !b || !y_dev) return set_error("op_conv: null argument");
    if (precision < 0 || precision > 3) return set_error("op_conv: precision %d", precision);
    if (!conv_form_ok(k, stride)) return set_error("op_conv: k=%d stride=%d unsupported", k, stride);
    const Format f(precision);
    DevScope m("op_conv", static_cast<hipStream_t>(stream_));
    esa::ConvParams p = op_conv_shape(f, n, cin, cout, height, width, stride, relu, res_dev);
    int rc = 0;
    if (op_conv_device(m, f, p, cin, cout, k, w, b, x_dev, res_dev, &rc)) return 1;
    if (!rc) rc = esa::launch_conv(p, k, stride, m.stream());
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, p.y, n, cout, p.OH, p.OW, p.Coutp, f32(y_dev), m.stream());      // the cout real channels
    return m.finish(rc);
}

int esahrnet_op_fuse(const void* const* xs_dev, const int* hs, const int* ws, int nterms, int n, int c,
                     int height, int width, int relu, void* y_dev, esahrnet_stream stream_) {
    return esahrnet_op_fuse_ex(xs_dev, hs, ws, nterms, n, c, height, width, relu, y_dev, 0, stream_);
}

int esahrnet_op_fuse_ex(const void* const* xs_dev, const int* hs, const int* ws, int nterms, int n, int c,
                        int height, int width, int relu, void* y_dev, int precision, esahrnet_stream stream_) {
    if (!xs_dev || !hs || !ws || !y_dev || nterms < 1 || nterms > 4) return set_error("op_fuse: bad argument");
    if (precision < 0 || precision > 3) return set_error("op_fuse: precision %d", precision);
    const Format f(precision);
    DevScope m("op_fuse", static_cast<hipStream_t>(stream_));
    const int cp = f.pad(c);
    int rc = 0;
    esa::FuseParams p{};
    p.nterms = nterms; p.N = n; p.H = height; p.W = width; p.Cp = cp; p.relu = relu; p.fmt = f.fmt;
    for (int i = 0; i < nterms && !rc; ++i) {
        char* x = nullptr;
        if (m.alloc(&x, (size_t)n * hs[i] * ws[i] * cp * f.eb)) return 1;
        rc = esa::launch_nchw_to_fmt(f.fmt, f32(xs_dev[i]), n, c, hs[i], ws[i], x, cp, m.stream());
        p.x[i] = x; p.h[i] = hs[i]; p.w[i] = ws[i];
    }
    if (!rc && m.alloc(&p.y, (size_t)n * height * width * cp * f.eb)) return 1;
    if (!rc) rc = esa::launch_fuse(p, m.stream());
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, p.y, n, c, height, width, cp, f32(y_dev), m.stream());
    return m.finish(rc);
}

int esahrnet_op_cbam(const void* x_dev, const void* res_dev, int n, int c, int height, int width, const float* w_fc0,
                     const float* w_fc2, const float* w_sa, int relu, void* y_dev, int cy, int c0, int fused, int precision,
                     esahrnet_stream stream_) {
    return esahrnet_op_cbam_steps(x_dev, res_dev, n, c, height, width, w_fc0, w_fc2, w_sa, relu, y_dev, cy, c0, fused, precision,
                                  0, nullptr, nullptr, nullptr, stream_);
}

int esahrnet_op_cbam_steps(const void* x_dev, const void* res_dev, int n, int c, int height, int width, const float* w_fc0,
                           const float* w_fc2, const float* w_sa, int relu, void* y_dev, int cy, int c0, int fused, int precision,
                           int slabs, void* partial_out, void* ca_out, void* maps_out, esahrnet_stream stream_) {
    if (!x_dev || !w_fc0 || !w_fc2 || !w_sa || !y_dev || n <= 0 || height <= 0 || width <= 0) return set_error("op_cbam: bad argument");
    if (precision < 0 || precision > 2) return set_error("op_cbam: precision %d", precision);
    if (c < 16 || (c & 7)) return set_error("op_cbam: c=%d (a multiple of 8, at least 16: ChannelAttention's ratio)", c);
    const Format f(precision);
    const int cp = f.pad(c), cyp = f.pad(cy);
    if (cp > 512) return set_error("op_cbam: c=%d is %d channels padded, ca_mlp serves at most 512", c, cp);
    if (c0 < 0 || (c0 & 7) || c0 + cp > cyp) return set_error("op_cbam: slice [%d, %d) outside the %d channels of y", c0, c0 + cp, cyp);
    if (fused && !esa::cbam_spatial_supported(cp)) return set_error("op_cbam: cbam_spatial does not serve %d channels", cp);
    if (fused && maps_out) return set_error("op_cbam: maps_out with fused = 1 (cbam_spatial keeps the maps in LDS)");
    if ((long long)height * width > 0x7fffffffLL / n) return set_error("op_cbam: %d x %d x %d pixels", n, height, width);
    const int cr = c / 16, hw = height * width;
    if (slabs < 0 || slabs > std::min(1024, hw)) return set_error("op_cbam: slabs=%d (0, or 1 .. min(1024, %d pixels))", slabs, hw);
    const int P = slabs ? slabs : std::min(esa::POOL_SLABS, hw);
    DevScope m("op_cbam", static_cast<hipStream_t>(stream_));
    hipStream_t stream = m.stream();
    const std::vector<float> h0(w_fc0, w_fc0 + (size_t)cr * c), h2(w_fc2, w_fc2 + (size_t)c * cr), hs(w_sa, w_sa + 98);
    char *xs = nullptr, *rs = nullptr, *ys = nullptr;
    float *part = nullptr, *ca = nullptr, *maps = nullptr, *w0 = nullptr, *w2 = nullptr, *wsa = nullptr;
    if (m.upload(h0, &w0) || m.upload(h2, &w2) || m.upload(hs, &wsa)) return 1;
    const size_t npix = (size_t)n * hw;
    const size_t part_bytes = (size_t)n * P * cp * 2 * sizeof(float), ca_bytes = (size_t)n * cp * sizeof(float),
                 maps_bytes = npix * 2 * sizeof(float);
    if (m.alloc(&xs, npix * cp * f.eb) || (res_dev && m.alloc(&rs, npix * cp * f.eb)) || m.alloc(&ys, npix * cyp * f.eb) ||
        m.alloc(&part, part_bytes) || m.alloc(&ca, ca_bytes) || m.alloc(&maps, maps_bytes)) return 1;
    int rc = esa::launch_nchw_to_fmt(f.fmt, f32(x_dev), n, c, height, width, xs, cp, stream);
    if (!rc && res_dev) rc = esa::launch_nchw_to_fmt(f.fmt, f32(res_dev), n, c, height, width, rs, cp, stream);
    if (!rc) rc = esa::launch_nchw_to_fmt(f.fmt, f32(y_dev), n, cy, height, width, ys, cyp, stream);
    if (!rc) rc = esa::launch_pool_partial(xs, part, n, hw, cp, P, stream, f.fmt);
    if (!rc) rc = esa::launch_ca_mlp(part, w0, w2, ca, n, hw, c, cp, cr, P, stream);
    esa::CbamApplyParams ap{};
    ap.x = xs; ap.res = rs; ap.ca = ca; ap.maps = maps; ap.w_sa = wsa; ap.y = ys;
    ap.N = n; ap.H = height; ap.W = width; ap.Cp = cp; ap.y_pix_bytes = cyp * f.eb; ap.y_c0 = c0; ap.relu = relu; ap.C = c; ap.fmt = f.fmt;
    if (!rc && fused) rc = esa::launch_cbam_spatial(ap, stream);
    if (!rc && !fused) rc = esa::launch_cbam_maps(ap.x, ap.ca, maps, n, hw, c, cp, stream, f.fmt);
    if (!rc && !fused) rc = esa::launch_cbam_apply(ap, stream);
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, ys, n, cy, height, width, cyp, f32(y_dev), stream);
    hipError_t ce = hipSuccess;         // the steps' own buffers, as the kernels left them
    if (!rc && partial_out) ce = hipMemcpyAsync(partial_out, part, part_bytes, hipMemcpyDeviceToDevice, stream);
    if (!rc && ce == hipSuccess && ca_out) ce = hipMemcpyAsync(ca_out, ca, ca_bytes, hipMemcpyDeviceToDevice, stream);
    if (!rc && ce == hipSuccess && maps_out) ce = hipMemcpyAsync(maps_out, maps, maps_bytes, hipMemcpyDeviceToDevice, stream);
    return m.finish(rc, ce, "copying a step's output");
}

int esahrnet_op_stem(const void* x_dev, int n, int height, int width, const float* w, const float* b, int relu, int pooled,
                     int precision, void* y_dev, void* partial_out, int* slabs_out, esahrnet_stream stream_) {
    if (!x_dev || !w || !b || !y_dev || n <= 0 || height <= 0 || width <= 0) return set_error("op_stem: bad argument");
    if (precision < 0 || precision > 2) return set_error("op_stem: precision %d (0, 1 or 2)", precision);
    if ((long long)height * width > 0x7fffffffLL / 64 / n) return set_error("op_stem: %d x %d x %d pixels", n, height, width);
    constexpr int cout = 64;            // padded alike in every format
    const int slabs = pooled ? esa::stem_pool_slabs(1, cout, height, width) : 0;
    if (pooled && (!partial_out || !slabs_out)) return set_error("op_stem: pooled = 1 needs partial_out and slabs_out");
    if (pooled && slabs <= 0) return set_error("op_stem: launch_stem_pool does not serve %d x %d", height, width);
    const Format f(precision);
    DevScope m("op_stem", static_cast<hipStream_t>(stream_));
    const std::vector<float> wp = esa::pack_stem_w(w, cout, 1, cout), bp(b, b + cout);      // [cout/8][1][9][8], esahrnet_commit's packing
    const float *dw = nullptr, *db = nullptr;
    char* ys = nullptr;
    float* part = nullptr;
    if (m.upload(wp, &dw) || m.upload(bp, &db)) return 1;
    const size_t part_bytes = (size_t)n * slabs * cout * 2 * sizeof(float);
    if (m.alloc(&ys, (size_t)n * height * width * cout * f.eb) || (pooled && m.alloc(&part, part_bytes))) return 1;
    esa::StemParams p{f32(x_dev), ys, dw, db, n, height, width, 1, cout, relu ? 1 : 0, f.fmt};
    int rc = pooled ? esa::launch_stem_pool(p, part, m.stream()) : esa::launch_stem(p, m.stream());
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, ys, n, cout, height, width, cout, f32(y_dev), m.stream());
    hipError_t ce = hipSuccess;
    if (!rc && pooled) ce = hipMemcpyAsync(partial_out, part, part_bytes, hipMemcpyDeviceToDevice, m.stream());
    if (m.finish(rc, ce, "copying the partials")) return 1;
    if (pooled) *slabs_out = slabs;
    return 0;
}

int esahrnet_op_resample(const void* x_dev, int n, int c, int h, int w, void* y_dev, int cy, int c0, int height, int width,
                         int align, int precision, esahrnet_stream stream_) {
    if (!x_dev || !y_dev || n <= 0 || c <= 0 || cy <= 0 || h <= 0 || w <= 0 || height <= 0 || width <= 0) return set_error("op_resample: bad argument");
    if (precision < 0 || precision > 2) return set_error("op_resample: precision %d (resample_slice serves 0, 1 and 2)", precision);
    const Format f(precision);
    const int cp = f.pad(c), cyp = f.pad(cy);
    const int cw = (c + 7) & ~7;        // the kernel writes whole 8-channel groups
    if (c0 < 0 || (c0 & 7)) return set_error("op_resample: c0=%d is not a multiple of 8", c0);
    if (c0 + cw > cyp) return set_error("op_resample: slice [%d, %d) outside the %d channels of y", c0, c0 + cw, cyp);
    DevScope m("op_resample", static_cast<hipStream_t>(stream_));
    char *xs = nullptr, *ys = nullptr;
    if (m.alloc(&xs, (size_t)n * h * w * cp * f.eb) || m.alloc(&ys, (size_t)n * height * width * cyp * f.eb)) return 1;
    int rc = esa::launch_nchw_to_fmt(f.fmt, f32(x_dev), n, c, h, w, xs, cp, m.stream());
    if (!rc) rc = esa::launch_nchw_to_fmt(f.fmt, f32(y_dev), n, cy, height, width, ys, cyp, m.stream());
    esa::ResampleParams p{};
    p.x = xs; p.y = ys; p.N = n; p.h = h; p.w = w; p.H = height; p.W = width;
    p.C = c; p.Cp_src = cp; p.y_pix_bytes = cyp * f.eb; p.y_c0 = c0; p.align = align ? 1 : 0; p.fmt = f.fmt;
    if (!rc) rc = esa::launch_resample_slice(p, m.stream());
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, ys, n, cy, height, width, cyp, f32(y_dev), m.stream());
    return m.finish(rc);
}

int esahrnet_op_zero_slice(void* y_dev, int n, int cy, int height, int width, int c0, int nchan, int precision,
                           esahrnet_stream stream_) {
    if (!y_dev || n <= 0 || cy <= 0 || height <= 0 || width <= 0) return set_error("op_zero_slice: bad argument");
    if (precision < 0 || precision > 2) return set_error("op_zero_slice: precision %d (zero_slice serves 0, 1 and 2)", precision);
    const Format f(precision);
    const int cyp = f.pad(cy);
    if (c0 < 0 || (c0 & 7) || nchan <= 0 || (nchan & 7)) return set_error("op_zero_slice: c0=%d, nchan=%d must be multiples of 8", c0, nchan);
    if (nchan > cyp - c0) return set_error("op_zero_slice: slice [%d, %d) outside the %d channels of y", c0, c0 + nchan, cyp);
    DevScope m("op_zero_slice", static_cast<hipStream_t>(stream_));
    char* ys = nullptr;
    const long long npix = (long long)n * height * width;
    if (m.alloc(&ys, (size_t)npix * cyp * f.eb)) return 1;
    int rc = esa::launch_nchw_to_fmt(f.fmt, f32(y_dev), n, cy, height, width, ys, cyp, m.stream());
    if (!rc) rc = esa::launch_zero_slice(ys, npix, cyp * f.eb, c0, nchan, m.stream(), f.fmt);
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, ys, n, cy, height, width, cyp, f32(y_dev), m.stream());
    return m.finish(rc);
}

// ---- every convolution launcher on its own (tests/test_gpu_conv.py) --------------------------------------------------
int esahrnet_op_conv_kernel(int n, int cin, int cout, int height, int width, int k, int stride, int has_res, int precision,
                            char* out, size_t cap) {
    if (!out || cap == 0) return set_error("op_conv_kernel: null argument");
    if (precision < 0 || precision > 3) return set_error("op_conv_kernel: precision %d", precision);
    if (!op_conv_dims_ok(n, cin, cout, height, width, k, stride))
        return set_error("op_conv_kernel: n=%d cin=%d cout=%d %dx%d k=%d stride=%d unsupported", n, cin, cout, height, width, k, stride);
    static const char some_residual = 0;
    const esa::ConvParams p = op_conv_shape(Format(precision), n, cin, cout, height, width, stride, 0, has_res ? &some_residual : nullptr);
    snprintf(out, cap, "%s", esa::conv_kernel_name(p, k, stride));
    return 0;
}

int esahrnet_op_conv_group(int count, const void* const* xs_dev, const int* ns, const int* cins, const int* heights, const int* widths,
                           const float* const* ws, const float* const* bs, const int* couts, int k, int stride, const int* relus,
                           const void* const* res_dev, void* const* ys_dev, int precision, char* kernel_out, size_t kernel_cap,
                           esahrnet_stream stream_) {
    const char* who = "op_conv_group";
    if (!xs_dev || !ns || !cins || !heights || !widths || !ws || !bs || !couts || !relus || !ys_dev) return set_error("%s: null argument", who);
    if (count < 1 || count > 6) return set_error("%s: count=%d (1 .. 6)", who, count);
    if (precision < 0 || precision > 3) return set_error("%s: precision %d", who, precision);
    const Format f(precision);
    esa::ConvParams ps[6];
    for (int j = 0; j < count; ++j) {
        if (!xs_dev[j] || !ws[j] || !bs[j] || !ys_dev[j]) return set_error("%s: null argument (member %d)", who, j);
        if (!op_conv_dims_ok(ns[j], cins[j], couts[j], heights[j], widths[j], k, stride))
            return set_error("%s: member %d: n=%d cin=%d cout=%d %dx%d k=%d stride=%d unsupported", who, j, ns[j], cins[j], couts[j],
                             heights[j], widths[j], k, stride);
        ps[j] = op_conv_shape(f, ns[j], cins[j], couts[j], heights[j], widths[j], stride, relus[j], res_dev ? res_dev[j] : nullptr);
    }
    char kernel[64];
    if (count == 1) {
        snprintf(kernel, sizeof kernel, "%s", esa::conv_kernel_name(ps[0], k, stride));
        if (!strcmp(kernel, "none")) return set_error("%s: no kernel of precision %d serves this convolution", who, precision);
    } else {
        if (!esa::conv_group_mergeable(f.fmt, ps, count, k, stride))
            return set_error("%s: these %d convolutions (k=%d, stride=%d, precision %d) have no merged launch", who, count, k, stride, precision);
        esa::conv_group_kernel_name(kernel, sizeof kernel, f.fmt, ps, count, k, stride);
    }
    DevScope m(who, static_cast<hipStream_t>(stream_));
    for (int j = 0; j < count; ++j) {
        int rc = 0;
        if (op_conv_device(m, f, ps[j], cins[j], couts[j], k, ws[j], bs[j], xs_dev[j], res_dev ? res_dev[j] : nullptr, &rc)) return 1;
        if (rc) return set_error("%s: layout conversion failed: %s", who, hipGetErrorString((hipError_t)rc));
    }
    int rc = count == 1 ? esa::launch_conv(ps[0], k, stride, m.stream())
           : f.x6 ? esa::launch_conv_x6_jobs(ps, count, k, stride, m.stream())
           : k == 1 ? esa::launch_conv1x1_jobs(ps, count, m.stream()) : esa::launch_conv_jobs(ps, count, stride, m.stream());
    for (int j = 0; j < count && !rc; ++j)      // all C' channels: the padding comes back too
        rc = esa::launch_fmt_to_nchw(f.fmt, ps[j].y, ps[j].N, ps[j].Coutp, ps[j].OH, ps[j].OW, ps[j].Coutp, f32(ys_dev[j]), m.stream());
    if (m.finish(rc)) return 1;
    if (kernel_out && kernel_cap) snprintf(kernel_out, kernel_cap, "%s", kernel);
    return 0;
}

int esahrnet_op_conv_multi(const void* x_dev, int n, int cin, int height, int width, int nheads, const float* const* ws,
                           const float* const* bs, const int* couts, const int* relus, void* const* ys_dev, esahrnet_stream stream_) {
    const char* who = "op_conv_multi";
    const Format f(0);
    if (!x_dev || !ws || !bs || !couts || !relus || !ys_dev) return set_error("%s: null argument", who);
    if (nheads < 2 || nheads > 3) return set_error("%s: nheads=%d (2 or 3)", who, nheads);
    int total = 0;
    for (int h = 0; h < nheads; ++h) {
        if (!ws[h] || !bs[h] || !ys_dev[h]) return set_error("%s: null argument (head %d)", who, h);
        if (couts[h] <= 0 || (couts[h] & 31)) return set_error("%s: head %d has %d couts (a positive multiple of 32)", who, h, couts[h]);
        total += couts[h];
    }
    if (!op_conv_dims_ok(n, cin, total, height, width, 3, 2)) return set_error("%s: n=%d cin=%d couts=%d %dx%d unsupported", who, n, cin, total, height, width);
    esa::ConvParams p = op_conv_shape(f, n, cin, total, height, width, 2, 0, nullptr);
    p.nheads = nheads;
    std::vector<char> packed;
    std::vector<float> bias;
    for (int h = 0; h < nheads; ++h) {          // members' packed weights / biases back to back, as esahrnet_commit lays them
        const std::vector<char> wh = f.pack(ws[h], couts[h], cin, 3, couts[h], p.Cinp);
        packed.insert(packed.end(), wh.begin(), wh.end());
        bias.insert(bias.end(), bs[h], bs[h] + couts[h]);
        p.hb[h + 1] = p.hb[h] + couts[h];
        p.hrelu[h] = relus[h] ? 1 : 0;
    }
    DevScope m(who, static_cast<hipStream_t>(stream_));
    char* xs = nullptr;
    if (m.upload(packed, &p.w) || m.upload(bias, &p.bias) || m.alloc(&xs, (size_t)n * height * width * p.Cinp * 4)) return 1;
    for (int h = 0; h < nheads; ++h)
        if (m.alloc(&p.yh[h], (size_t)n * p.OH * p.OW * couts[h] * 4)) return 1;
    p.x = xs;
    if (!esa::conv_s2c32_multi_supported(p)) return set_error("%s: launch_conv_s2c32_multi does not serve these heads", who);
    int rc = esa::launch_nchw_to_fmt(f.fmt, f32(x_dev), n, cin, height, width, xs, p.Cinp, m.stream());
    if (!rc) rc = esa::launch_conv_s2c32_multi(p, m.stream());
    for (int h = 0; h < nheads && !rc; ++h)
        rc = esa::launch_fmt_to_nchw(f.fmt, p.yh[h], n, couts[h], p.OH, p.OW, couts[h], f32(ys_dev[h]), m.stream());
    return m.finish(rc);
}

int esahrnet_op_block32(const void* x_dev, int n, int height, int width, const float* w1, const float* b1, const float* w2,
                        const float* b2, void* y_dev, esahrnet_stream stream_) {
    const char* who = "op_block32";
    const Format f(0);
    if (!x_dev || !w1 || !b1 || !w2 || !b2 || !y_dev) return set_error("%s: null argument", who);
    if (!op_conv_dims_ok(n, 32, 32, height, width, 3, 1)) return set_error("%s: n=%d %dx%d unsupported", who, n, height, width);
    DevScope m(who, static_cast<hipStream_t>(stream_));
    const std::vector<float> hb1(b1, b1 + 32), hb2(b2, b2 + 32);
    esa::BlockParams p{};
    p.N = n; p.H = height; p.W = width;
    char* xs = nullptr;
    if (m.upload(f.pack(w1, 32, 32, 3, 32, 32), &p.w1) || m.upload(f.pack(w2, 32, 32, 3, 32, 32), &p.w2) || m.upload(hb1, &p.bias1) ||
        m.upload(hb2, &p.bias2)) return 1;
    const size_t bytes = (size_t)n * height * width * 128;
    if (m.alloc(&xs, bytes) || m.alloc(&p.y, bytes)) return 1;
    p.x = xs;
    int rc = esa::launch_nchw_to_fmt(f.fmt, f32(x_dev), n, 32, height, width, xs, 32, m.stream());
    if (!rc) rc = esa::launch_bblock32(p, m.stream());
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, p.y, n, 32, height, width, 32, f32(y_dev), m.stream());
    return m.finish(rc);
}

int esahrnet_op_stem2(const void* x_dev, int n, int cin, int height, int width, const float* w1, const float* b1, int cmid,
                      const float* w2, const float* b2, int cout, int precision, void* y_dev, esahrnet_stream stream_) {
    const char* who = "op_stem2";
    if (!x_dev || !w1 || !b1 || !w2 || !b2 || !y_dev) return set_error("%s: null argument", who);
    if (precision != 0 && precision != 2) return set_error("%s: precision %d (0: stem_fused, 2: stem_x6_kernel)", who, precision);
    const Format f(precision);
    if (cin < 1 || cin > 4) return set_error("%s: cin=%d (1 .. 4)", who, cin);
    if (cmid <= 0 || (cmid & 31)) return set_error("%s: cmid=%d (a positive multiple of 32)", who, cmid);
    if (!op_conv_dims_ok(n, cmid, cout, height, width, 3, 2)) return set_error("%s: n=%d cmid=%d cout=%d %dx%d unsupported", who, n, cmid, cout, height, width);
    const int coutp = f.pad(cout), oh = (height + 1) / 2, ow = (width + 1) / 2;
    if (f.x6 && !esa::stem_fused_x6_supported(cin, cmid, coutp)) return set_error("%s: stem_x6_kernel does not serve cin=%d cmid=%d cout=%d", who, cin, cmid, cout);
    std::vector<float> w1p, b1p(b1, b1 + cmid), b2p(coutp, 0.f);
    std::copy(b2, b2 + cout, b2p.begin());
    if (f.x6) {                                 // conv1 in stem_x6_kernel's layout (bias inside), as esahrnet_commit packs it
        w1p.assign(2 * 4 * 10 * 8, 0.f);
        esa::pack_stem_w1_x6(w1, b1, w1p.data());
    } else {                                    // [cmid/8][cin][9][8]
        w1p = esa::pack_stem_w(w1, cmid, cin, cmid);
    }
    DevScope m(who, static_cast<hipStream_t>(stream_));
    esa::StemFusedParams p{};
    p.x = f32(x_dev);
    p.N = n; p.H = height; p.W = width; p.OH = oh; p.OW = ow; p.cin = cin; p.Cmid = cmid; p.Coutp = coutp;
    if (m.upload(w1p, &p.w1) || m.upload(b1p, &p.bias1) || m.upload(f.pack(w2, cout, cmid, 3, coutp, cmid), &p.w2) || m.upload(b2p, &p.bias2)) return 1;
    if (m.alloc(&p.y, (size_t)n * oh * ow * coutp * 4)) return 1;
    int rc = f.x6 ? esa::launch_stem_fused_x6(p, m.stream()) : esa::launch_stem_fused(p, m.stream());
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, p.y, n, coutp, oh, ow, coutp, f32(y_dev), m.stream());
    return m.finish(rc);
}

// ---- the stem outside esahrnet_op_stem's one configuration, the layout conversions and the tile-maximum kernels on their own
// (tests/test_gpu_layout.py) ---------------------------------------------------------------------------------------------------
int esahrnet_op_stem_ex(const void* x_dev, int n, int cin, int height, int width, const float* w, const float* b, int cout,
                        int relu, int precision, void* y_dev, esahrnet_stream stream_) {
    const char* who = "op_stem_ex";
    if (!x_dev || !w || !b || !y_dev) return set_error("%s: null argument", who);
    if (precision < 0 || precision > 3) return set_error("%s: precision %d (0 .. 3)", who, precision);
    const Format f(precision);
    if (cin < 1 || cin > 4) return set_error("%s: cin=%d (1 .. 4)", who, cin);
    if (cout <= 0 || (cout & 31)) return set_error("%s: cout=%d (a positive multiple of 32)", who, cout);
    if (f.half && (cout & 63)) return set_error("%s: cout=%d (the 16-bit formats hold blocks of 64 channels)", who, cout);
    if (n <= 0 || height <= 0 || width <= 0 || (long long)n * height * width * cout * 4 > 0x7fffffffLL)
        return set_error("%s: n=%d %dx%d cout=%d unsupported", who, n, height, width, cout);
    DevScope m(who, static_cast<hipStream_t>(stream_));
    const std::vector<float> wp = esa::pack_stem_w(w, cout, cin, cout), bp(b, b + cout);     // esahrnet_commit's packing of conv1
    const float *dw = nullptr, *db = nullptr;
    char* ys = nullptr;
    if (m.upload(wp, &dw) || m.upload(bp, &db) || m.alloc(&ys, (size_t)n * height * width * cout * f.eb)) return 1;
    esa::StemParams p{f32(x_dev), ys, dw, db, n, height, width, cin, cout, relu ? 1 : 0, f.fmt};
    int rc = esa::launch_stem(p, m.stream());
    if (!rc) rc = esa::launch_fmt_to_nchw(f.fmt, ys, n, cout, height, width, cout, f32(y_dev), m.stream());
    return m.finish(rc);
}

int esahrnet_op_layout(int dir, const void* x_dev, int n, int c, int height, int width, int cp, int precision, void* raw_dev,
                       void* y_dev, esahrnet_stream stream_) {
    const char* who = "op_layout";
    if (dir != 0 && dir != 1) return set_error("%s: dir=%d (0: f32 NCHW -> raw -> f32 NCHW, 1: raw -> f32 NCHW)", who, dir);
    if (!raw_dev || !y_dev || (dir == 0 && !x_dev)) return set_error("%s: null argument", who);
    if (precision < 0 || precision > 3) return set_error("%s: precision %d (0 .. 3)", who, precision);
    if (n <= 0 || c <= 0 || height <= 0 || width <= 0) return set_error("%s: n=%d c=%d %dx%d unsupported", who, n, c, height, width);
    if (cp < c || (cp & 7)) return set_error("%s: cp=%d (a multiple of 8, at least c=%d)", who, cp, c);
    if ((long long)n * height * width * cp * 4 > 0x7fffffffLL) return set_error("%s: n=%d cp=%d %dx%d unsupported", who, n, cp, height, width);
    if (!aligned(raw_dev, 16) || !aligned(y_dev, 4) || !aligned(x_dev, 4))
        return set_error("%s: raw_dev must be 16-byte aligned, x_dev and y_dev 4-byte aligned", who);
    const int fmt = Format(precision).fmt;
    DevScope m(who, static_cast<hipStream_t>(stream_));         // (the caller's buffers only)
    int rc = 0;
    if (dir == 0) rc = esa::launch_nchw_to_fmt(fmt, f32(x_dev), n, c, height, width, static_cast<char*>(raw_dev), cp, m.stream());
    if (!rc) rc = esa::launch_fmt_to_nchw(fmt, static_cast<const char*>(raw_dev), n, c, height, width, cp, f32(y_dev), m.stream());
    return m.finish(rc);
}

int esahrnet_op_tile_max(const void* raw_dev, int n, int c, int height, int width, int cp, int precision, int store, void* y_dev,
                         void* part_dev, int* ntiles_out, void* kp_dev, void* idx_dev, esahrnet_stream stream_) {
    const char* who = "op_tile_max";
    if (!raw_dev || !part_dev || !ntiles_out) return set_error("%s: null argument", who);
    if (precision != 0 && precision != 2) return set_error("%s: precision %d (0: split-bf16, 2: f32)", who, precision);
    if (store != 0 && store != 1) return set_error("%s: store=%d (0 or 1)", who, store);
    if (store && !y_dev) return set_error("%s: store = 1 needs y_dev", who);
    if (n <= 0 || height <= 0 || width <= 0) return set_error("%s: n=%d %dx%d unsupported", who, n, height, width);
    if (c < 1 || c > 32) return set_error("%s: c=%d (1 .. 32)", who, c);
    if (cp < c || (cp & 7)) return set_error("%s: cp=%d (a multiple of 8, at least c=%d)", who, cp, c);
    if ((long long)n * height * width * cp * 4 > 0x7fffffffLL) return set_error("%s: n=%d cp=%d %dx%d unsupported", who, n, cp, height, width);
    if (!aligned(raw_dev, 16) || !aligned(part_dev, 8) || !aligned(y_dev, 4) || !aligned(kp_dev, 4) || !aligned(idx_dev, 4))
        return set_error("%s: raw_dev must be 16-byte aligned, part_dev 8-byte, y_dev, kp_dev and idx_dev 4-byte", who);
    const int fmt = Format(precision).fmt, ntiles = esa::to_nchw_part_tiles(height, width);
    DevScope m(who, static_cast<hipStream_t>(stream_));         // (the caller's buffers only)
    const char* raw = static_cast<const char*>(raw_dev);
    float2* part = static_cast<float2*>(part_dev);
    int rc = store ? esa::launch_to_nchw_part(fmt, raw, n, c, height, width, cp, f32(y_dev), part, m.stream())
                   : esa::launch_tile_max(fmt, raw, n, c, height, width, cp, part, m.stream());
    if (!rc && kp_dev)
        rc = esa::launch_keypoints_finish_nhwc(fmt, raw, n, c, height, width, cp, part, ntiles, f32(kp_dev), static_cast<int*>(idx_dev), m.stream());
    if (m.finish(rc)) return 1;
    *ntiles_out = ntiles;
    return 0;
}

}  // extern "C"
