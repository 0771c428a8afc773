// report.hip — the handle entries of the two reports over a forward's tensors: the activation range report (kernels: stats.hip)
// and the precision report of one handle against another (diff.hip), with their stand-alone tensor entries.
#include "plan.h"

using namespace esa;

extern "C" {

// Both reports read every tensor after the forward, so they plan and run with esahrnet_set_debug_keep's mode forced on one handle
// or two; leaving the scope puts back what the handles had.
struct KeepScope {
    esahrnet_ctx *a, *b;
    const bool ka, kb;
    explicit KeepScope(esahrnet_ctx* h, esahrnet_ctx* href = nullptr) : a(h), b(href ? href : h), ka(a->keep), kb(b->keep) { a->keep = b->keep = true; }
    ~KeepScope() { a->keep = ka; b->keep = kb; }
};

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
    if (!h || !rows) return set_error("stats_rows: null argument");
    *rows = (int)h->tensors.size() + 1;
    return 0;
}

int esahrnet_stats_row_get(esahrnet_handle h, int row, int n, int height, int width, esahrnet_stats_row_desc* out) {
    if (!h || !out) return set_error("stats_row_get: null argument");
    const int nt = (int)h->tensors.size();
    if (row < 0 || row > nt) return set_error("stats_row_get: row %d out of range (0..%d)", row, nt);
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

// the keep-mode plan of the shape (the caller holds a KeepScope), then the partials behind it
static int stats_plan(const char* who, esahrnet_ctx& c, int n, int height, int width, size_t* bytes) {
    if (plan_shape(c, n, height, width)) return 1;
    const long long parts = stats_partials_per_image(c, c.sp);
    if (parts < 0) return set_error("%s: crop %dx%d is beyond the scan of the heat-maps", who, height, width);
    *bytes = pad256(pad256(c.sp.bytes) + (size_t)parts * n * sizeof(esahrnet_stats_record));
    return 0;
}

int esahrnet_forward_stats_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    if (!h || !bytes) return set_error("forward_stats_workspace_bytes: null argument");
    const KeepScope keep(h);
    return stats_plan("forward_stats_workspace_bytes", *h, n, height, width, bytes);
}

// the partials of the fused head's range form behind the scan's (esahrnet_forward_stats_h0); 0 where that head does not run
static size_t stats_h0_bytes(const esahrnet_ctx& c, const ShapePlan& sp) {
    if (c.head2_op < 0 || c.ops[c.head2_op].kind != OP_HEADBF || c.x6() || !sp.head2) return 0;
    const Tensor& t0 = c.tensors[c.ops[c.head2_op].in];
    return pad256((size_t)esa::head_bf_range_tiles(sp.lh[t0.level], sp.lw[t0.level]) * sp.n * 8);
}

// esahrnet_forward_stats (h0_dev == nullptr, with_h0 false) and esahrnet_forward_stats_h0
static int forward_stats(const char* who, bool with_h0, esahrnet_handle h, const void* x_dev, int n, int height, int width,
                         void* heat_dev, void* ws_dev, size_t ws_bytes, void* stats_dev, void* h0_dev, esahrnet_stream stream_) {
    if (!h || !x_dev || !heat_dev || !ws_dev || !stats_dev || (with_h0 && !h0_dev)) return set_error("%s: null argument", who);
    if (!h->committed) return set_error("%s: esahrnet_commit has not been called", who);
    if (with_h0 && h->gnames.empty()) return set_error("%s: variant 0 with precision 1 or 3 only (the head that rounds h0 in registers)", who);
    if (with_h0 && h->opt.bf_head_valu && !h->hf()) return set_error("%s: the range form is the matrix-core head's: unset ESAHRNET_BF_HEAD_VALU", who);
    const KeepScope keep(h);
    size_t need = 0;
    if (stats_plan(who, *h, n, height, width, &need)) return 1;
    const size_t h0_off = need, h0_bytes = with_h0 ? stats_h0_bytes(*h, h->sp) : 0;
    need += h0_bytes;
    if (check_workspace(who, ws_dev, ws_bytes, need)) return 1;
    if (reinterpret_cast<uintptr_t>(stats_dev) & 7) return set_error("%s: stats_dev must be 8-byte aligned", who);
    if (with_h0 && (reinterpret_cast<uintptr_t>(h0_dev) & 7)) return set_error("%s: h0_dev must be 8-byte aligned", who);
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
    const int rc = esa::launch_stats(jobs.data(), (int)jobs.size(), n, ws + pad256(sp.bytes), stats_dev, stream);
    if (rc) return set_error("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    if (with_h0 && !h0_bytes) {     // the materialised head ran: h0 is the stored row "head0"
        int row = -1;
        for (size_t ti = 0; ti < h->tensors.size(); ++ti)
            if (h->tensors[ti].tap == "head0" && stats_scanned(*h, sp, h->tensors[ti])) row = (int)ti;
        if (row < 0) return set_error("%s: no head0 tensor at this shape", who);
        HIP_OK(hipMemcpyAsync(h0_dev, static_cast<const esahrnet_stats_record*>(stats_dev) + (size_t)row * n,
                              (size_t)n * sizeof(esahrnet_stats_record), hipMemcpyDeviceToDevice, stream));
    }
    return 0;
}

int esahrnet_forward_stats(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* ws_dev,
                           size_t ws_bytes, void* stats_dev, esahrnet_stream stream) {
    return forward_stats("forward_stats", false, h, x_dev, n, height, width, heat_dev, ws_dev, ws_bytes, stats_dev, nullptr, stream);
}

int esahrnet_forward_stats_h0_workspace_bytes(esahrnet_handle h, int n, int height, int width, size_t* bytes) {
    if (!h || !bytes) return set_error("forward_stats_h0_workspace_bytes: null argument");
    const KeepScope keep(h);
    if (stats_plan("forward_stats_h0_workspace_bytes", *h, n, height, width, bytes)) return 1;
    *bytes += stats_h0_bytes(*h, h->sp);
    return 0;
}

int esahrnet_forward_stats_h0(esahrnet_handle h, const void* x_dev, int n, int height, int width, void* heat_dev, void* ws_dev,
                              size_t ws_bytes, void* stats_dev, void* h0_dev, esahrnet_stream stream) {
    return forward_stats("forward_stats_h0", true, h, x_dev, n, height, width, heat_dev, ws_dev, ws_bytes, stats_dev, h0_dev, stream);
}

static int tensor_stats_parts(const char* who, int fmt, int n, int c, int cp, int h, int w, int* parts) {
    if (n < 1) return set_error("%s: batch must be positive (got %d)", who, n);
    const long long hw = (long long)h * w;
    *parts = h > 0 && w > 0 && hw <= 0x7fffffffLL && fmt >= esa::STATS_NCHW && fmt <= esa::FMT_HF
                 ? esa::stats_parts(fmt, c, cp, (int)hw) : 0;
    if (*parts <= 0)
        return set_error("%s: no scan for format %d, %d channels (%d padded), %dx%d (formats -1..3; SB: padded channels a multiple "
                         "of 8, BF / HF of 8, F32 of 4; an image below 2 GiB)", who, fmt, c, cp, h, w);
    return 0;
}

int esahrnet_tensor_stats_workspace_bytes(int fmt, int n, int c, int cp, int h, int w, size_t* bytes) {
    if (!bytes) return set_error("tensor_stats_workspace_bytes: null argument");
    int parts = 0;
    if (tensor_stats_parts("tensor_stats_workspace_bytes", fmt, n, c, cp, h, w, &parts)) return 1;
    *bytes = (size_t)parts * n * sizeof(esahrnet_stats_record);
    return 0;
}

int esahrnet_tensor_stats(const void* t_dev, int fmt, int n, int c, int cp, int h, int w, void* ws_dev, size_t ws_bytes,
                          void* stats_dev, esahrnet_stream stream) {
    if (!t_dev || !ws_dev || !stats_dev) return set_error("tensor_stats: null argument");
    int parts = 0;
    if (tensor_stats_parts("tensor_stats", fmt, n, c, cp, h, w, &parts)) return 1;
    const size_t need = (size_t)parts * n * sizeof(esahrnet_stats_record);
    if (ws_bytes < need) return set_error("tensor_stats: workspace too small (%zu < %zu)", ws_bytes, need);
    if (fmt != esa::STATS_NCHW && (reinterpret_cast<uintptr_t>(t_dev) & 15)) return set_error("tensor_stats: t_dev must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(ws_dev) & 7) return set_error("tensor_stats: workspace must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(stats_dev) & 7) return set_error("tensor_stats: stats_dev must be 8-byte aligned");
    const esa::StatsJob job{t_dev, fmt, c, cp, h * w, 0};
    const int rc = esa::launch_stats(&job, 1, n, ws_dev, stats_dev, static_cast<hipStream_t>(stream));
    if (rc) return set_error("tensor_stats: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
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
    if (!h || !href || !out) return set_error("diff_row_get: null argument");
    const int nt = (int)h->tensors.size();
    if (row < 0 || row > nt) return set_error("diff_row_get: row %d out of range (0..%d)", row, nt);
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

// both keep-mode plans of the shape (the caller holds a KeepScope on both handles), the rows, the workspace
static int diff_plan(const char* who, esahrnet_ctx& a, esahrnet_ctx& b, int n, int height, int width, DiffPlan* dp) {
    int va = 0, vb = 0;
    if (const char* f = diff_cfg_field(a.cfg, b.cfg, &va, &vb))
        return set_error("%s: the handles differ in %s (%d against %d): they may differ in precision only", who, f, va, vb);
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
    if (!dp->rows[rows - 1].compared) return set_error("%s: crop %dx%d is beyond the scan of the heat-maps", who, height, width);
    dp->off_b = pad256(a.sp.bytes);
    dp->off_parts = dp->off_b + pad256(b.sp.bytes);
    dp->bytes = pad256(dp->off_parts + (size_t)parts * n * sizeof(esahrnet_diff_record));
    return 0;
}

int esahrnet_forward_diff_workspace_bytes(esahrnet_handle h, esahrnet_handle href, int n, int height, int width, size_t* bytes) {
    if (!h || !href || !bytes) return set_error("forward_diff_workspace_bytes: null argument");
    const KeepScope keep(h, href);
    DiffPlan dp;
    if (diff_plan("forward_diff_workspace_bytes", *h, *href, n, height, width, &dp)) return 1;
    *bytes = dp.bytes;
    return 0;
}

int esahrnet_forward_diff(esahrnet_handle h, esahrnet_handle href, const void* x_dev, int n, int height, int width,
                          void* heat_dev, void* heat_ref_dev, void* ws_dev, size_t ws_bytes, void* diff_dev, esahrnet_stream stream_) {
    const char* who = "forward_diff";
    if (!h || !href || !x_dev || !heat_dev || !heat_ref_dev || !ws_dev || !diff_dev) return set_error("%s: null argument", who);
    if (!h->committed || !href->committed)
        return set_error("%s: esahrnet_commit has not been called on the %s handle", who, !h->committed ? "tested" : "reference");
    if (h->device != href->device) return set_error("%s: the handles live on different devices (%d and %d)", who, h->device, href->device);
    const KeepScope keep(h, href);
    DiffPlan dp;
    if (diff_plan(who, *h, *href, n, height, width, &dp)) return 1;
    if (check_workspace(who, ws_dev, ws_bytes, dp.bytes)) return 1;
    if (reinterpret_cast<uintptr_t>(diff_dev) & 7) return set_error("%s: diff_dev must be 8-byte aligned", who);
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
    if (rc) return set_error("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    return 0;
}

static int tensor_diff_parts(const char* who, int fmt_a, int cp_a, int fmt_b, int cp_b, int exponent, int n, int c, int h, int w,
                             int* parts) {
    if (n < 1) return set_error("%s: batch must be positive (got %d)", who, n);
    if (exponent < -ESAHRNET_SCALE_MAX_EXPONENT || exponent > ESAHRNET_SCALE_MAX_EXPONENT)
        return set_error("%s: exponent %d outside -%d..%d", who, exponent, ESAHRNET_SCALE_MAX_EXPONENT, ESAHRNET_SCALE_MAX_EXPONENT);
    const bool nchw = fmt_a == esa::STATS_NCHW && fmt_b == esa::STATS_NCHW;
    if (!nchw && (fmt_a < esa::FMT_SB || fmt_a > esa::FMT_HF || fmt_b != esa::FMT_F32))
        return set_error("%s: no scan for format %d against format %d (0..3 against 2, or -1 against -1)", who, fmt_a, fmt_b);
    const long long hw = (long long)h * w;
    *parts = h > 0 && w > 0 && hw <= 0x7fffffffLL ? esa::diff_parts(fmt_a, cp_a, fmt_b, cp_b, c, (int)hw) : 0;
    if (*parts <= 0)
        return set_error("%s: no scan for %d channels (%d and %d padded), %dx%d (padded channels a multiple of 8 and at least the "
                         "channels; an image below 2 GiB on either side)", who, c, cp_a, cp_b, h, w);
    return 0;
}

int esahrnet_tensor_diff_workspace_bytes(int fmt_a, int cp_a, int fmt_b, int cp_b, int n, int c, int h, int w, size_t* bytes) {
    if (!bytes) return set_error("tensor_diff_workspace_bytes: null argument");
    int parts = 0;
    if (tensor_diff_parts("tensor_diff_workspace_bytes", fmt_a, cp_a, fmt_b, cp_b, 0, n, c, h, w, &parts)) return 1;
    *bytes = (size_t)parts * n * sizeof(esahrnet_diff_record);
    return 0;
}

int esahrnet_tensor_diff(const void* a_dev, int fmt_a, int cp_a, const void* b_dev, int fmt_b, int cp_b, int exponent,
                         int n, int c, int h, int w, void* ws_dev, size_t ws_bytes, void* diff_dev, esahrnet_stream stream) {
    if (!a_dev || !b_dev || !ws_dev || !diff_dev) return set_error("tensor_diff: null argument");
    int parts = 0;
    if (tensor_diff_parts("tensor_diff", fmt_a, cp_a, fmt_b, cp_b, exponent, n, c, h, w, &parts)) return 1;
    const size_t need = (size_t)parts * n * sizeof(esahrnet_diff_record);
    if (ws_bytes < need) return set_error("tensor_diff: workspace too small (%zu < %zu)", ws_bytes, need);
    if (fmt_a != esa::STATS_NCHW && ((reinterpret_cast<uintptr_t>(a_dev) | reinterpret_cast<uintptr_t>(b_dev)) & 15))
        return set_error("tensor_diff: a_dev and b_dev must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(a_dev) | reinterpret_cast<uintptr_t>(b_dev)) & 3)
        return set_error("tensor_diff: a_dev and b_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(ws_dev) & 7) return set_error("tensor_diff: workspace must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(diff_dev) & 7) return set_error("tensor_diff: diff_dev must be 8-byte aligned");
    const esa::DiffJob job{a_dev, fmt_a, cp_a, b_dev, fmt_b, cp_b, c, h * w, exponent, 0};
    const int rc = esa::launch_diff(&job, 1, n, ws_dev, diff_dev, static_cast<hipStream_t>(stream));
    if (rc) return set_error("tensor_diff: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

}  // extern "C"
