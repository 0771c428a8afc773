// diff.hip — the precision report: one record of esahrnet_diff_record (include/esahrnet.h) per (tensor, image), scanned from
// the SAME tensor of two forwards where they left it: A in the tested format, B in the fp32-grade format (plain f32 NHWC).
// The shape of stats.hip, with a second operand:
//   scan    a workgroup owns a fixed range of pixels of ONE image and leaves one partial record.  The two sides pad their
//           channels differently, so a lane owns one GROUP of 8 channels of a pixel on both sides: one 16-byte chunk of a
//           bf16 / fp16 tensor, the hi and the lo chunk of a split-bf16 tensor (joined as join8 joins them: the bits
//           esahrnet_tap_read returns), two chunks of an f32 tensor.  Groups without a real channel are never read; the padding
//           channels of the last group are loaded on both sides and masked, whatever they hold.  A lane keeps its group from
//           iteration to iteration, so its count of real channels is computed once, outside the pixel loop.
//   finish  one wave per (tensor, image) merges that image's partials: maxima, `at` and counts exactly, the sums in index order.
// No atomics; neither the number of partials of an image nor any offset inside an image depends on the batch (a 64-bit base
// per image, 32-bit offsets inside), so an image's record has the same bits alone, in a batch and in a permuted batch.
// Per element: d = a - b in f32 (one rounding), err = |d|; the three sums are carried in f64 per element (err^2 and b^2 are exact
// in f64: one v_fma_f64 each), which is what bounds the scan — it is VALU-bound, not read-bound.
#include <cstddef>
#include <vector>

#include "../../include/esahrnet.h"
#include "kernels.h"
#include "sb.h"

namespace esa {
namespace {

typedef esahrnet_diff_record Rec;
static_assert(sizeof(Rec) == ESAHRNET_DIFF_RECORD_BYTES, "the record is 64 bytes");
static_assert(offsetof(Rec, sum_abs_err) == 0 && offsetof(Rec, sum_sq_ref) == 16 && offsetof(Rec, max_abs_err) == 24 &&
              offsetof(Rec, at) == 36 && offsetof(Rec, n_class_differs) == 52 && offsetof(Rec, reserved) == 56,
              "the record has no holes");

constexpr int NT = 256;                     // threads of a scan workgroup
constexpr int WG_BYTES = 32768;             // bytes of B a scan workgroup owns (about: whole pixels)
constexpr int MAXJOBS = 16;                 // tensor pairs per launch (the job table travels as a kernel argument)
constexpr unsigned NONE = 0xFFFFFFFFu;

struct Job {
    const char* a;
    const char* b;
    unsigned long long img_a, img_b;        // one image of either tensor
    int pix_a, pix_b;                       // bytes per pixel
    int G, GT, PT;                          // groups of 8 channels with a real channel; a workgroup's lanes cover GT groups of PT pixels
    int HW, C, ppw, parts;                  // pixels (NCHW: elements) per image and per workgroup; partials per image
    int e;                                  // A enters as ldexpf(a, e)
    unsigned block0, part0;                 // first workgroup of the job in the launch; first partial in the workspace
    int row;
};
struct Jobs {
    int n, N;
    Rec* partials;                          // the workspace: the jobs' partials, Job::part0 onwards, image-major
    Rec* records;                           // [rows][N]
    Job job[MAXJOBS];
};

// what a lane has seen.  m < 0: nothing compared yet (any compared element, err >= 0, takes its place)
struct Acc {
    double s1, s2, sr;
    float m, mref, mtest;
    unsigned at, cmp, nfa, nfb, cls;
};
__device__ __forceinline__ Acc acc_init() { return Acc{0.0, 0.0, 0.0, -1.f, 0.f, 0.f, NONE, 0u, 0u, 0u, 0u}; }

// 0 finite, 1 NaN, 2 +inf, 3 -inf
__device__ __forceinline__ unsigned kind_of(float x) { return x != x ? 1u : x == INFINITY ? 2u : x == -INFINITY ? 3u : 0u; }

__device__ __forceinline__ void take(Acc& s, float a, float b, unsigned idx) {
    const unsigned ka = kind_of(a), kb = kind_of(b);
    const bool both = (ka | kb) == 0u;
    const float err = both ? fabsf(a - b) : -2.f;             // (finite operands: never NaN; +inf where the difference overflows)
    const float bz = both ? b : 0.f;
    const double e64 = both ? (double)err : 0.0, b64 = (double)bz;
    s.s1 += e64;
    s.s2 = fma(e64, e64, s.s2);
    s.sr = fma(b64, b64, s.sr);
    if (err > s.m || (err == s.m && idx < s.at)) { s.m = err; s.at = idx; }       // err = -2 never passes: m >= -1
    s.mref = fmaxf(s.mref, fabsf(bz));
    s.mtest = fmaxf(s.mtest, both ? fabsf(a) : 0.f);
    s.cmp += both ? 1u : 0u;
    s.nfa += ka ? 1u : 0u;
    s.nfb += kb ? 1u : 0u;
    s.cls += ka != kb ? 1u : 0u;
}

__device__ __forceinline__ void merge(Acc& a, const Acc& b) {
    a.s1 += b.s1; a.s2 += b.s2; a.sr += b.sr;
    if (b.m > a.m || (b.m == a.m && b.at < a.at)) { a.m = b.m; a.at = b.at; }
    a.mref = fmaxf(a.mref, b.mref); a.mtest = fmaxf(a.mtest, b.mtest);
    a.cmp += b.cmp; a.nfa += b.nfa; a.nfb += b.nfb; a.cls += b.cls;
}

__device__ __forceinline__ Acc shfl_acc(const Acc& a, int m) {
    Acc b;
    b.s1 = __shfl_xor(a.s1, m); b.s2 = __shfl_xor(a.s2, m); b.sr = __shfl_xor(a.sr, m);
    b.m = __shfl_xor(a.m, m); b.mref = __shfl_xor(a.mref, m); b.mtest = __shfl_xor(a.mtest, m);
    b.at = __shfl_xor(a.at, m); b.cmp = __shfl_xor(a.cmp, m); b.nfa = __shfl_xor(a.nfa, m);
    b.nfb = __shfl_xor(a.nfb, m); b.cls = __shfl_xor(a.cls, m);
    return b;
}

// the workgroup's partial record: lanes by an xor tree, then the waves in wave order (executed by all NT threads).  A partial
// keeps max_abs_err = -1 where nothing was compared; the finish turns that into 0.
__device__ __forceinline__ void write_partial(Acc a, Rec* out) {
    __shared__ Acc s[NT / 64];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const Acc b = shfl_acc(a, m);
        merge(a, b);
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < NT / 64; ++w) merge(a, s[w]);
    Rec r;
    r.sum_abs_err = a.s1; r.sum_sq_err = a.s2; r.sum_sq_ref = a.sr;
    r.max_abs_err = a.m; r.max_abs_ref = a.mref; r.max_abs_test = a.mtest;
    r.at = a.at; r.n_compared = a.cmp; r.n_nonfinite_test = a.nfa; r.n_nonfinite_ref = a.nfb; r.n_class_differs = a.cls;
    r.reserved[0] = r.reserved[1] = 0u;
    *out = r;
}

__device__ __forceinline__ Job find_job(const Jobs& js) {
    int j = 0;
    while (j + 1 < js.n && blockIdx.x >= js.job[j + 1].block0) ++j;
    return js.job[j];
}

__device__ __forceinline__ void f32x8_of(uint4 u, uint4 v, float f[8]) {
    f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y); f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
    f[4] = __uint_as_float(v.x); f[5] = __uint_as_float(v.y); f[6] = __uint_as_float(v.z); f[7] = __uint_as_float(v.w);
}

// FMT: the format of A (FMT_* codes); B is FMT_F32.  A group of 8 channels is 32 bytes in SB (hi chunk, lo chunk) and F32, 16
// bytes in BF and HF.
template <int FMT>
__global__ __launch_bounds__(NT) void diff_scan_kernel(Jobs js) {
    constexpr unsigned GA = FMT == FMT_SB || FMT == FMT_F32 ? 32u : 16u;
    const Job q = find_job(js);
    const unsigned local = blockIdx.x - q.block0;
    const unsigned img = local / (unsigned)q.parts, part = local - img * (unsigned)q.parts;
    const char* pa = q.a + (size_t)img * q.img_a;               // 64-bit per image, 32-bit inside it
    const char* pb = q.b + (size_t)img * q.img_b;
    const int p_begin = (int)part * q.ppw, p_end = min(p_begin + q.ppw, q.HW);
    const int tid = threadIdx.x;
    Acc acc = acc_init();
    if (tid < q.GT * q.PT) {
        const int g0 = tid % q.GT, p0 = tid / q.GT;
        for (int g = g0; g < q.G; g += q.GT) {                  // (one pass unless a pixel has more than NT groups)
            const int nreal = min(q.C - g * 8, 8);              // the lane's real channels: once, not per element
            const unsigned step_a = (unsigned)q.PT * (unsigned)q.pix_a, step_b = (unsigned)q.PT * (unsigned)q.pix_b;
            const unsigned step_i = (unsigned)q.PT * (unsigned)q.C;
            unsigned off_a = (unsigned)(p_begin + p0) * (unsigned)q.pix_a + (unsigned)g * GA;
            unsigned off_b = (unsigned)(p_begin + p0) * (unsigned)q.pix_b + (unsigned)g * 32u;
            unsigned idx = (unsigned)(p_begin + p0) * (unsigned)q.C + (unsigned)g * 8u;
#pragma unroll 2
            for (int p = p_begin + p0; p < p_end; p += q.PT, off_a += step_a, off_b += step_b, idx += step_i) {
                const uint4 a0 = *reinterpret_cast<const uint4*>(pa + off_a);
                const uint4 b0 = *reinterpret_cast<const uint4*>(pb + off_b);
                const uint4 b1 = *reinterpret_cast<const uint4*>(pb + off_b + 16);
                float fa[8], fb[8];
                if constexpr (FMT == FMT_SB) {
                    join8(a0, *reinterpret_cast<const uint4*>(pa + off_a + 16), fa);
                } else if constexpr (FMT == FMT_F32) {
                    f32x8_of(a0, *reinterpret_cast<const uint4*>(pa + off_a + 16), fa);
                } else if constexpr (FMT == FMT_HF) {
                    unpack8_f16(a0, fa);
                } else {
                    unpack8_bf16(a0, fa);
                }
                f32x8_of(b0, b1, fb);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < nreal) take(acc, ldexpf(fa[k], q.e), fb[k], idx + (unsigned)k);
            }
        }
    }
    write_partial(acc, js.partials + q.part0 + (size_t)img * (unsigned)q.parts + part);
}

// plain f32 [N][C][H][W] on both sides (the heat-maps, in caller memory): every element is real; a workgroup owns ppw
// consecutive elements of one image, a wave's lanes read consecutive dwords of either tensor
__global__ __launch_bounds__(NT) void diff_scan_nchw_kernel(Jobs js) {
    const Job q = find_job(js);
    const unsigned local = blockIdx.x - q.block0;
    const unsigned img = local / (unsigned)q.parts, part = local - img * (unsigned)q.parts;
    const float* pa = reinterpret_cast<const float*>(q.a + (size_t)img * q.img_a);
    const float* pb = reinterpret_cast<const float*>(q.b + (size_t)img * q.img_b);
    const int e_begin = (int)part * q.ppw, e_end = min(e_begin + q.ppw, q.HW);
    Acc acc = acc_init();
#pragma unroll 4
    for (int e = e_begin + (int)threadIdx.x; e < e_end; e += NT) take(acc, ldexpf(pa[e], q.e), pb[e], (unsigned)e);
    write_partial(acc, js.partials + q.part0 + (size_t)img * (unsigned)q.parts + part);
}

// one wave per (job, image): the image's partials into its record.  Maxima, `at` and counts are exact in any order; the three
// sums are added by lane 0 in index order.
__global__ __launch_bounds__(64) void diff_finish_kernel(Jobs js) {
    const Job q = js.job[blockIdx.x / (unsigned)js.N];
    const unsigned img = blockIdx.x % (unsigned)js.N;
    const Rec* p = js.partials + q.part0 + (size_t)img * (unsigned)q.parts;
    const int lane = threadIdx.x;
    Acc a = acc_init();
    for (int i = lane; i < q.parts; i += 64) {
        const Rec t = p[i];
        const Acc b{0.0, 0.0, 0.0, t.max_abs_err, t.max_abs_ref, t.max_abs_test, t.at, t.n_compared, t.n_nonfinite_test,
                    t.n_nonfinite_ref, t.n_class_differs};
        merge(a, b);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const Acc b = shfl_acc(a, m);
        merge(a, b);
    }
    if (lane != 0) return;
    Rec r;
    r.sum_abs_err = r.sum_sq_err = r.sum_sq_ref = 0.0;
    for (int i = 0; i < q.parts; ++i) { r.sum_abs_err += p[i].sum_abs_err; r.sum_sq_err += p[i].sum_sq_err; r.sum_sq_ref += p[i].sum_sq_ref; }
    r.max_abs_err = fmaxf(a.m, 0.f); r.max_abs_ref = a.mref; r.max_abs_test = a.mtest;
    r.at = a.at; r.n_compared = a.cmp; r.n_nonfinite_test = a.nfa; r.n_nonfinite_ref = a.nfb; r.n_class_differs = a.cls;
    r.reserved[0] = r.reserved[1] = 0u;
    js.records[(size_t)q.row * (unsigned)js.N + img] = r;
}

// the shape-only geometry of a job; false: a pair the scan does not serve
bool make_job(const DiffJob& s, Job* out) {
    Job q{};
    q.a = static_cast<const char*>(s.a); q.b = static_cast<const char*>(s.b); q.C = s.C; q.row = s.row; q.e = s.e;
    if (s.C < 1 || s.HW < 1 || s.e < -32 || s.e > 32) return false;
    if (s.fmt_a == STATS_NCHW || s.fmt_b == STATS_NCHW) {
        if (s.fmt_a != s.fmt_b) return false;
        const long long e = (long long)s.C * s.HW;
        if (e > 0x1fffffffLL) return false;                     // (32-bit byte offsets inside an image)
        q.HW = (int)e; q.img_a = q.img_b = (unsigned long long)e * 4; q.ppw = WG_BYTES / 4;
    } else {
        const bool half = fmt_half(s.fmt_a);
        if (s.fmt_b != FMT_F32 || (s.fmt_a != FMT_SB && s.fmt_a != FMT_F32 && !half)) return false;
        // whole groups of 8 channels on both sides: a lane's two chunks of an f32 pixel never leave the pixel
        if (s.C > s.cp_a || s.C > s.cp_b || s.cp_a % 8 || s.cp_b % 8) return false;
        const long long pix_a = (long long)s.cp_a * (half ? 2 : 4), pix_b = (long long)s.cp_b * 4;
        if (pix_a * s.HW > 0x7fffffffLL || pix_b * s.HW > 0x7fffffffLL || (long long)s.C * s.HW > 0xfffffffeLL) return false;
        q.pix_a = (int)pix_a; q.pix_b = (int)pix_b;
        q.img_a = (unsigned long long)(pix_a * s.HW); q.img_b = (unsigned long long)(pix_b * s.HW);
        q.G = (s.C + 7) / 8; q.GT = q.G < NT ? q.G : NT; q.PT = NT / q.GT;
        q.HW = s.HW;
        const int want = WG_BYTES / (q.G * 32) > 1 ? WG_BYTES / (q.G * 32) : 1;
        q.ppw = (want + q.PT - 1) / q.PT * q.PT;
    }
    q.parts = (q.HW + q.ppw - 1) / q.ppw;
    *out = q;
    return true;
}

}  // namespace

int diff_parts(int fmt_a, int cp_a, int fmt_b, int cp_b, int C, int HW) {
    Job q;
    return make_job(DiffJob{nullptr, fmt_a, cp_a, nullptr, fmt_b, cp_b, C, HW, 0, 0}, &q) ? q.parts : 0;
}

// Scan + finish of `njobs` pairs of N images each: launches of at most MAXJOBS pairs of one format of A, each followed by its
// finish.  partials: diff_parts(...) * N records per job, in job order.  Nothing is allocated or synchronised.
int launch_diff(const DiffJob* jobs, int njobs, int N, void* partials, void* records, hipStream_t stream) {
    if (njobs < 0 || N < 1 || !partials || !records) return (int)hipErrorInvalidValue;
    static const int fmts[] = {FMT_SB, FMT_BF, FMT_F32, FMT_HF, STATS_NCHW};
    std::vector<unsigned long long> part0(njobs);
    unsigned long long total = 0;
    for (int j = 0; j < njobs; ++j) {
        Job q;
        if (!jobs[j].a || !jobs[j].b || !make_job(jobs[j], &q)) return (int)hipErrorInvalidValue;
        part0[j] = total;
        total += (unsigned long long)q.parts * N;
    }
    if (total > 0xffffffffULL) return (int)hipErrorInvalidValue;
    for (int fmt : fmts) {
        Jobs js{};
        js.N = N; js.partials = static_cast<Rec*>(partials); js.records = static_cast<Rec*>(records);
        unsigned long long blocks = 0;
        auto flush = [&]() -> int {
            if (!js.n) return 0;
            if (blocks > 0x7fffffffULL || (unsigned long long)js.n * N > 0x7fffffffULL) return (int)hipErrorInvalidValue;
            const dim3 grid((unsigned)blocks);
            switch (fmt) {
                case FMT_SB: hipLaunchKernelGGL(diff_scan_kernel<FMT_SB>, grid, dim3(NT), 0, stream, js); break;
                case FMT_BF: hipLaunchKernelGGL(diff_scan_kernel<FMT_BF>, grid, dim3(NT), 0, stream, js); break;
                case FMT_F32: hipLaunchKernelGGL(diff_scan_kernel<FMT_F32>, grid, dim3(NT), 0, stream, js); break;
                case FMT_HF: hipLaunchKernelGGL(diff_scan_kernel<FMT_HF>, grid, dim3(NT), 0, stream, js); break;
                default: hipLaunchKernelGGL(diff_scan_nchw_kernel, grid, dim3(NT), 0, stream, js); break;
            }
            int rc = (int)hipGetLastError();
            if (rc) return rc;
            hipLaunchKernelGGL(diff_finish_kernel, dim3((unsigned)(js.n * N)), dim3(64), 0, stream, js);
            rc = (int)hipGetLastError();
            js.n = 0; blocks = 0;
            return rc;
        };
        for (int j = 0; j < njobs; ++j) {
            if (jobs[j].fmt_a != fmt) continue;
            Job q;
            make_job(jobs[j], &q);
            q.block0 = (unsigned)blocks; q.part0 = (unsigned)part0[j];
            blocks += (unsigned long long)q.parts * N;
            js.job[js.n++] = q;
            if (js.n == MAXJOBS || blocks > 0x3fffffffULL)
                if (const int rc = flush()) return rc;
        }
        if (const int rc = flush()) return rc;
    }
    return 0;
}

}  // namespace esa
