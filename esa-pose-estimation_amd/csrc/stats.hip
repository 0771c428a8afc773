// stats.hip — the activation range report: one record of esahrnet_stats_record (include/esahrnet.h) per (tensor, image), scanned
// from the tensors where a forward left them.  Two stages, both fixed by the tensor's shape alone:
//   scan    a workgroup owns a fixed range of pixels of ONE image and leaves one partial record.  Its lanes cover consecutive
//           16-byte chunks of consecutive pixels (every load instruction of a wave reads whole 128-byte lines); a lane keeps
//           the same chunk position of the pixel from iteration to iteration, so which of its channels are real (c < C) is
//           computed once, outside the pixel loop.  Lane -> wave (xor tree) -> workgroup (wave order): a fixed order.
//   finish  one wave per (tensor, image) adds that image's partials: maxima and counts exactly, sum_abs in index order.
// No atomics, and neither the number of partials of an image nor any offset inside an image depends on the batch: the image
// enters through a 64-bit base only, so an image's record has the same bits alone, in a batch and in a permuted batch.
// The scan is read-bound by design: 16 bytes per lane and load, a few VALU instructions per element.
#include <cstddef>
#include <vector>

#include "../../include/esahrnet.h"
#include "kernels.h"
#include "sb.h"

namespace esa {
namespace {

typedef esahrnet_stats_record Rec;
static_assert(sizeof(Rec) == ESAHRNET_STATS_RECORD_BYTES, "the record is 64 bytes");
static_assert(offsetof(Rec, sum_abs) == 0 && offsetof(Rec, max_abs) == 8 && offsetof(Rec, n_finite) == 20 &&
              offsetof(Rec, n_f16_tiny) == 40 && offsetof(Rec, reserved) == 44, "the record has no holes");

constexpr int NT = 256;                     // threads of a scan workgroup
constexpr int WG_BYTES = 32768;             // bytes a scan workgroup owns (about: whole pixels, a multiple of its pixel stride)
constexpr int MAXJOBS = 16;                 // tensors per launch (the job table travels as a kernel argument)

struct Job {
    const char* x;
    unsigned long long img_bytes;           // one image of the tensor
    int pix_bytes, Q, QT, PT;               // chunks per pixel; a workgroup's lanes cover QT chunks of PT pixels at a time
    int HW, C, ppw, parts;                  // pixels (NCHW: elements) per image and per workgroup; partials per image
    unsigned block0, part0;                 // first workgroup of the job in the launch; first partial in the workspace
    int row, pad;
};
struct Jobs {
    int n, N;
    esahrnet_stats_record* partials;        // the workspace: the jobs' partials, Job::part0 onwards, image-major
    esahrnet_stats_record* records;         // [rows][N]
    Job job[MAXJOBS];
};

// what a lane has seen.  Non-finite values enter the maxima and the sum as 0 / +-inf, so that no NaN reaches a v_max; the
// three counters z, ge, lt are taken of that sanitised |x| and sorted out once per workgroup (write_partial)
struct Acc {
    double sum;
    float max_abs, mn, mx;
    unsigned cnt, nan, inf, z, ge, lt;
};
__device__ __forceinline__ Acc acc_init() { return Acc{0.0, 0.f, INFINITY, -INFINITY, 0u, 0u, 0u, 0u, 0u, 0u}; }

__device__ __forceinline__ void take(Acc& a, float x) {
    const float ab = fabsf(x);
    const bool fin = ab < INFINITY;         // false for NaN and +-inf
    const float af = fin ? ab : 0.f;
    a.nan += x != x ? 1u : 0u;
    a.inf += ab == INFINITY ? 1u : 0u;
    a.max_abs = fmaxf(a.max_abs, af);
    a.mn = fminf(a.mn, fin ? x : INFINITY);
    a.mx = fmaxf(a.mx, fin ? x : -INFINITY);
    a.sum += (double)af;
    a.z += af == 0.f ? 1u : 0u;             // +-0 and the non-finite
    a.ge += af >= 65504.f ? 1u : 0u;
    a.lt += af < 0x1p-14f ? 1u : 0u;        // fp16's subnormal range, +-0 and the non-finite
}

__device__ __forceinline__ void merge(Acc& a, const Acc& b) {
    a.sum += b.sum;
    a.max_abs = fmaxf(a.max_abs, b.max_abs); a.mn = fminf(a.mn, b.mn); a.mx = fmaxf(a.mx, b.mx);
    a.cnt += b.cnt; a.nan += b.nan; a.inf += b.inf; a.z += b.z; a.ge += b.ge; a.lt += b.lt;
}

__device__ __forceinline__ Acc shfl_acc(const Acc& a, int m) {
    Acc b;
    b.sum = __shfl_xor(a.sum, m);
    b.max_abs = __shfl_xor(a.max_abs, m); b.mn = __shfl_xor(a.mn, m); b.mx = __shfl_xor(a.mx, m);
    b.cnt = __shfl_xor(a.cnt, m); b.nan = __shfl_xor(a.nan, m); b.inf = __shfl_xor(a.inf, m);
    b.z = __shfl_xor(a.z, m); b.ge = __shfl_xor(a.ge, m); b.lt = __shfl_xor(a.lt, m);
    return b;
}

// the workgroup's partial record: lanes by an xor tree, then the waves in wave order (executed by all NT threads)
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
    r.sum_abs = a.sum; r.max_abs = a.max_abs; r.min = a.mn; r.max = a.mx;
    r.n_finite = a.cnt - a.nan - a.inf; r.n_nan = a.nan; r.n_inf = a.inf;
    r.n_zero = a.z - a.nan - a.inf; r.n_ge_f16max = a.ge; r.n_f16_tiny = a.lt - a.z;
    for (int i = 0; i < 5; ++i) r.reserved[i] = 0u;
    *out = r;
}

__device__ __forceinline__ Job find_job(const Jobs& js) {
    int j = 0;
    while (j + 1 < js.n && blockIdx.x >= js.job[j + 1].block0) ++j;
    return js.job[j];
}

// the neighbour's dword inside a lane pair (quad_perm [1, 0, 3, 2]); both lanes of a pair are always active together
__device__ __forceinline__ uint32_t pair_swap(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
}

// FMT: the FMT_* codes.  Values per 16-byte chunk: F32 4; SB 4 (chunk 2g is the hi half of channels 8g..8g+7, chunk 2g+1 their
// lo half: the even lane of a pair takes channels 8g..8g+3 and the odd lane 8g+4..8g+7, each with two dwords of the other's
// chunk, and forms hi + lo as join8 does); BF and HF 8.
template <int FMT>
__global__ __launch_bounds__(NT) void stats_scan_kernel(Jobs js) {
    constexpr int NV = FMT == FMT_F32 || FMT == FMT_SB ? 4 : 8;
    const Job q = find_job(js);
    const unsigned local = blockIdx.x - q.block0;
    const unsigned img = local / (unsigned)q.parts, part = local - img * (unsigned)q.parts;
    const char* base = q.x + (size_t)img * q.img_bytes;         // 64-bit per image, 32-bit inside it
    const int p_begin = (int)part * q.ppw, p_end = min(p_begin + q.ppw, q.HW);
    const int tid = threadIdx.x;
    Acc a = acc_init();
    if (tid < q.QT * q.PT) {
        const int q0 = tid % q.QT, p0 = tid / q.QT;
        for (int c = q0; c < q.Q; c += q.QT) {                  // (one pass unless a pixel has more than NT chunks)
            const int ch0 = FMT == FMT_SB ? (c >> 1) * 8 + (c & 1) * 4 : c * NV;
            const int nreal = min(max(q.C - ch0, 0), NV);       // the lane's real channels: once, not per element
            const unsigned step = (unsigned)q.PT * (unsigned)q.pix_bytes;
            unsigned off = (unsigned)(p_begin + p0) * (unsigned)q.pix_bytes + (unsigned)c * 16u;
#pragma unroll 4
            for (int p = p_begin + p0; p < p_end; p += q.PT, off += step) {
                const uint4 v = *reinterpret_cast<const uint4*>(base + off);
                float f[NV];
                if constexpr (FMT == FMT_F32) {
                    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
                } else if constexpr (FMT == FMT_SB) {
                    const bool odd = c & 1;
                    const uint32_t r0 = pair_swap(odd ? v.x : v.z), r1 = pair_swap(odd ? v.y : v.w);
                    const uint2 hi = odd ? make_uint2(r0, r1) : make_uint2(v.x, v.y);
                    const uint2 lo = odd ? make_uint2(v.z, v.w) : make_uint2(r0, r1);
                    join4(hi, lo, f);
                } else if constexpr (FMT == FMT_HF) {
                    unpack8_f16(v, f);
                } else {
                    unpack8_bf16(v, f);
                }
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (k < nreal) take(a, f[k]);
                a.cnt += (unsigned)nreal;
            }
        }
    }
    write_partial(a, js.partials + q.part0 + (size_t)img * (unsigned)q.parts + part);
}

// plain f32 [N][C][H][W] (heat-maps in caller memory): every element is real; a workgroup owns ppw consecutive elements of
// one image, a wave's lanes read consecutive dwords (256 bytes per load instruction)
__global__ __launch_bounds__(NT) void stats_scan_nchw_kernel(Jobs js) {
    const Job q = find_job(js);
    const unsigned local = blockIdx.x - q.block0;
    const unsigned img = local / (unsigned)q.parts, part = local - img * (unsigned)q.parts;
    const float* base = reinterpret_cast<const float*>(q.x + (size_t)img * q.img_bytes);
    const int e_begin = (int)part * q.ppw, e_end = min(e_begin + q.ppw, q.HW);
    Acc a = acc_init();
#pragma unroll 4
    for (int e = e_begin + (int)threadIdx.x; e < e_end; e += NT) {
        take(a, base[e]);
        a.cnt += 1u;
    }
    write_partial(a, js.partials + q.part0 + (size_t)img * (unsigned)q.parts + part);
}

// one wave per (job, image): the image's partials into its record.  Maxima and counts are exact in any order; sum_abs is
// added by lane 0 in index order.
__global__ __launch_bounds__(64) void stats_finish_kernel(Jobs js) {
    const Job q = js.job[blockIdx.x / (unsigned)js.N];
    const unsigned img = blockIdx.x % (unsigned)js.N;
    const Rec* p = js.partials + q.part0 + (size_t)img * (unsigned)q.parts;
    const int lane = threadIdx.x;
    Rec r;
    r.sum_abs = 0.0; r.max_abs = 0.f; r.min = INFINITY; r.max = -INFINITY;
    r.n_finite = r.n_nan = r.n_inf = r.n_zero = r.n_ge_f16max = r.n_f16_tiny = 0u;
    for (int i = lane; i < q.parts; i += 64) {
        const Rec t = p[i];
        r.max_abs = fmaxf(r.max_abs, t.max_abs); r.min = fminf(r.min, t.min); r.max = fmaxf(r.max, t.max);
        r.n_finite += t.n_finite; r.n_nan += t.n_nan; r.n_inf += t.n_inf; r.n_zero += t.n_zero;
        r.n_ge_f16max += t.n_ge_f16max; r.n_f16_tiny += t.n_f16_tiny;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        r.max_abs = fmaxf(r.max_abs, __shfl_xor(r.max_abs, m));
        r.min = fminf(r.min, __shfl_xor(r.min, m)); r.max = fmaxf(r.max, __shfl_xor(r.max, m));
        r.n_finite += __shfl_xor(r.n_finite, m); r.n_nan += __shfl_xor(r.n_nan, m); r.n_inf += __shfl_xor(r.n_inf, m);
        r.n_zero += __shfl_xor(r.n_zero, m); r.n_ge_f16max += __shfl_xor(r.n_ge_f16max, m);
        r.n_f16_tiny += __shfl_xor(r.n_f16_tiny, m);
    }
    if (lane != 0) return;
    for (int i = 0; i < q.parts; ++i) r.sum_abs += p[i].sum_abs;
    for (int i = 0; i < 5; ++i) r.reserved[i] = 0u;
    js.records[(size_t)q.row * (unsigned)js.N + img] = r;
}

// the shape-only geometry of a job; false: a shape the scan does not serve
bool make_job(const StatsJob& s, Job* out) {
    Job q{};
    q.x = static_cast<const char*>(s.x); q.C = s.C; q.row = s.row;
    if (s.C < 1 || s.HW < 1) return false;
    if (s.fmt == STATS_NCHW) {
        const long long e = (long long)s.C * s.HW;
        if (e > 0x1fffffffLL) return false;                     // (32-bit byte offsets inside an image)
        q.HW = (int)e; q.img_bytes = (unsigned long long)e * 4; q.ppw = WG_BYTES / 4;
    } else {
        const bool half = fmt_half(s.fmt);
        if (s.fmt != FMT_SB && s.fmt != FMT_F32 && !half) return false;
        if (s.C > s.Cp || s.Cp % (half ? 8 : 4) || (s.fmt == FMT_SB && s.Cp % 8)) return false;
        const long long pix = (long long)s.Cp * (half ? 2 : 4), img = pix * s.HW;
        if (img > 0x7fffffffLL || (long long)s.C * s.HW > 0xffffffffLL) return false;
        q.pix_bytes = (int)pix; q.Q = (int)(pix / 16); q.QT = q.Q < NT ? q.Q : NT; q.PT = NT / q.QT;
        q.HW = s.HW; q.img_bytes = (unsigned long long)img;
        const int want = (int)(WG_BYTES / pix) > 1 ? (int)(WG_BYTES / pix) : 1;
        q.ppw = (want + q.PT - 1) / q.PT * q.PT;
    }
    q.parts = (q.HW + q.ppw - 1) / q.ppw;
    *out = q;
    return true;
}

}  // namespace

int stats_parts(int fmt, int C, int Cp, int HW) {
    Job q;
    return make_job(StatsJob{nullptr, fmt, C, Cp, HW, 0}, &q) ? q.parts : 0;
}

// Scan + finish of `njobs` tensors of N images each: launches of at most MAXJOBS tensors of one format, each followed by its
// finish.  partials: stats_parts(...) * N records per job, in job order.  Nothing is allocated or synchronised.
int launch_stats(const StatsJob* jobs, int njobs, int N, void* partials, void* records, hipStream_t stream) {
    if (njobs < 0 || N < 1 || !partials || !records) return (int)hipErrorInvalidValue;
    static const int fmts[] = {FMT_SB, FMT_BF, FMT_F32, FMT_HF, STATS_NCHW};
    std::vector<unsigned long long> part0(njobs);
    unsigned long long total = 0;
    for (int j = 0; j < njobs; ++j) {
        Job q;
        if (!jobs[j].x || !make_job(jobs[j], &q)) return (int)hipErrorInvalidValue;
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
                case FMT_SB: hipLaunchKernelGGL(stats_scan_kernel<FMT_SB>, grid, dim3(NT), 0, stream, js); break;
                case FMT_BF: hipLaunchKernelGGL(stats_scan_kernel<FMT_BF>, grid, dim3(NT), 0, stream, js); break;
                case FMT_F32: hipLaunchKernelGGL(stats_scan_kernel<FMT_F32>, grid, dim3(NT), 0, stream, js); break;
                case FMT_HF: hipLaunchKernelGGL(stats_scan_kernel<FMT_HF>, grid, dim3(NT), 0, stream, js); break;
                default: hipLaunchKernelGGL(stats_scan_nchw_kernel, grid, dim3(NT), 0, stream, js); break;
            }
            int rc = (int)hipGetLastError();
            if (rc) return rc;
            hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)(js.n * N)), dim3(64), 0, stream, js);
            rc = (int)hipGetLastError();
            js.n = 0; blocks = 0;
            return rc;
        };
        for (int j = 0; j < njobs; ++j) {
            if (jobs[j].fmt != fmt) continue;
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
