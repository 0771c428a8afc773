// layout.hip — f32 NCHW <-> SB (split-bf16 NHWC), BF and F32 conversion.  Used by the per-operator test entry points, by
// esahrnet_tap_read and for seg_hrnet3's heat-maps; the network itself enters its format through the stem kernel.
#include "final2.h"
#include "kernels.h"
#include "sb.h"

namespace esa {
namespace {

// EL (sb.h): EL_SB, EL_BF or EL_HF (fp16: rounded to nearest even, saturated)
template <int EL>
__global__ __launch_bounds__(256) void nchw_to_sb_kernel(const float* x, int N, int C, int H, int W,
                                                         char* y, int Cp, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int G = Cp >> 3;
    const int c8 = (int)(idx % G);
    const long long pix = idx / G;
    const long long hw = (long long)H * W;
    const int n = (int)(pix / hw);
    const long long s = pix - (long long)n * hw;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = c8 * 8 + i;
        v[i] = c < C ? x[((size_t)n * C + c) * hw + s] : 0.f;
    }
    if (el_half(EL)) {
        *reinterpret_cast<uint4*>(y + (size_t)pix * (size_t)(Cp * 2) + c8 * 16) = pack8_el<EL>(v);
        return;
    }
    uint4 hi, lo;
    split8(v, hi, lo);
    char* o = y + (size_t)pix * (size_t)(Cp * 4) + c8 * 32;
    *reinterpret_cast<uint4*>(o) = hi;
    *reinterpret_cast<uint4*>(o + 16) = lo;
}

template <int EL>
__global__ __launch_bounds__(256) void sb_to_nchw_kernel(const char* x, int N, int C, int H, int W,
                                                         int Cp, float* y, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // over (n, c, s), s fastest
    if (idx >= total) return;
    const long long hw = (long long)H * W;
    const long long s = idx % hw;
    const long long nc = idx / hw;
    const int c = (int)(nc % C);
    const int n = (int)(nc / C);
    if (el_half(EL)) {
        const uint32_t b = *reinterpret_cast<const unsigned short*>(x + ((size_t)n * hw + s) * (size_t)(Cp * 2) + c * 2);
        y[idx] = EL == EL_HF ? f16_bits_to_f32(b) : bf16_bits_to_f32(b);
        return;
    }
    const char* a = x + ((size_t)n * hw + s) * (size_t)(Cp * 4) + (c >> 3) * 32 + (c & 7) * 2;
    const uint32_t hi = *reinterpret_cast<const unsigned short*>(a);
    const uint32_t lo = *reinterpret_cast<const unsigned short*>(a + 16);
    y[idx] = bf16_bits_to_f32(hi) + bf16_bits_to_f32(lo);
}

// HF -> NCHW at true scale (esahrnet_tap_read of a tensor stored as T * 2^-e): the conversion above times 2^e, one exact
// multiply (a power of two; beyond f32's range only for a value no forward can hold).  A kernel of its own, so that the
// conversion every other caller uses keeps its code.
__global__ __launch_bounds__(256) void hf_to_nchw_scaled_kernel(const char* x, int C, long long hw, int Cp, float* y, long long total,
                                                                float scale) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // over (n, c, s), s fastest
    if (idx >= total) return;
    const long long s = idx % hw;
    const long long nc = idx / hw;
    const int c = (int)(nc % C);
    const long long n = nc / C;
    const uint32_t b = *reinterpret_cast<const unsigned short*>(x + ((size_t)n * hw + s) * (size_t)(Cp * 2) + c * 2);
    y[idx] = f16_bits_to_f32(b) * scale;
}

// SB -> NCHW for the network output: thread = (pixel, 8-channel group), group fastest, so a wave reads whole pixels
// (contiguous 32-byte groups) and writes 64-byte runs of 16 consecutive pixels into each of its planes.  The element-wise
// kernel above (thread = output element) touches a different 128-byte line per lane for two bytes: 0.9 TB/s.
__global__ __launch_bounds__(256) void sb_to_nchw_groups_kernel(const char* x, int C, long long hw, int Cp, float* y, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int G = (C + 7) >> 3;
    const int g = (int)(idx % G);
    const long long pix = idx / G;                  // n * hw + s
    const long long n = pix / hw, sp = pix - n * hw;
    const char* a = x + (size_t)pix * (size_t)(Cp * 4) + g * 32;
    float v[8];
    join8(*reinterpret_cast<const uint4*>(a), *reinterpret_cast<const uint4*>(a + 16), v);
    float* o = y + ((size_t)n * C + (size_t)g * 8) * (size_t)hw + sp;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (g * 8 + j < C) o[(size_t)j * hw] = v[j];
}

// plain f32 NHWC <-> f32 NCHW: thread = (pixel, 8-channel group), group fastest (a pixel's channels are contiguous)
__global__ __launch_bounds__(256) void nchw_to_f32_kernel(const float* x, int C, long long hw, float* y, int Cp, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int G = Cp >> 3;
    const int c8 = (int)(idx % G);
    const long long pix = idx / G;
    const long long n = pix / hw, s = pix - n * hw;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = c8 * 8 + i;
        v[i] = c < C ? x[((size_t)n * C + c) * hw + s] : 0.f;
    }
    float* o = y + (size_t)pix * Cp + c8 * 8;
    *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
}
__global__ __launch_bounds__(256) void f32_to_nchw_kernel(const float* x, int C, long long hw, int Cp, float* y, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int G = (C + 7) >> 3;
    const int g = (int)(idx % G);
    const long long pix = idx / G;
    const long long n = pix / hw, sp = pix - n * hw;
    const float* a = x + (size_t)pix * Cp + g * 8;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(a), a1 = *reinterpret_cast<const f32x4*>(a + 4);
    const float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    float* o = y + ((size_t)n * C + (size_t)g * 8) * (size_t)hw + sp;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (g * 8 + j < C) o[(size_t)j * hw] = v[j];
}

// The network output with per-tile maxima (seg_hrnet3 under esahrnet_forward_partials): f32 or SB NHWC -> f32 NCHW, the
// same values as the two kernels above.  A workgroup owns TONCHW_TP consecutive row-major pixels of one crop (the last
// tile of a plane is shorter).  It reads them as whole 32-byte channel groups, all loads of a thread in flight at once, turns
// them round in LDS, writes each plane's run with consecutive lanes, and leaves the run's first maximum per plane as (value,
// int bits of row * W + col) in part[(n * C + c) * ntiles + tile], the layout keypoints_finish_kernel reads.  Every step goes
// through argmax_take, whose order does not depend on the order of the steps: the finish over these runs picks what the
// full sweep picks.  Eight waves per workgroup: with 33 KB of LDS four workgroups fit a CU, and those fill it.
constexpr int TONCHW_TP = 256, TONCHW_NT = 512;
// STORE = false (seg_hrnet3 under esahrnet_forward_keypoints): the maxima only, no NCHW copy — the heat-maps stay in the
// workspace and keypoints_finish_nhwc_kernel refines from there; read-bound, Cp * 4 bytes per pixel
template <bool F32, bool STORE>
__global__ __launch_bounds__(TONCHW_NT) void to_nchw_part_kernel(const char* x, int C, int hw, int Cp, float* y, float2* part,
                                                                 int ntiles) {
    __shared__ float s[32][TONCHW_TP + 2];         // C <= 32 planes; (+2: a wave's 8-channel groups write to different banks)
    constexpr int IT = TONCHW_TP * 4 / TONCHW_NT;   // (pixel, 8-channel group) items per thread: G <= 4
    const int tile = (int)(blockIdx.x % (unsigned)ntiles), n = (int)(blockIdx.x / (unsigned)ntiles);
    const int q0 = tile * TONCHW_TP, np = min(TONCHW_TP, hw - q0);
    const int G = (C + 7) >> 3, tid = threadIdx.x;
    uint4 a[IT], b[IT];
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int i = tid + k * TONCHW_NT, pl = i / G, g = i - pl * G;
        if (i < np * G) {
            const char* p = x + ((size_t)n * hw + q0 + pl) * (size_t)(Cp * 4) + g * 32;
            a[k] = *reinterpret_cast<const uint4*>(p);
            b[k] = *reinterpret_cast<const uint4*>(p + 16);
        }
    }
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int i = tid + k * TONCHW_NT, pl = i / G, g = i - pl * G;
        if (i < np * G) {
            float v[8];
            join8_fmt(a[k], b[k], v, F32);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (g * 8 + j < C) s[g * 8 + j][pl] = v[j];
        }
    }
    __syncthreads();
    const int lane = tid & 63;
    for (int c = tid >> 6; c < C; c += TONCHW_NT / 64) {     // plane c: one wave
        float* o = STORE ? y + ((size_t)n * C + c) * hw + q0 : nullptr;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < TONCHW_TP / 64; ++r) {
            const int p = lane + r * 64;
            if (p < np) {
                const float v = s[c][p];
                if constexpr (STORE) o[p] = v;
                argmax_take(v, q0 + p, bv, bi);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            argmax_take(ov, oi, bv, bi);
        }
        if (lane == 0) part[((size_t)n * C + c) * ntiles + tile] = make_float2(bv, __int_as_float(bi));
    }
}
}  // namespace

int to_nchw_part_tiles(int H, int W) {
    const long long hw = (long long)H * W;
    return H > 0 && W > 0 && hw <= 0x7fffffffLL ? (int)((hw + TONCHW_TP - 1) / TONCHW_TP) : 0;
}

int launch_to_nchw_part(int fmt, const char* x, int N, int C, int H, int W, int Cp, float* y, float2* part, hipStream_t s) {
    const int ntiles = to_nchw_part_tiles(H, W);
    const long long nblk = (long long)N * ntiles;
    if (ntiles <= 0 || N <= 0 || nblk > 0x7fffffffLL || C < 1 || C > 32 || C > Cp || (Cp & 7) || (fmt != FMT_SB && fmt != FMT_F32))
        return (int)hipErrorInvalidValue;
    auto kern = fmt == FMT_F32 ? to_nchw_part_kernel<true, true> : to_nchw_part_kernel<false, true>;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(TONCHW_NT), 0, s, x, C, H * W, Cp, y, part, ntiles);
    return (int)hipGetLastError();
}

// get_final2 straight from seg_hrnet3's NHWC heat-maps (final2.h's kernels with the NHWC plane accessor)
int launch_keypoints_final2_nhwc(int fmt, const char* x, int N, int C, int H, int W, int Cp, float* kp, int* idx_out, void* ws,
                                 size_t ws_bytes, hipStream_t stream, double* hess) {
    if (N <= 0 || C < 1 || C > Cp || (Cp & 7) || (long long)N * C > 0x7fffffffLL || (fmt != FMT_SB && fmt != FMT_F32))
        return (int)hipErrorInvalidValue;
    const int planes = N * C;
    if (hess) {
        if (fmt == FMT_F32)
            return launch_final2<F2Nhwc<true>, true>(F2Nhwc<true>{x, C, Cp}, planes, H, W, kp, idx_out, ws, ws_bytes, stream, hess);
        return launch_final2<F2Nhwc<false>, true>(F2Nhwc<false>{x, C, Cp}, planes, H, W, kp, idx_out, ws, ws_bytes, stream, hess);
    }
    if (fmt == FMT_F32) return launch_final2(F2Nhwc<true>{x, C, Cp}, planes, H, W, kp, idx_out, ws, ws_bytes, stream);
    return launch_final2(F2Nhwc<false>{x, C, Cp}, planes, H, W, kp, idx_out, ws, ws_bytes, stream);
}

int launch_tile_max(int fmt, const char* x, int N, int C, int H, int W, int Cp, float2* part, hipStream_t s) {
    const int ntiles = to_nchw_part_tiles(H, W);
    const long long nblk = (long long)N * ntiles;
    if (ntiles <= 0 || N <= 0 || nblk > 0x7fffffffLL || C < 1 || C > 32 || C > Cp || (Cp & 7) || (fmt != FMT_SB && fmt != FMT_F32))
        return (int)hipErrorInvalidValue;
    auto kern = fmt == FMT_F32 ? to_nchw_part_kernel<true, false> : to_nchw_part_kernel<false, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(TONCHW_NT), 0, s, x, C, H * W, Cp, nullptr, part, ntiles);
    return (int)hipGetLastError();
}

int launch_nchw_to_f32(const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s) {
    const long long total = (long long)N * H * W * (Cp >> 3);
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || (Cp & 7) || C > Cp) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(nchw_to_f32_kernel, dim3((unsigned)nblk), dim3(256), 0, s, x, C, (long long)H * W, reinterpret_cast<float*>(y), Cp, total);
    return (int)hipGetLastError();
}

int launch_f32_to_nchw(const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s) {
    const long long total = (long long)N * H * W * ((C + 7) >> 3);
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || C > Cp || (Cp & 7)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(f32_to_nchw_kernel, dim3((unsigned)nblk), dim3(256), 0, s, reinterpret_cast<const float*>(x), C, (long long)H * W, Cp, y, total);
    return (int)hipGetLastError();
}

int launch_nchw_to_fmt(int fmt, const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s) {
    return fmt == FMT_BF ? launch_nchw_to_bf(x, N, C, H, W, y, Cp, s) : fmt == FMT_HF ? launch_nchw_to_hf(x, N, C, H, W, y, Cp, s) : fmt == FMT_F32 ? launch_nchw_to_f32(x, N, C, H, W, y, Cp, s)
                                                                                          : launch_nchw_to_sb(x, N, C, H, W, y, Cp, s);
}
int launch_fmt_to_nchw(int fmt, const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s) {
    return fmt == FMT_BF ? launch_bf_to_nchw(x, N, C, H, W, Cp, y, s) : fmt == FMT_HF ? launch_hf_to_nchw(x, N, C, H, W, Cp, y, s) : fmt == FMT_F32 ? launch_f32_to_nchw(x, N, C, H, W, Cp, y, s)
                                                                                          : launch_sb_to_nchw(x, N, C, H, W, Cp, y, s);
}

int launch_nchw_to_sb(const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s) {
    const long long total = (long long)N * H * W * (Cp >> 3);
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || (Cp & 7) || C > Cp) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(nchw_to_sb_kernel<EL_SB>, dim3((unsigned)nblk), dim3(256), 0, s, x, N, C, H, W, y, Cp, total);
    return (int)hipGetLastError();
}

int launch_nchw_to_bf(const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s) {
    const long long total = (long long)N * H * W * (Cp >> 3);
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || (Cp & 7) || C > Cp) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(nchw_to_sb_kernel<EL_BF>, dim3((unsigned)nblk), dim3(256), 0, s, x, N, C, H, W, y, Cp, total);
    return (int)hipGetLastError();
}

int launch_nchw_to_hf(const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s) {
    const long long total = (long long)N * H * W * (Cp >> 3);
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || (Cp & 7) || C > Cp) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(nchw_to_sb_kernel<EL_HF>, dim3((unsigned)nblk), dim3(256), 0, s, x, N, C, H, W, y, Cp, total);
    return (int)hipGetLastError();
}

int launch_hf_to_nchw(const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s) {
    const long long total = (long long)N * C * H * W;
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || C > Cp) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sb_to_nchw_kernel<EL_HF>, dim3((unsigned)nblk), dim3(256), 0, s, x, N, C, H, W, Cp, y, total);
    return (int)hipGetLastError();
}

int launch_hf_to_nchw_scaled(const char* x, int N, int C, int H, int W, int Cp, float* y, float scale, hipStream_t s) {
    const long long total = (long long)N * C * H * W;
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || C > Cp) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hf_to_nchw_scaled_kernel, dim3((unsigned)nblk), dim3(256), 0, s, x, C, (long long)H * W, Cp, y, total, scale);
    return (int)hipGetLastError();
}

int launch_sb_to_nchw(const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s) {
    const long long total = (long long)N * H * W * ((C + 7) >> 3);
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || C > Cp || (Cp & 7)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sb_to_nchw_groups_kernel, dim3((unsigned)nblk), dim3(256), 0, s, x, C, (long long)H * W, Cp, y, total);
    return (int)hipGetLastError();
}

int launch_bf_to_nchw(const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s) {
    const long long total = (long long)N * C * H * W;
    const long long nblk = (total + 255) / 256;
    if (nblk <= 0 || nblk > 0x7fffffffLL || C > Cp) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sb_to_nchw_kernel<EL_BF>, dim3((unsigned)nblk), dim3(256), 0, s, x, N, C, H, W, Cp, y, total);
    return (int)hipGetLastError();
}

}  // namespace esa
