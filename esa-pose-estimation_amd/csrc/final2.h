// final2.h — the get_final2 tile pass and finish (keypoints_final2.hip's header comment), templated on how a plane is read:
// NCHW f32 (keypoints_final2.hip: esahrnet_keypoints_final2, and the matrix-core output layer's heat-maps under
// esahrnet_forward_keypoints_final2) or seg_hrnet3's NHWC tensor in the forward's workspace, f32 or split-bf16, one channel
// decoded as join8_fmt decodes it (layout.hip: esahrnet_forward_keypoints_final2, no NCHW copy).  The staging, the tap
// order and every f64 sum are the same for both, so the blurred values are the same bits.  No fma anywhere in this file (each
// function turns contraction off itself: layout.hip includes this header too).
#pragma once
#include "kernels.h"
#include "refine.h"
#include "sb.h"

namespace esa {
namespace {

constexpr int F2_TW = 64, F2_TH = 32, F2_R = 5;            // tile width / height, blur radius
constexpr int F2_SW = F2_TW + 2 * F2_R, F2_SH = F2_TH + 2 * F2_R;
constexpr int F2_T = 256;                                  // 4 waves per tile
constexpr int F2_RUN = F2_TH / (F2_T / F2_TW);             // column-pass outputs per thread (a vertical run of 8)

// plane accessors: pl = src.plane(p, H, W) is plane p, pl[i] its value at index i = y * W + x; f2_at(pl, W, y, x) and
// f2_row(pl, W, y)[x] the value at row y, column x
struct F2Nchw {                                            // f32 [planes][H][W]: a plane is its pointer
    const float* heat;
    __device__ __forceinline__ const float* plane(int p, int H, int W) const { return heat + (size_t)p * H * W; }
};
__device__ __forceinline__ float f2_at(const float* pl, int W, int y, int x) { return pl[y * W + x]; }
__device__ __forceinline__ const float* f2_row(const float* pl, int W, int y) { return pl + (size_t)y * W; }
template <bool F32>
struct F2Nhwc {                                            // [N][H][W][Cp], planes n * C + c; f32 or split-bf16 (sb.h)
    const char* x;
    int C, Cp;
    struct Plane {
        const char* img;
        int Cp, j;
        __device__ __forceinline__ float operator[](int i) const { return load1_fmt(img + (size_t)i * (Cp * 4), j, F32); }
    };
    __device__ __forceinline__ Plane plane(int p, int H, int W) const {
        const int n = p / C, c = p - n * C;
        return {x + (size_t)n * ((size_t)H * W * Cp * 4) + (c >> 3) * 32, Cp, c & 7};
    }
};
template <class Plane>
__device__ __forceinline__ float f2_at(const Plane& pl, int W, int y, int x) { return pl[y * W + x]; }
template <class Plane>
__device__ __forceinline__ Plane f2_row(Plane pl, int W, int y) {
    pl.img += (size_t)y * W * (pl.Cp * 4);
    return pl;
}

template <class Src>
__global__ __launch_bounds__(F2_T) void final2_tile_kernel(Src src, int H, int W, int tiles_x, int ntiles, float2* part,
                                                           float* bmax) {
#pragma clang fp contract(off)
    __shared__ float sraw[F2_SH][F2_SW];
    __shared__ double srow[F2_SH][F2_TW];
    __shared__ float sv[F2_T / 64], sb[F2_T / 64];
    __shared__ int si[F2_T / 64];
    const int plane = (int)(blockIdx.x / (unsigned)ntiles), t = (int)(blockIdx.x % (unsigned)ntiles);
    const int y0 = (t / tiles_x) * F2_TH, x0 = (t % tiles_x) * F2_TW;
    const auto pl = src.plane(plane, H, W);
    {                                      // all of a thread's loads in flight before the first LDS write (one wait, not 13)
        constexpr int NST = (F2_SH * F2_SW + F2_T - 1) / F2_T;
        float v[NST];
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = threadIdx.x + j * F2_T, r = i / F2_SW, c = i % F2_SW, y = y0 - F2_R + r, x = x0 - F2_R + c;
            v[j] = (i < F2_SH * F2_SW && y >= 0 && y < H && x >= 0 && x < W) ? f2_at(pl, W, y, x) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = threadIdx.x + j * F2_T;
            if (i < F2_SH * F2_SW) sraw[i / F2_SW][i % F2_SW] = v[j];
        }
    }
    __syncthreads();
    float bv = -INFINITY, bm = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < F2_TH * F2_TW; i += F2_T) {
        const int r = i / F2_TW, c = i % F2_TW, y = y0 + r, x = x0 + c;
        if (y < H && x < W) argmax_take(sraw[r + F2_R][c + F2_R], y * W + x, bv, bi);
    }
    for (int i = threadIdx.x; i < F2_SH * F2_TW; i += F2_T) {               // row pass: every staged row, the tile's columns
        const int r = i / F2_TW, c = i % F2_TW;
        srow[r][c] = blur_taps([&](int k) { return sraw[r][c + k]; });
    }
    __syncthreads();
    {                                                                       // column pass: a run of F2_RUN rows per thread
        const int c = threadIdx.x % F2_TW, r0 = (threadIdx.x / F2_TW) * F2_RUN, x = x0 + c;
        double col[F2_RUN + 2 * F2_R];
#pragma unroll
        for (int j = 0; j < F2_RUN + 2 * F2_R; ++j) col[j] = srow[r0 + j][c];
#pragma unroll
        for (int j = 0; j < F2_RUN; ++j) {
            const float b = (float)blur_taps([&](int k) { return col[j + k]; });
            if (y0 + r0 + j < H && x < W) bm = max_nan(bm, b);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        argmax_take(ov, oi, bv, bi);
        bm = max_nan(bm, __shfl_xor(bm, off));
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; sb[threadIdx.x >> 6] = bm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < F2_T / 64; ++w) { argmax_take(sv[w], si[w], bv, bi); bm = max_nan(bm, sb[w]); }
        part[blockIdx.x] = make_float2(bv, __int_as_float(bi));
        bmax[blockIdx.x] = bm;
    }
}

// blurred value at (y, x) of plane pl, exactly as the tile pass computes it: the row pass at rows y-5..y+5 (zero outside the
// plane), then the column pass over those 11 values
template <class Plane>
__device__ __forceinline__ double blur_at(Plane pl, int H, int W, int y, int x) {
#pragma clang fp contract(off)
    auto row = [&](int r) {
        const int yy = y - F2_R + r;
        if (yy < 0 || yy >= H) return blur_taps([](int) { return 0.f; });
        const auto pr = f2_row(pl, W, yy);
        return blur_taps([&](int k) { const int xx = x - F2_R + k; return xx >= 0 && xx < W ? pr[xx] : 0.f; });
    };
    return blur_taps([&](int r) { return row(r); });
}

// HESS: also hess[plane] = (dxx, dxy, dyy) (refine.h final2_finish); the false instantiation never reads `hess`
template <class Src, bool HESS>
__global__ __launch_bounds__(64) void final2_finish_kernel(Src src, const float2* part, const float* bmax, int ntiles, int H,
                                                           int W, float* kp, int* idx_out, double* hess) {
#pragma clang fp contract(off)
    const int plane = blockIdx.x;
    float bv;
    int bi;
    reduce_tile_maxima(part + (size_t)plane * ntiles, ntiles, bv, bi);
    float bm = -INFINITY;
    for (int t = threadIdx.x; t < ntiles; t += 64) bm = max_nan(bm, bmax[(size_t)plane * ntiles + t]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bm = max_nan(bm, __shfl_xor(bm, off));
    if (bi == 0x7fffffff) bi = 0;                          // all -inf plane
    const int px = bi % W, py = bi / W;
    const auto pl = src.plane(plane, H, W);
    final2_finish<HESS>(
        bv, bi, bm, H, W,
        [&](int j) { return (float)blur_at(pl, H, W, py + final2_point_dy(j), px + final2_point_dx(j)); },
        [&] { return pl[bi]; }, kp, idx_out, plane, hess);
}

// HESS: the finish also writes hess f64 [planes][3] (not null).  A template flag, so that a file which never asks for the
// Hessian instantiates the two kernels it always had.
template <class Src, bool HESS = false>
int launch_final2(Src src, int planes, int H, int W, float* kp, int* idx_out, void* ws, size_t ws_bytes, hipStream_t stream,
                  double* hess = nullptr) {
    if (HESS != (hess != nullptr)) return (int)hipErrorInvalidValue;
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const int ntiles = final2_tiles(H, W);
    if ((long long)planes * ntiles > 0x7fffffLL || ws_bytes < final2_workspace_bytes(planes, H, W) ||
        (reinterpret_cast<uintptr_t>(ws) & 255))
        return (int)hipErrorInvalidValue;
    const size_t nt = (size_t)planes * ntiles;
    float2* part = static_cast<float2*>(ws);
    float* bmax = reinterpret_cast<float*>(static_cast<char*>(ws) + ((nt * 8 + 255) & ~(size_t)255));
    hipLaunchKernelGGL(final2_tile_kernel<Src>, dim3((unsigned)nt), dim3(F2_T), 0, stream, src, H, W, (W + F2_TW - 1) / F2_TW,
                       ntiles, part, bmax);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((final2_finish_kernel<Src, HESS>), dim3((unsigned)planes), dim3(64), 0, stream, src, part, bmax, ntiles, H,
                       W, kp, idx_out, hess);
    return (int)hipGetLastError();
}

}  // namespace
}  // namespace esa
