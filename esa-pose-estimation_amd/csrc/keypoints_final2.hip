// keypoints_final2.hip — heat-maps -> keypoints with the reference's second decoder, get_final2 (inference.py:154-169):
// an 11x11 Gaussian blur of each plane rescaled to the plane's raw maximum (gaussian_blur, :96-111), np.maximum(., 1e-10),
// log, then one Newton step with the full 2x2 Hessian (taylor, :54-73).  f32 [planes][H][W] -> f32 [planes][3] = (x, y, raw
// peak) and the int32 arg-max index, the same layout and the same arg-max / peak bits as keypoints.hip.
//
// Two launches, the heat-maps are read once and the blurred planes never leave the chip:
//   tile pass   one workgroup per (plane, 32x64 tile): the tile and its 5-pixel halo (zeros outside the plane) go to LDS,
//               a row pass and a column pass in f64 (fixed tap order) give the blurred tile, rounded to f32; the workspace
//               receives the tile's first raw maximum (value, index), as the output layer's per-tile maxima do, and its
//               blurred maximum (NaN wins, as in np.max).
//   finish      one wave per plane: the first raw maximum over the tiles (reduce_tile_maxima: the arg-max and peak of
//               launch_keypoints), the blurred maximum, and the 13 blurred values the Newton step reads, each re-evaluated
//               from the raw plane (121 taps) by the tile pass's own function, so that they are the same f32 values.
// Numerics (refine.h final2_newton): the restatement in tests/final2_ref.py.  No fma anywhere in this file: the host
// restatement sums in plain IEEE f64.
#include "kernels.h"
#include "refine.h"

#pragma clang fp contract(off)

namespace esa {
namespace {

constexpr int F2_TW = 64, F2_TH = 32, F2_R = 5;            // tile width / height, blur radius
constexpr int F2_SW = F2_TW + 2 * F2_R, F2_SH = F2_TH + 2 * F2_R;
constexpr int F2_T = 256;                                  // 4 waves per tile
constexpr int F2_RUN = F2_TH / (F2_T / F2_TW);             // column-pass outputs per thread (a vertical run of 8)

__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

// sum_t G[t] * p[t * stride], t = 0..10 in this order, in f64 (the one summation both passes and both kernels use)
template <class V>
__device__ __forceinline__ double blur_taps(V p) {
    double a = kFinal2Gauss[0] * (double)p(0);
#pragma unroll
    for (int t = 1; t < 11; ++t) a = a + kFinal2Gauss[t] * (double)p(t);
    return a;
}

__global__ __launch_bounds__(F2_T) void final2_tile_kernel(const float* heat, int H, int W, int tiles_x, int ntiles,
                                                           float2* part, float* bmax) {
    __shared__ float sraw[F2_SH][F2_SW];
    __shared__ double srow[F2_SH][F2_TW];
    __shared__ float sv[F2_T / 64], sb[F2_T / 64];
    __shared__ int si[F2_T / 64];
    const int plane = (int)(blockIdx.x / (unsigned)ntiles), t = (int)(blockIdx.x % (unsigned)ntiles);
    const int y0 = (t / tiles_x) * F2_TH, x0 = (t % tiles_x) * F2_TW;
    const float* pl = heat + (size_t)plane * H * W;
    {                                      // all of a thread's loads in flight before the first LDS write (one wait, not 13)
        constexpr int NST = (F2_SH * F2_SW + F2_T - 1) / F2_T;
        float v[NST];
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = threadIdx.x + j * F2_T, r = i / F2_SW, c = i % F2_SW, y = y0 - F2_R + r, x = x0 - F2_R + c;
            v[j] = (i < F2_SH * F2_SW && y >= 0 && y < H && x >= 0 && x < W) ? pl[y * W + x] : 0.f;
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
__device__ __forceinline__ double blur_at(const float* pl, int H, int W, int y, int x) {
    auto row = [&](int r) {
        const int yy = y - F2_R + r;
        if (yy < 0 || yy >= H) return blur_taps([](int) { return 0.f; });
        const float* pr = pl + (size_t)yy * W;
        return blur_taps([&](int k) { const int xx = x - F2_R + k; return xx >= 0 && xx < W ? pr[xx] : 0.f; });
    };
    return blur_taps([&](int r) { return row(r); });
}

__global__ __launch_bounds__(64) void final2_finish_kernel(const float* heat, const float2* part, const float* bmax, int ntiles,
                                                           int H, int W, float* kp, int* idx_out) {
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
    const float* pl = heat + (size_t)plane * H * W;
    // gaussian_blur's rescale factor origin_max / max(blurred), f32 (inference.py:110)
    const float s = (float)((double)bv / (double)bm);
    const bool go = 1 < px && px < W - 2 && 1 < py && py < H - 2 && isfinite(bv) && isfinite(bm) && isfinite(s);
    float lv = 0.f;                                        // lane j < 13: log of the rescaled, clamped blurred value at point j
    if (go && threadIdx.x < 13) {
        const int j = threadIdx.x;
        const float b = (float)blur_at(pl, H, W, py + final2_point_dy(j), px + final2_point_dx(j));
        lv = final2_log(b, s);
    }
    float h[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) h[j] = __shfl(lv, j);
    if (threadIdx.x == 0) {
        float fx = (float)px, fy = (float)py;
        if (go) final2_newton(h, px, py, fx, fy);
        float* kp3 = kp + (size_t)plane * 3;
        kp3[0] = fx;
        kp3[1] = fy;
        kp3[2] = pl[bi];
        if (idx_out) idx_out[plane] = bi;
    }
}

}  // namespace

int final2_tiles(int H, int W) { return ((H + F2_TH - 1) / F2_TH) * ((W + F2_TW - 1) / F2_TW); }

size_t final2_workspace_bytes(long long planes, int H, int W) {
    const size_t nt = (size_t)planes * final2_tiles(H, W);
    return ((nt * 8 + 255) & ~(size_t)255) + ((nt * 4 + 255) & ~(size_t)255);
}

int launch_keypoints_final2(const float* heat, int planes, int H, int W, float* kp, int* idx_out, void* ws, size_t ws_bytes,
                            hipStream_t stream) {
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const int ntiles = final2_tiles(H, W);
    if ((long long)planes * ntiles > 0x7fffffLL || ws_bytes < final2_workspace_bytes(planes, H, W) ||
        (reinterpret_cast<uintptr_t>(ws) & 255))
        return (int)hipErrorInvalidValue;
    const size_t nt = (size_t)planes * ntiles;
    float2* part = static_cast<float2*>(ws);
    float* bmax = reinterpret_cast<float*>(static_cast<char*>(ws) + ((nt * 8 + 255) & ~(size_t)255));
    hipLaunchKernelGGL(final2_tile_kernel, dim3((unsigned)nt), dim3(F2_T), 0, stream, heat, H, W, (W + F2_TW - 1) / F2_TW, ntiles,
                       part, bmax);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(final2_finish_kernel, dim3((unsigned)planes), dim3(64), 0, stream, heat, part, bmax, ntiles, H, W, kp,
                       idx_out);
    return (int)hipGetLastError();
}

}  // namespace esa
