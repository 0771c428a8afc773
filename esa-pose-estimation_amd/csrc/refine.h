// refine.h — integer peak -> sub-pixel keypoint, the one refinement every keypoint kernel uses (keypoints.hip: the heat-map
// sweep and the finishes over per-tile maxima, NCHW or NHWC; head.hip: the finish of the keypoints-only VALU output layer),
// and the pieces every get_final2 kernel shares (keypoints_final2.hip's tile pass and finish over NCHW or NHWC heat-maps; head.hip's
// blurring output layer and its finish): the f64 blur taps, the Newton step and the end of the finish.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace esa {

// integer peak `bi` (row * W + column) of a plane whose values at(row, col) returns -> kp3 = (x, y, peak): the 9-tap
// log-quadratic offset in f64 exactly as the reference's Python floats do (inference.py:75-94, 136-152).  `at` is called
// for the peak and, when the peak is at least 2 px inside the plane, for its 8 neighbours at +-1 and +-2 in x and in y.
template <class At>
__device__ __forceinline__ void refine_keypoint(At at, int H, int W, int bi, float* kp3, int* idx_slot) {
    if (bi == 0x7fffffff) bi = 0;                        // all-NaN / all -inf plane
    const int px = bi % W, py = bi / W;
    float fx = (float)px, fy = (float)py;
    if (1 < px && px < W - 2 && 1 < py && py < H - 2) {   // inference.py:81
        // np.maximum(hm, 1e-10) of inference.py:141 (NaN-propagating, unlike fmaxf), then math.log in f64
        auto lg = [&](int yy, int xx) {
            const float v = at(yy, xx);
            return log((double)(v < 1e-10f ? 1e-10f : v));
        };
        const double c = lg(py, px);
        const double hx = 0.5 * (lg(py, px + 1) - lg(py, px - 1));
        const double hy = 0.5 * (lg(py + 1, px) - lg(py - 1, px));
        const double hxx = 0.25 * (lg(py, px + 2) - 2 * c + lg(py, px - 2));
        const double hyy = 0.25 * (lg(py + 2, px) - 2 * c + lg(py - 2, px));
        if (hxx != 0 && hyy != 0) {
            const double ox = -hx / hxx, oy = -hy / hyy;
            if (ox < 1 && oy < 1) {                        // signed, both-or-neither (:92)
                fx = (float)((double)fx + ox);
                fy = (float)((double)fy + oy);
            }
        }
    }
    kp3[0] = fx;
    kp3[1] = fy;
    kp3[2] = at(py, px);
    if (idx_slot) *idx_slot = bi;
}

// first maximum of a plane over its `ntiles` per-tile maxima pp[0 .. ntiles), one wave: every lane ends with the same
// (value, index) — argmax_take's order does not depend on the order of its steps
__device__ __forceinline__ void reduce_tile_maxima(const float2* pp, int ntiles, float& bv, int& bi) {
    bv = -INFINITY;
    bi = 0x7fffffff;
    for (int t = threadIdx.x; t < ntiles; t += 64) {
        const float2 q = pp[t];
        argmax_take(q.x, __float_as_int(q.y), bv, bi);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        argmax_take(ov, oi, bv, bi);
    }
}

// The nine pixels refine_keypoint reads around a peak, numbered: 0 the peak, 1 / 2 x -1 / +1, 3 / 4 x -2 / +2, 5 / 6 y -1 / +1,
// 7 / 8 y -2 / +2.  Kernels that evaluate those pixels themselves (instead of reading a stored heat-map) use this order.
__device__ __forceinline__ int refine_point_dx(int pt) { return pt == 0 || pt > 4 ? 0 : (pt & 1 ? -1 : 1) * ((pt + 1) >> 1); }
__device__ __forceinline__ int refine_point_dy(int pt) { return pt <= 4 ? 0 : (pt & 1 ? -1 : 1) * ((pt - 3) >> 1); }
__device__ __forceinline__ int refine_point_of(int dy, int dx) {
    if (dy == 0) return dx == 0 ? 0 : dx == -1 ? 1 : dx == 1 ? 2 : dx == -2 ? 3 : 4;
    return dy == -1 ? 5 : dy == 1 ? 6 : dy == -2 ? 7 : 8;
}

// ---- get_final2 (inference.py:154-169): blur, rescale, log, full-Hessian Newton step ------------------------------------
// The 11 taps of cv2.GaussianBlur(., (11, 11), 0) (getGaussianKernel: sigma 0.3 * ((11 - 1) * 0.5 - 1) + 0.8 = 2,
// t_i = exp(-(i - 5)^2 / 8), each times 1 / sum_i t_i, in f64), written out so that host and device agree on every bit.
constexpr double kFinal2Gauss[11] = {0x1.20c2564ee6770p-7, 0x1.bcb86a082c301p-6, 0x1.0ab50979aaf94p-4, 0x1.f2464c62edaf4p-4,
                                     0x1.6a7e1d504a91ep-3, 0x1.9ac20a36ea596p-3, 0x1.6a7e1d504a91ep-3, 0x1.f2464c62edaf4p-4,
                                     0x1.0ab50979aaf94p-4, 0x1.bcb86a082c301p-6, 0x1.20c2564ee6770p-7};

__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }   // np.max: NaN wins

// sum_t G[t] * p[t * stride], t = 0..10 in this order, in f64 without fma: the one summation of the blur's row and column
// passes, in every get_final2 kernel (the tile passes, the finishes) and in the host restatement
template <class V>
__device__ __forceinline__ double blur_taps(V p) {
#pragma clang fp contract(off)
    double a = kFinal2Gauss[0] * (double)p(0);
#pragma unroll
    for (int t = 1; t < 11; ++t) a = a + kFinal2Gauss[t] * (double)p(t);
    return a;
}

// The 13 blurred points the Newton step reads: 0..8 as refine_point_dx / _dy, then 9 / 10 / 11 / 12 at (y-1, x-1),
// (y-1, x+1), (y+1, x-1), (y+1, x+1).
__device__ __forceinline__ int final2_point_dx(int pt) { return pt < 9 ? refine_point_dx(pt) : pt & 1 ? -1 : 1; }
__device__ __forceinline__ int final2_point_dy(int pt) { return pt < 9 ? refine_point_dy(pt) : pt < 11 ? -1 : 1; }

// blurred f32 value b -> the value the Newton step reads: b * s in f32 (the rescale, inference.py:110), np.maximum(., 1e-10)
// (NaN-propagating), then log, taken as f32(log(f64(.))) on host and device alike (NumPy's f32 log may differ by one ulp)
__device__ __forceinline__ float final2_log(float b, float s) {
#pragma clang fp contract(off)
    float v = (float)((double)b * (double)s);              // exact product, one rounding: the f32 product
    v = v < 1e-10f ? 1e-10f : v;
    return (float)log((double)v);
}

// taylor (inference.py:54-73) on the 13 log values h[]: the differences of two f32 values are f32 (NumPy scalars), the first
// product with a Python number and everything after it f64 (NumPy 1.x promotion); the inverse in closed form.  The step is
// taken when det != 0 and the offset is finite; then (fx, fy) = f32(f64(p) + offset).  HESS: a step that is taken also leaves
// the Hessian it used in hess3 = (dxx, dxy, dyy) (otherwise hess3 is not touched); the false instantiation is the code it was.
template <bool HESS = false>
__device__ __forceinline__ void final2_newton(const float* h, int px, int py, float& fx, float& fy, double* hess3 = nullptr) {
#pragma clang fp contract(off)                             // the host restatement has no fma
    const double dx = 0.5 * (double)(h[2] - h[1]);
    const double dy = 0.5 * (double)(h[6] - h[5]);
    const double c2 = 2 * (double)h[0];
    const double dxx = 0.25 * (((double)h[4] - c2) + (double)h[3]);
    const double dyy = 0.25 * (((double)h[8] - c2) + (double)h[7]);
    const double dxy = 0.25 * (double)(((h[12] - h[10]) - h[11]) + h[9]);
    const double det = dxx * dyy - dxy * dxy;
    if (det != 0) {
        const double i00 = dyy / det, i01 = -dxy / det, i11 = dxx / det;
        const double ox = -(i00 * dx + i01 * dy), oy = -(i01 * dx + i11 * dy);
        if (isfinite(ox) && isfinite(oy)) {
            fx = (float)((double)px + ox);
            fy = (float)((double)py + oy);
            if constexpr (HESS) {
                hess3[0] = dxx;
                hess3[1] = dxy;
                hess3[2] = dyy;
            }
        }
    }
}

// The end of get_final2's finish for one plane, one wave: bv / bm the plane's first raw maximum and its blurred maximum, bi
// the raw maximum's index (0 for an all -inf / all-NaN plane).  blurred(pt) is the f32 blurred value at final2 point pt; lanes
// 0..12 call it, and only when the step is taken.  peak() is the raw value at bi (lane 0).  Lane 0 writes kp[plane] (x, y,
// peak) and, when idx_out is not null, idx_out[plane] = bi.  HESS: lane 0 also writes hess[plane] = (dxx, dxy, dyy), f64, the
// Hessian of the blurred log heat-map that the step used, or NaN x 3 when no step is taken (border, det == 0, non-finite).
template <bool HESS = false, class Blurred, class Peak>
__device__ __forceinline__ void final2_finish(float bv, int bi, float bm, int H, int W, Blurred blurred, Peak peak, float* kp,
                                              int* idx_out, int plane, double* hess = nullptr) {
#pragma clang fp contract(off)
    const int px = bi % W, py = bi / W;
    // gaussian_blur's rescale factor origin_max / max(blurred), f32 (inference.py:110)
    const float s = (float)((double)bv / (double)bm);
    const bool go = 1 < px && px < W - 2 && 1 < py && py < H - 2 && isfinite(bv) && isfinite(bm) && isfinite(s);
    float lv = 0.f;                                        // lane j < 13: log of the rescaled, clamped blurred value at point j
    if (go && threadIdx.x < 13) {
        const int j = threadIdx.x;
        lv = final2_log(blurred(j), s);
    }
    float h[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) h[j] = __shfl(lv, j);
    if (threadIdx.x == 0) {
        float fx = (float)px, fy = (float)py;
        if constexpr (HESS) {
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            double hs[3] = {nan, nan, nan};
            if (go) final2_newton<true>(h, px, py, fx, fy, hs);
            double* h3 = hess + (size_t)plane * 3;
            h3[0] = hs[0];
            h3[1] = hs[1];
            h3[2] = hs[2];
        } else {
            if (go) final2_newton(h, px, py, fx, fy);
        }
        float* kp3 = kp + (size_t)plane * 3;
        kp3[0] = fx;
        kp3[1] = fy;
        kp3[2] = peak();
        if (idx_out) idx_out[plane] = bi;
    }
}

}  // namespace esa
