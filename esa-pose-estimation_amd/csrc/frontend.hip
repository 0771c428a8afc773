// frontend.hip — the loader on the device: detector boxes and camera frames to the network's crops, without a host
// round trip (DESIGN.md §8 NEXT-2).
//
//   box_kernel           the crop-box rule of ESAValDataSet.__getitem__ (data_load_val.py:127-158, rule 0) and of
//                        ESADataSet.__getitem__ (data_load4.py:112-141, rule 1: the same with the box forced square before
//                        the clamps), in Python's arithmetic: true division and k * size in f64, int() truncating toward
//                        zero.  This file is compiled with -ffp-contract=off (build.py PER_FILE_FLAGS) and the product is
//                        written as __dmul_rn besides: int(c0 - 1.05 * size) must see the rounded product.
//   crop_ex_kernel       crop_kernel of crops.hip (same 11-bit coefficients, same integer passes, same normalisation: bit-
//                        identical on gray frames with the identity index) with a frame index per crop, RGB8 frames reduced
//                        by PIL's convert('L') before the resize, and invalid crops written as zeros.
//   mark_invalid_kernel  keypoint rows of invalid crops become NaN (index -1) after the forward.
//   mark_invalid_refined_kernel  the same for the refined candidates' outputs: K * M rows per crop, f64 outputs and a status.
#include "kernels.h"

namespace esa {
namespace {

__device__ __forceinline__ int sat32(long long v) {
    return (int)(v < -2147483647LL - 1 ? -2147483647LL - 1 : (v > 2147483647LL ? 2147483647LL : v));
}

// one thread per box.  det: (x, y, x2, y2); crop: (x_new, y_new, w_new, h_new), (w_new, h_new) the far corner.
// frame_idx (may be null): a crop whose frame does not exist is invalid as well.
__global__ __launch_bounds__(256) void box_kernel(const int* det, const int* frame_idx, int nframes, int m, int FH, int FW,
                                                  int S, int rule, double k, int* crop, double* rates, int* valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const long long x = det[i * 4 + 0], y = det[i * 4 + 1], w = det[i * 4 + 2], h = det[i * 4 + 3];
    // int(a / 2) of Python ints: the quotient is exact in f64 (|a| < 2^33), the conversion truncates toward zero
    const long long c0 = (long long)((double)(x + w) / 2.0);
    const long long c1 = (long long)((double)(y + h) / 2.0);
    const long long dw = w - x, dh = h - y;
    const long long size = (long long)((double)(dw > dh ? dw : dh) / 2.0);
    const double ks = __dmul_rn(k, (double)size);
    long long x_new = (long long)__dsub_rn((double)c0, ks), y_new = (long long)__dsub_rn((double)c1, ks);
    long long w_new = (long long)__dadd_rn((double)c0, ks), h_new = (long long)__dadd_rn((double)c1, ks);
    if (rule == 1 && (w_new - x_new) != (h_new - y_new)) h_new = y_new + (w_new - x_new);       // data_load4.py:120-121
    if (x_new < 0) { w_new -= x_new; x_new = 0; }
    if (y_new < 0) { h_new -= y_new; y_new = 0; }
    if (w_new > FW) {
        x_new = x_new + FW - w_new;
        if (x_new < 0) x_new = 0;
        w_new = FW;
    }
    if (h_new > FH) {
        y_new = y_new + FH - h_new;
        if (y_new < 0) y_new = 0;
        h_new = FH;
    }
    const long long xs = w_new - x_new, ys = h_new - y_new, sz = xs > ys ? xs : ys;
    // a corner outside int32 only happens for an empty box (after the clamps 0 <= x_new, w_new <= FW): stored saturated
    crop[i * 4 + 0] = sat32(x_new);
    crop[i * 4 + 1] = sat32(y_new);
    crop[i * 4 + 2] = sat32(w_new);
    crop[i * 4 + 3] = sat32(h_new);
    rates[i] = sz == S ? 1.0 : (double)S / (double)sz;
    bool ok = xs > 0 && ys > 0;
    if (frame_idx) ok = ok && frame_idx[i] >= 0 && frame_idx[i] < nframes;
    valid[i] = ok ? 1 : 0;
}

// crops.hip's coef(): OpenCV's 8-bit INTER_LINEAR source index and 11-bit coefficient pair of destination index d
__device__ __forceinline__ void coef(int d, int src, int dst, int& s0, int& s1, int& a0, int& a1) {
    const double scale = (double)src / (double)dst;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    s0 = s;
    s1 = min(s + 1, src - 1);
    a0 = (int)rintf((1.f - f) * 2048.f);     // saturate_cast<short>: round to nearest even
    a1 = (int)rintf(f * 2048.f);
}

// one block per 256 pixels of one output row: crop index and row (blockIdx.x) are uniform, so the row's coefficients are
// the same in every lane.  RGB: 0 = gray8 [nframes][FH][FW], 1 = RGB8 interleaved [nframes][FH][FW][3].
template <int RGB>
__global__ __launch_bounds__(256) void crop_ex_kernel(const unsigned char* frames, int nframes, const int* frame_idx,
                                                      const int* boxes, const int* valid, float* out, int m, int FH, int FW,
                                                      int S, float mean, float std_) {
    const int dx = blockIdx.y * 256 + threadIdx.x;
    if (dx >= S) return;
    const int n = blockIdx.x / S, dy = blockIdx.x - n * S;
    float* o = out + ((size_t)n * S + dy) * S + dx;
    const int fi = frame_idx ? frame_idx[n] : n;
    const int x0 = boxes[n * 4 + 0], y0 = boxes[n * 4 + 1], x1 = boxes[n * 4 + 2], y1 = boxes[n * 4 + 3];
    // the subtractions below must not overflow: a box that the rule produced lies inside the frame
    const bool sane = x0 >= 0 && y0 >= 0 && x1 > x0 && y1 > y0 && x1 <= FW && y1 <= FH;
    if (fi < 0 || fi >= nframes || (valid && !valid[n]) || !sane) {
        *o = 0.f;
        return;
    }
    const int xs = x1 - x0, ys = y1 - y0, size = max(xs, ys);
    const int rows = ys + (size - xs), cols = xs + (size - ys);       // reference's swapped pad amounts
    int sx0, sx1, ax0, ax1, sy0, sy1, by0, by1;
    coef(dx, cols, S, sx0, sx1, ax0, ax1);
    coef(dy, rows, S, sy0, sy1, by0, by1);
    const unsigned char* f = frames + (size_t)fi * FH * FW * (RGB ? 3 : 1);
    auto px = [&](int r, int c) {
        const int yy = min(max(y0 + min(r, ys - 1), 0), FH - 1), xx = min(max(x0 + min(c, xs - 1), 0), FW - 1);
        const size_t at = (size_t)yy * FW + xx;
        if (!RGB) return (int)f[at];
        // PIL's convert('L'): ITU-R 601-2 luma in 16-bit fixed point, rounded
        return ((int)f[at * 3] * 19595 + (int)f[at * 3 + 1] * 38470 + (int)f[at * 3 + 2] * 7471 + 0x8000) >> 16;
    };
    const int r0 = px(sy0, sx0) * ax0 + px(sy0, sx1) * ax1;
    const int r1 = px(sy1, sx0) * ax0 + px(sy1, sx1) * ax1;
    int v = (((by0 * (r0 >> 4)) >> 16) + ((by1 * (r1 >> 4)) >> 16) + 2) >> 2;
    v = min(max(v, 0), 255);
    *o = ((float)v / 255.f - mean) / std_;
}

// one thread per (crop, keypoint)
__global__ __launch_bounds__(256) void mark_invalid_kernel(const int* valid, int m, int K, float* kp, int* idx) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m * K) return;
    if (valid[t / K]) return;
    const float nan = __int_as_float(0x7fc00000);
    kp[(size_t)t * 3 + 0] = nan;
    kp[(size_t)t * 3 + 1] = nan;
    kp[(size_t)t * 3 + 2] = nan;
    if (idx) idx[t] = -1;
}

// mark_invalid_kernel for esahrnet_frames_keypoints_gaussfit: the decoder's other outputs too
__global__ __launch_bounds__(256) void mark_invalid_gaussfit_kernel(const int* valid, int m, int K, float* kp, int* idx, double* fit,
                                                                    int* status, double* hess) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m * K) return;
    if (valid[t / K]) return;
    const float nan = __int_as_float(0x7fc00000);
    const double dnan = __longlong_as_double(0x7ff8000000000000LL);
    kp[(size_t)t * 3 + 0] = nan;
    kp[(size_t)t * 3 + 1] = nan;
    kp[(size_t)t * 3 + 2] = nan;
    if (idx) idx[t] = -1;
    if (fit)
        for (int i = 0; i < 8; ++i) fit[(size_t)t * 8 + i] = dnan;
    if (hess)
        for (int i = 0; i < 3; ++i) hess[(size_t)t * 3 + i] = dnan;
    status[t] = -1;
}

// mark_invalid_gaussfit_kernel for esahrnet_frames_keypoints_gaussfit_cov: cov and info too
__global__ __launch_bounds__(256) void mark_invalid_gfcov_kernel(const int* valid, int m, int K, float* kp, int* idx, double* fit,
                                                                 int* status, double* hess, double* cov, double* info) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m * K) return;
    if (valid[t / K]) return;
    const float nan = __int_as_float(0x7fc00000);
    const double dnan = __longlong_as_double(0x7ff8000000000000LL);
    kp[(size_t)t * 3 + 0] = nan;
    kp[(size_t)t * 3 + 1] = nan;
    kp[(size_t)t * 3 + 2] = nan;
    if (idx) idx[t] = -1;
    if (fit)
        for (int i = 0; i < 8; ++i) fit[(size_t)t * 8 + i] = dnan;
    if (hess)
        for (int i = 0; i < 3; ++i) hess[(size_t)t * 3 + i] = dnan;
    if (cov)
        for (int i = 0; i < 3; ++i) cov[(size_t)t * 3 + i] = dnan;
    if (info)
        for (int i = 0; i < 3; ++i) info[(size_t)t * 3 + i] = dnan;
    status[t] = -1;
}

// for esahrnet_frames_keypoints_candidates_refined: one thread per (crop, slot), slots = K * M candidate rows per crop; every
// output but cand is optional
__global__ __launch_bounds__(256) void mark_invalid_refined_kernel(const int* valid, int m, int slots, float* cand, int* cidx,
                                                                   int* status, double* hess, double* fit, double* cov,
                                                                   double* info) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m * slots) return;
    if (valid[t / slots]) return;
    const float nan = __int_as_float(0x7fc00000);
    const double dnan = __longlong_as_double(0x7ff8000000000000LL);
    cand[(size_t)t * 3 + 0] = nan;
    cand[(size_t)t * 3 + 1] = nan;
    cand[(size_t)t * 3 + 2] = nan;
    if (cidx) cidx[t] = -1;
    if (status) status[t] = -1;
    if (fit)
        for (int i = 0; i < 8; ++i) fit[(size_t)t * 8 + i] = dnan;
    if (hess)
        for (int i = 0; i < 3; ++i) hess[(size_t)t * 3 + i] = dnan;
    if (cov)
        for (int i = 0; i < 3; ++i) cov[(size_t)t * 3 + i] = dnan;
    if (info)
        for (int i = 0; i < 3; ++i) info[(size_t)t * 3 + i] = dnan;
}

}  // namespace

int launch_boxes(const int* det, const int* frame_idx, int nframes, int m, int FH, int FW, int S, int rule, int* crop,
                 double* rates, int* valid, hipStream_t s) {
    if (m <= 0 || FH <= 0 || FW <= 0 || S <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(box_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, det, frame_idx, nframes, m, FH, FW, S,
                       rule, 1.05, crop, rates, valid);
    return (int)hipGetLastError();
}

int launch_crops_ex(const unsigned char* frames, int nframes, int FH, int FW, int rgb, const int* frame_idx, const int* boxes,
                    const int* valid, float* out, int m, int S, float mean, float std_, hipStream_t s) {
    if (m <= 0 || nframes <= 0 || FH <= 0 || FW <= 0 || S <= 0 || (long long)m * S > 0xffffffLL) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)(m * S), (unsigned)((S + 255) / 256));
    if (rgb)
        hipLaunchKernelGGL(crop_ex_kernel<1>, grid, dim3(256), 0, s, frames, nframes, frame_idx, boxes, valid, out, m, FH, FW, S,
                           mean, std_);
    else
        hipLaunchKernelGGL(crop_ex_kernel<0>, grid, dim3(256), 0, s, frames, nframes, frame_idx, boxes, valid, out, m, FH, FW, S,
                           mean, std_);
    return (int)hipGetLastError();
}

int launch_mark_invalid(const int* valid, int m, int K, float* kp, int* idx, hipStream_t s) {
    if (m <= 0 || K <= 0 || (long long)m * K > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mark_invalid_kernel, dim3((unsigned)(((long long)m * K + 255) / 256)), dim3(256), 0, s, valid, m, K, kp,
                       idx);
    return (int)hipGetLastError();
}

int launch_mark_invalid_gaussfit(const int* valid, int m, int K, float* kp, int* idx, double* fit, int* status, double* hess,
                                 hipStream_t s) {
    if (m <= 0 || K <= 0 || (long long)m * K > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mark_invalid_gaussfit_kernel, dim3((unsigned)(((long long)m * K + 255) / 256)), dim3(256), 0, s, valid, m, K,
                       kp, idx, fit, status, hess);
    return (int)hipGetLastError();
}

int launch_mark_invalid_gaussfit_cov(const int* valid, int m, int K, float* kp, int* idx, double* fit, int* status, double* hess,
                                     double* cov, double* info, hipStream_t s) {
    if (!cov && !info) return launch_mark_invalid_gaussfit(valid, m, K, kp, idx, fit, status, hess, s);
    if (m <= 0 || K <= 0 || (long long)m * K > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mark_invalid_gfcov_kernel, dim3((unsigned)(((long long)m * K + 255) / 256)), dim3(256), 0, s, valid, m, K, kp,
                       idx, fit, status, hess, cov, info);
    return (int)hipGetLastError();
}

int launch_mark_invalid_refined(const int* valid, int m, int slots, float* cand, int* cidx, int* status, double* hess, double* fit,
                                double* cov, double* info, hipStream_t s) {
    if (m <= 0 || slots <= 0 || (long long)m * slots > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mark_invalid_refined_kernel, dim3((unsigned)(((long long)m * slots + 255) / 256)), dim3(256), 0, s, valid, m,
                       slots, cand, cidx, status, hess, fit, cov, info);
    return (int)hipGetLastError();
}

}  // namespace esa
