// correspond.h — keypoint rows -> the correspondences handed to the pose solver (val.py:172-180), the one statement of that
// arithmetic: the device stage (correspond.hip: correspond_kernel) and the host solver (pnp_host.hip: esahrnet_pnp_batch)
// both call these functions, so that a point selected and back-projected on the device has the bits the host gives it.
//
//   selection        k = max(#(peak > thresh), min_k), at most K; the k keypoints with the largest peaks, largest first, equal
//                    peaks by lower index (heapq.nlargest over range(K), val.py:172-177).
//   back-projection  ori = p * (1 / rate) + origin (val.py:180): the reciprocal once per crop, then one product and one sum per
//                    coordinate in f64, never contracted into an fma (the functions turn contraction off themselves; the
//                    device file does so at file scope besides).
//   weights          mode 0 "peak": (wxx, wxy, wyy) = (peak, 0, peak), the scalar weight of val.py:194-209.
//                    mode 1 "hessian": rate * (-H)^(1/2), H = (dxx, dxy, dyy) the Hessian of the blurred log heat-map that the
//                    get_final2 step used.  For a Gaussian blob -H is the information matrix of the keypoint in crop pixels;
//                    its symmetric square root W makes |W d|^2 the Mahalanobis distance, and d_crop = rate * d_img puts it in
//                    image pixels, where the residual of uncertainty_pnp.cpp:30-31 lives.  Closed form for A = [[a, b], [b, c]]
//                    positive definite: s = sqrt(det A), t = sqrt(a + c + 2 s), A^(1/2) = (A + s I) / t.
//
// Edge cases of the device stage (correspond_kernel):
//   * an invalid crop (valid == 0) has count 0: nothing of it reaches the solver, which answers fewer than 4 points with NaN;
//   * a NaN peak in a valid crop is never selected: NaN peaks rank behind every number and count is at most the number of
//     peaks that are numbers (the host sort of esahrnet_pnp_batch has no defined order for NaN: keep NaN rows away from it);
//   * mode 1: when -H is not positive definite (a <= 0 or det <= 0), H holds a NaN (no step was taken) or the weight is not
//     finite, w = (0, 0, 0): the point still reaches EPnP / RANSAC but carries no weight in the refinement.
#pragma once
#include <hip/hip_runtime.h>

namespace esa {

// keypoint a (peak pa) is handed over before keypoint b: the order of heapq.nlargest / a stable descending sort
__host__ __device__ inline bool corr_before(float pa, int a, float pb, int b) { return pa > pb || (pa == pb && a < b); }

// number of keypoints handed over: `above` of K peaks exceed the threshold
__host__ __device__ inline int corr_count(int above, int min_k, int K) {
    const int k = above > min_k ? above : min_k;
    return k < K ? k : K;
}

__host__ __device__ inline double corr_inv_rate(double rate) { return 1.0 / rate; }

// one coordinate of val.py:180: crop coordinate p -> image pixels
__host__ __device__ inline double corr_to_image(float p, double inv_rate, int origin) {
#pragma clang fp contract(off)
    const double scaled = (double)p * inv_rate;
    return scaled + (double)origin;
}

// mode 1: H = (dxx, dxy, dyy) -> w3 = rate * (-H)^(1/2) as (wxx, wxy, wyy), or zeros (see above)
__host__ __device__ inline void corr_hessian_weight(const double* H, double rate, double* w3) {
#pragma clang fp contract(off)
    const double a = -H[0], b = -H[1], c = -H[2];
    const double det = a * c - b * b;
    w3[0] = w3[1] = w3[2] = 0.0;
    if (!(a > 0.0 && det > 0.0)) return;                   // NaN fails both
    const double s = sqrt(det), t = sqrt((a + c) + 2.0 * s);
    const double wxx = rate * ((a + s) / t), wxy = rate * (b / t), wyy = rate * ((c + s) / t);
    if (!(wxx - wxx == 0.0 && wxy - wxy == 0.0 && wyy - wyy == 0.0)) return;      // inf or NaN
    w3[0] = wxx;
    w3[1] = wxy;
    w3[2] = wyy;
}

}  // namespace esa
