// correspond.hip — keypoints to the record the host pose solver consumes, on the device (val.py:172-180): the top-k rule, the
// heapq.nlargest order and the back-projection to image pixels, with the weight of the refinement beside each point.  The
// arithmetic is correspond.h's, the header pnp_host.hip uses for the same step; this whole file is compiled without
// contraction, as frontend.hip's box_kernel is (here by the file-scope pragma below, which also covers the header), so that
// product and sum of the back-projection round one by one, as the host's do.
//
// correspond_kernel: one wave per crop, lane j < K holds keypoint j (K <= 32).  No LDS and no barrier: the two counts are
// wave ballots, and the order is a rank-by-counting sort — every lane reads the K peaks lane by lane (a wave-uniform source
// lane each time) and counts the keypoints handed over before its own, which is its slot.  A lane writes its own slot when it is
// selected, and clears slot `lane` when that slot lies beyond count, so every element of the record is written exactly once,
// with plain per-lane (vector) stores.
#pragma clang fp contract(off)
#include "correspond.h"
#include "kernels.h"

namespace esa {
namespace {

__global__ __launch_bounds__(64) void correspond_kernel(const float* kp, const double* hess, const int* crop, const double* rates,
                                                        const int* valid, int K, double thresh, int min_k, int mode, int* count,
                                                        int* order, double* pts, double* w) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const bool have = lane < K, ok = valid[c] != 0;
    float x = 0.f, y = 0.f, peak = 0.f;
    if (have) {
        const float* r = kp + ((size_t)c * K + lane) * 3;
        x = r[0];
        y = r[1];
        peak = r[2];
    }
    const bool cand = ok && have && peak == peak;          // a NaN peak is never selected
    const int ncand = __popcll(__ballot(cand));
    const int above = __popcll(__ballot(cand && (double)peak > thresh));
    const int cnt = corr_count(above, min_k, ncand);
    int rank = 0;                                          // candidates handed over before this lane's keypoint
    for (int j = 0; j < K; ++j) {
        const float pj = __shfl(peak, j);
        const int cj = __shfl((int)cand, j);
        rank += cj && corr_before(pj, j, peak, lane);
    }
    int* ord = order + (size_t)c * K;
    double* p2 = pts + (size_t)c * K * 2;
    double* w3 = w + (size_t)c * K * 3;
    if (cand && rank < cnt) {
        const double inv = corr_inv_rate(rates[c]);
        ord[rank] = lane;
        p2[rank * 2 + 0] = corr_to_image(x, inv, crop[c * 4 + 0]);
        p2[rank * 2 + 1] = corr_to_image(y, inv, crop[c * 4 + 1]);
        double wv[3] = {(double)peak, 0.0, (double)peak};
        if (mode == 1) corr_hessian_weight(hess + ((size_t)c * K + lane) * 3, rates[c], wv);
        w3[rank * 3 + 0] = wv[0];
        w3[rank * 3 + 1] = wv[1];
        w3[rank * 3 + 2] = wv[2];
    }
    if (have && lane >= cnt) {                             // the slots beyond count
        ord[lane] = -1;
        p2[lane * 2 + 0] = 0.0;
        p2[lane * 2 + 1] = 0.0;
        w3[lane * 3 + 0] = 0.0;
        w3[lane * 3 + 1] = 0.0;
        w3[lane * 3 + 2] = 0.0;
    }
    if (lane == 0) count[c] = cnt;
}

}  // namespace

int launch_correspond(const float* kp, const double* hess, const int* crop, const double* rates, const int* valid, int m, int K,
                      double thresh, int min_k, int mode, int* count, int* order, double* pts, double* w, hipStream_t s) {
    if (!kp || !crop || !rates || !valid || !count || !order || !pts || !w || m <= 0 || K < 1 || K > 32 || (mode != 0 && mode != 1) ||
        (mode == 1 && !hess))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(correspond_kernel, dim3((unsigned)m), dim3(64), 0, s, kp, hess, crop, rates, valid, K, thresh, min_k, mode,
                       count, order, pts, w);
    return (int)hipGetLastError();
}

}  // namespace esa
