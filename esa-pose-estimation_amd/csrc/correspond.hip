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
//
// correspond_cand_kernel: the same stage on candidate rows (esahrnet_correspondences_cand): the selection by candidate 0, then
// every candidate of a selected keypoint in image pixels with its own weight and peak, the record
// esahrnet_pnp_batch_cand_pts solves on.  Described at the kernel.
#pragma clang fp contract(off)
#include "correspond.h"
#include "kernels.h"

#include "../../include/esahrnet.h"

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

// one slot of the candidate record: candidate mm of keypoint `row` (null: a slot beyond count, zeros) into rank slot `slot`
__device__ inline void cand_slot(const float* row, const double* hrow, int mm, int slot, int M, double inv, double rate, int x0,
                                 int y0, int mode, double* cpts, double* cw, float* cpeak) {
    double px = 0.0, py = 0.0, wv[3] = {0.0, 0.0, 0.0};
    float pk = 0.f;
    if (row) {
        const float x = row[mm * 3 + 0], y = row[mm * 3 + 1];
        pk = row[mm * 3 + 2];
        if (x - x == 0.f && y - y == 0.f) {                // both coordinates finite
            px = corr_to_image(x, inv, x0);
            py = corr_to_image(y, inv, y0);
            if (mode == 1) corr_hessian_weight(hrow + mm * 3, rate, wv);
            else wv[0] = wv[2] = (double)pk;
        } else {                                           // an absent runner-up's NaN row among them: no point, no weight
            px = py = __builtin_nan("");
        }
    }
    const size_t s = (size_t)slot * M + mm;
    cpts[s * 2 + 0] = px;
    cpts[s * 2 + 1] = py;
    cw[s * 3 + 0] = wv[0];
    cw[s * 3 + 1] = wv[1];
    cw[s * 3 + 2] = wv[2];
    cpeak[s] = pk;
}

// correspond_cand_kernel: correspond_kernel's selection on the candidate-0 rows of cand [m][K][M][3], then every candidate of a
// selected keypoint back-projected and weighed into the keypoint's rank slot.  One wave per crop, no LDS, no barrier.  K <= 32, so
// both halves of the wave hold the keypoints: lane j and lane j + 32 read keypoint j's primary peak and count the same rank (the
// ballots look at the lower half only); the lower half then writes the even candidates of its keypoint, the upper half the odd
// ones, at most two each.  As in correspond_kernel a lane writes rank slot `rank` when its keypoint is selected and clears slot j
// when j lies beyond count: the selected ranks are exactly 0 .. count - 1 and the cleared slots count .. K - 1, each (slot, mm)
// belongs to one half, so every element of cpts, cw and cpeak is written exactly once; order by the lower half, count by lane 0.
__global__ __launch_bounds__(64) void correspond_cand_kernel(const float* cand, const double* hess, const int* crop,
                                                             const double* rates, const int* valid, int K, int M, double thresh,
                                                             int min_k, int mode, int* count, int* order, double* cpts, double* cw,
                                                             float* cpeak) {
    const int c = blockIdx.x, lane = threadIdx.x, j = lane & 31, half = lane >> 5;
    const bool have = j < K, ok = valid[c] != 0;
    const float* row = cand + ((size_t)c * K + (have ? j : 0)) * M * 3;
    const float peak = have ? row[2] : 0.f;
    const bool sel = ok && have && peak == peak;           // a NaN primary peak is never selected
    const int ncand = __popcll(__ballot(sel && half == 0));
    const int above = __popcll(__ballot(sel && half == 0 && (double)peak > thresh));
    const int cnt = corr_count(above, min_k, ncand);
    int rank = 0;                                          // keypoints handed over before this lane's
    for (int i = 0; i < K; ++i) {
        const float pi = __shfl(peak, i);
        const int si = __shfl((int)sel, i);
        rank += si && corr_before(pi, i, peak, j);
    }
    int* ord = order + (size_t)c * K;
    double* p2 = cpts + (size_t)c * K * M * 2;
    double* w3 = cw + (size_t)c * K * M * 3;
    float* pk = cpeak + (size_t)c * K * M;
    if (sel && rank < cnt) {
        const double rate = rates[c], inv = corr_inv_rate(rate);
        const int x0 = crop[c * 4 + 0], y0 = crop[c * 4 + 1];
        const double* hrow = mode == 1 ? hess + ((size_t)c * K + j) * M * 3 : nullptr;
        if (half == 0) ord[rank] = j;
        for (int mm = half; mm < M; mm += 2) cand_slot(row, hrow, mm, rank, M, inv, rate, x0, y0, mode, p2, w3, pk);
    }
    if (have && j >= cnt) {                                // the slots beyond count
        if (half == 0) ord[j] = -1;
        for (int mm = half; mm < M; mm += 2) cand_slot(nullptr, nullptr, mm, j, M, 0.0, 0.0, 0, 0, 0, p2, w3, pk);
    }
    if (lane == 0) count[c] = cnt;
}

}  // namespace

int launch_correspond_cand(const float* cand, const double* hess, const int* crop, const double* rates, const int* valid, int m, int K,
                           int M, double thresh, int min_k, int mode, int* count, int* order, double* cpts, double* cw, float* cpeak,
                           hipStream_t s) {
    if (!cand || !crop || !rates || !valid || !count || !order || !cpts || !cw || !cpeak || m <= 0 || K < 1 || K > 32 || M < 1 ||
        M > ESAHRNET_MAX_CANDIDATES || (mode != 0 && mode != 1) || (mode == 1 && !hess))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(correspond_cand_kernel, dim3((unsigned)m), dim3(64), 0, s, cand, hess, crop, rates, valid, K, M, thresh, min_k,
                       mode, count, order, cpts, cw, cpeak);
    return (int)hipGetLastError();
}

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
