// keypoints_candidates.hip — the M best peaks of every heat-map:  f32 [planes][H][W] -> f32 [planes][M][3], int32 [planes][M].
//
// Every other decoder here returns one point per plane, the global arg-max; when that maximum sits on the wrong blob (a
// symmetric part of the spacecraft, an Earth-limb artefact) the right blob is almost always the second-highest local maximum,
// and this kernel keeps it: the pose solve can then swap it in where the consensus pose says the primary is wrong
// (pnp_host.hip: esahrnet_pnp_batch_cand).
//
//   candidate 0      the row of keypoints.hip's keypoints_kernel, bit for bit: the same sweep (argmax_take: first row-major
//                    maximum, NaN counts as the maximum, all-NaN / all -inf planes give index 0) and the same refine_keypoint.
//   candidate m >= 1 the largest value among the pixels that (a) are neither NaN nor -inf, (b) are local maxima — at least as
//                    large as each of their up to 8 neighbours inside the plane; a NaN neighbour disqualifies — and (c) lie at
//                    Chebyshev distance > r from every candidate 0..m-1; ties go to the lower flat index.  Refined by the same
//                    refine_keypoint at its own pixel, peak = the raw value there.  When no pixel qualifies, that row and all
//                    later ones are NaN x 3 with index -1.
//
// One workgroup (16 waves) per plane, as in keypoints_kernel, and the M sweeps of a plane inside one launch: the first sweep
// brings the plane into L2 (a 256 x 256 plane is 256 KB), the later ones are served from there.  A lane keeps the best
// QUALIFYING (value, index) of its pixels.  A runner-up sweep comes in two forms:
//   rows      (the plane 16-B aligned, W a multiple of 4: every real heat-map) each lane takes a float4 and the float4s above
//             and below it in one go; the columns left and right of it come from the neighbouring lanes' registers (a lane at
//             the end of a wave, when its row goes on, loads those three values itself).  (b) is eight comparisons per pixel on
//             registers, for every pixel, without a branch: the cost does not depend on what the plane holds — a smooth map, in
//             which hardly any pixel is a local maximum and a lane's best therefore stays empty, costs what a noisy one costs.
//   pixels    (any other plane) pixel by pixel; (c) and (b) only for a pixel that would replace the lane's best — a pixel that
//             does not qualify never replaces it —, the eight neighbours loaded together (out-of-plane coordinates clamped onto
//             the pixel's own row or column, where they name a real neighbour or the pixel itself: harmless duplicates).
// No workspace, no allocation, no synchronisation with the host; a plane's result depends on its own pixels alone.
#include "kernels.h"
#include "refine.h"

#include "../../include/esahrnet.h"

namespace esa {
namespace {

constexpr int KT = 1024;        // 16 waves per plane (keypoints.hip: the sweep is latency-bound, it wants loads in flight)
constexpr int KW = KT / 64;

// the lanes' (bv, bi) -> the workgroup's, in every thread: a 64-lane shuffle reduction, one LDS slot per wave (sv / si: this
// sweep's own KW slots, so that one barrier per sweep is enough), then every thread folds the KW slots itself
__device__ __forceinline__ void reduce_block(float& bv, int& bi, float* sv, int* si) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        argmax_take(ov, oi, bv, bi);
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    bv = sv[0];
    bi = si[0];
    for (int w = 1; w < KW; ++w) argmax_take(sv[w], si[w], bv, bi);
}

__global__ __launch_bounds__(KT) void keypoints_candidates_kernel(const float* heat, int H, int W, int M, int r, float* cand,
                                                                  int* cidx) {
    __shared__ float sv[ESAHRNET_MAX_CANDIDATES][KW];
    __shared__ int si[ESAHRNET_MAX_CANDIDATES][KW];
    const float* pl = heat + (size_t)blockIdx.x * H * W;
    const int total = H * W;
    float* row = cand + (size_t)blockIdx.x * M * 3;
    int* irow = cidx ? cidx + (size_t)blockIdx.x * M : nullptr;

    // ---- candidate 0: keypoints_kernel ----------------------------------------------------------------------------------
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    const int nvec = total >> 2;
    const bool aligned = ((reinterpret_cast<uintptr_t>(pl) & 15) == 0);
    if (aligned) {                                          // (keypoints_kernel's loops, statement for statement)
        for (int v4 = threadIdx.x; v4 < nvec; v4 += KT) {
            const float4 q = reinterpret_cast<const float4*>(pl)[v4];
            argmax_take(q.x, v4 * 4 + 0, bv, bi);
            argmax_take(q.y, v4 * 4 + 1, bv, bi);
            argmax_take(q.z, v4 * 4 + 2, bv, bi);
            argmax_take(q.w, v4 * 4 + 3, bv, bi);
        }
        for (int i = nvec * 4 + threadIdx.x; i < total; i += KT) argmax_take(pl[i], i, bv, bi);
    } else {
        for (int i = threadIdx.x; i < total; i += KT) argmax_take(pl[i], i, bv, bi);
    }
    reduce_block(bv, bi, sv[0], si[0]);
    if (threadIdx.x == 0)
        refine_keypoint([=](int yy, int xx) { return pl[yy * W + xx]; }, H, W, bi, row, irow);
    if (bi == 0x7fffffff) bi = 0;                          // all-NaN / all -inf plane: refine_keypoint reports pixel 0
    int cx[ESAHRNET_MAX_CANDIDATES], cy[ESAHRNET_MAX_CANDIDATES];      // (m is a compile-time index below: registers)
    cx[0] = bi % W;
    cy[0] = bi / W;

    // ---- candidates 1 .. M-1 --------------------------------------------------------------------------------------------
    const bool rows = aligned && (W & 3) == 0;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int m = 1; m < ESAHRNET_MAX_CANDIDATES; ++m) {
        if (m >= M) break;                                  // uniform over the workgroup
        bv = -INFINITY;
        bi = 0x7fffffff;
        // (v, i) at (x, y), known to meet (b) when it is not NaN: (a), (c), and better than the lane's best?  NaN and -inf
        // fail v > bv (bv starts at -inf and never is NaN)
        auto offer = [&](float v, int i, int x, int y) {
            if (!(v > bv || (v == bv && i < bi)) || v == -INFINITY) return;
#pragma unroll
            for (int j = 0; j < m; ++j) {
                const int dx = abs(x - cx[j]), dy = abs(y - cy[j]);
                if ((dx > dy ? dx : dy) <= r) return;
            }
            bv = v;
            bi = i;
        };
        if (rows) {
            const float4* p4 = reinterpret_cast<const float4*>(pl);
            const int wv = W >> 2;
            for (int base = 0; base < nvec; base += KT) {   // uniform trip count: the shuffles below see every lane
                const bool live = base + (int)threadIdx.x < nvec;
                const int v4 = live ? base + (int)threadIdx.x : nvec - 1;     // (an idle lane re-reads the last float4)
                const int y = v4 / wv, xv = v4 - y * wv, x = xv * 4;
                const int up = y > 0 ? v4 - wv : v4, dn = y < H - 1 ? v4 + wv : v4;     // no row there: its own, duplicates
                const float4 c = p4[v4], u = p4[up], d = p4[dn];
                float lu = __shfl_up(u.w, 1), lc = __shfl_up(c.w, 1), ld = __shfl_up(d.w, 1);
                float ru = __shfl_down(u.x, 1), rc = __shfl_down(c.x, 1), rd = __shfl_down(d.x, 1);
                if (xv == 0) lu = lc = ld = -INFINITY;       // no column there
                else if (lane == 0) { lu = pl[up * 4 - 1]; lc = pl[v4 * 4 - 1]; ld = pl[dn * 4 - 1]; }
                if (xv == wv - 1) ru = rc = rd = -INFINITY;
                else if (lane == 63) { ru = pl[up * 4 + 4]; rc = pl[v4 * 4 + 4]; rd = pl[dn * 4 + 4]; }
                // v >= each of the eight: a NaN among them, or in v, gives false
                auto peak = [](float v, float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
                    return (v >= a0) & (v >= a1) & (v >= a2) & (v >= a3) & (v >= a4) & (v >= a5) & (v >= a6) & (v >= a7);
                };
                if (live & peak(c.x, lc, c.y, lu, u.x, u.y, ld, d.x, d.y)) offer(c.x, v4 * 4 + 0, x + 0, y);
                if (live & peak(c.y, c.x, c.z, u.x, u.y, u.z, d.x, d.y, d.z)) offer(c.y, v4 * 4 + 1, x + 1, y);
                if (live & peak(c.z, c.y, c.w, u.y, u.z, u.w, d.y, d.z, d.w)) offer(c.z, v4 * 4 + 2, x + 2, y);
                if (live & peak(c.w, c.z, rc, u.z, u.w, ru, d.z, d.w, rd)) offer(c.w, v4 * 4 + 3, x + 3, y);
            }
        } else {
            for (int i = threadIdx.x; i < total; i += KT) {
                const float v = pl[i];
                if (!(v > bv)) continue;                    // (i grows along a lane's pixels: an equal value never replaces)
                const int x = i % W, y = i / W;
                const int y0 = (y > 0 ? y - 1 : y) * W, y1 = (y < H - 1 ? y + 1 : y) * W, yc = y * W;
                const int x0 = x > 0 ? x - 1 : x, x1 = x < W - 1 ? x + 1 : x;
                const float a0 = pl[y0 + x0], a1 = pl[y0 + x], a2 = pl[y0 + x1], a3 = pl[yc + x0], a4 = pl[yc + x1],
                            a5 = pl[y1 + x0], a6 = pl[y1 + x], a7 = pl[y1 + x1];
                if ((v >= a0) & (v >= a1) & (v >= a2) & (v >= a3) & (v >= a4) & (v >= a5) & (v >= a6) & (v >= a7)) offer(v, i, x, y);
            }
        }
        reduce_block(bv, bi, sv[m], si[m]);
        if (bi == 0x7fffffff) {                             // no pixel qualifies (uniform): this row and the later ones
            if (threadIdx.x == 0)
                for (int mm = m; mm < M; ++mm) {
                    row[mm * 3 + 0] = row[mm * 3 + 1] = row[mm * 3 + 2] = __int_as_float(0x7fc00000);
                    if (irow) irow[mm] = -1;
                }
            break;
        }
        if (threadIdx.x == 0)
            refine_keypoint([=](int yy, int xx) { return pl[yy * W + xx]; }, H, W, bi, row + m * 3, irow ? irow + m : nullptr);
        cx[m] = bi % W;
        cy[m] = bi / W;
    }
}

}  // namespace

int launch_keypoints_candidates(const float* heat, int planes, int H, int W, int M, int r, float* cand, int* cidx,
                                hipStream_t stream) {
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || M < 1 || M > ESAHRNET_MAX_CANDIDATES || r < 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(keypoints_candidates_kernel, dim3((unsigned)planes), dim3(KT), 0, stream, heat, H, W, M, r, cand, cidx);
    return (int)hipGetLastError();
}

}  // namespace esa

extern "C" int esahrnet_keypoints_candidates(const void* heat_dev, int n, int k, int height, int width, int candidates,
                                             int nms_radius, void* cand_dev, void* cidx_dev, esahrnet_stream stream) {
    if (!heat_dev || !cand_dev) return esa::set_error("keypoints_candidates: null argument");
    if (n <= 0 || k <= 0 || height <= 0 || width <= 0 || (long long)height * width > 0x7fffffffLL ||
        (long long)n * k > 0x7fffffffLL)
        return esa::set_error("keypoints_candidates: bad shape %d x %d x %d x %d", n, k, height, width);
    if (candidates < 1 || candidates > ESAHRNET_MAX_CANDIDATES)
        return esa::set_error("keypoints_candidates: %d candidates per heat-map unsupported (1..%d)", candidates,
                              ESAHRNET_MAX_CANDIDATES);
    if (nms_radius < 0) return esa::set_error("keypoints_candidates: negative nms_radius %d", nms_radius);
    if ((reinterpret_cast<uintptr_t>(heat_dev) | reinterpret_cast<uintptr_t>(cand_dev) | reinterpret_cast<uintptr_t>(cidx_dev)) & 3)
        return esa::set_error("keypoints_candidates: heat_dev, cand_dev and cidx_dev must be 4-byte aligned");
    const int rc = esa::launch_keypoints_candidates(static_cast<const float*>(heat_dev), n * k, height, width, candidates,
                                                    nms_radius, static_cast<float*>(cand_dev), static_cast<int*>(cidx_dev),
                                                    static_cast<hipStream_t>(stream));
    if (rc) return esa::set_error("keypoints_candidates: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}
