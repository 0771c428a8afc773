// keypoints_candidates_onepass.hip — the contract of keypoints_candidates.hip (candidate 0 the row of keypoints_kernel, candidate
// m >= 1 the best local maximum at Chebyshev distance > r from every earlier one, ties to the lower index, NaN x 3 / -1 from the
// first row without a qualifying pixel), bit for bit, with ONE sweep of the plane instead of M.
//
// The greedy rule does not need a sweep per runner-up.  Whether a pixel is a qualifying local maximum ((a) and (b) of
// keypoints_candidates.hip) does not depend on the candidates chosen so far; only (c), the suppression squares, does, and a new
// square changes the answer for the pixels inside it alone.  So:
//   pass 1      one sweep.  A wave owns a strip of 8 rows x 256 columns, a lane one float4 column of it: it loads the rows
//               y0 - 1 .. y0 + 8 (ten float4 loads for eight rows, 1.25 per float4 where the multi-sweep kernel makes 3) into a
//               window of three rows that rolls down the strip, takes
//               the side columns from its neighbours' registers (the first and last lane of a wave, when the row goes on, load
//               them themselves), feeds every pixel to argmax_take for candidate 0 and evaluates the eight-comparison test on
//               registers.  The best qualifying pixel of a lane's 8 x 4 pixels and that of the lane beside it make the entry of
//               one 8 x 8 cell in an LDS table, (value, flat index), empty = (-inf, 0x7fffffff): one writer per entry.
//   m >= 1      the cells that the square of candidate m - 1 touches are scanned again, one wave per cell, lane = pixel, now
//               with (c) against ALL squares so far (the 8 neighbours come from memory: L2-warm, at most (2r + 8)^2 pixels);
//               the wave's reduction rewrites the entry.  Then all threads reduce the table by (larger value, lower index).
// Exact: the arg-max of a total order does not depend on how the pixels are grouped, and after a rescan an entry is by
// construction the best unsuppressed qualifying pixel of its cell; an entry no new square touches stays that.
//
// Eligible planes: heat 16-byte aligned, W a multiple of 4 (the "rows" condition of the multi-sweep kernel) and at most
// kOnepassMaxCells cells (4096 = 32 KB of LDS: 512 x 512).  No workspace, no allocation, no synchronisation with the host; a
// plane's result depends on its own pixels alone.
#include "kernels.h"
#include "refine.h"

#include "../../include/esahrnet.h"

namespace esa {
namespace {

constexpr int KT = 1024;        // 16 waves per plane, as keypoints_candidates_kernel
constexpr int KW = KT / 64;
constexpr int CELL = 8;
constexpr int EMPTY = 0x7fffffff;

// keypoints_candidates.hip's reduce_block: the lanes' (bv, bi) -> the workgroup's, in every thread
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

// (v, i), a qualifying pixel (neither NaN nor -inf), against the best so far: larger value, then lower index
__device__ __forceinline__ void better(float v, int i, float& bv, int& bi) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// v >= each of the eight: a NaN among them, or in v, gives false
__device__ __forceinline__ bool peak8(float v, float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
    return (v >= a0) & (v >= a1) & (v >= a2) & (v >= a3) & (v >= a4) & (v >= a5) & (v >= a6) & (v >= a7);
}

__global__ __launch_bounds__(KT) void keypoints_candidates_onepass_kernel(const float* heat, int H, int W, int M, int r,
                                                                          float* cand, int* cidx) {
    __shared__ float tv[kOnepassMaxCells];
    __shared__ int ti[kOnepassMaxCells];
    __shared__ float sv[ESAHRNET_MAX_CANDIDATES][KW];
    __shared__ int si[ESAHRNET_MAX_CANDIDATES][KW];
    const float* pl = heat + (size_t)blockIdx.x * H * W;
    const float4* p4 = reinterpret_cast<const float4*>(pl);
    float* row = cand + (size_t)blockIdx.x * M * 3;
    int* irow = cidx ? cidx + (size_t)blockIdx.x * M : nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wv = W >> 2;                                  // float4s per row
    const int cw = (W + CELL - 1) / CELL, ch = (H + CELL - 1) / CELL, ncells = cw * ch;
    const float ninf = -INFINITY;

    // ---- pass 1: candidate 0 and the table ------------------------------------------------------------------------------
    float bv = ninf;
    int bi = EMPTY;
    const int nsx = (wv + 63) >> 6;                         // strips side by side: 64 float4 columns each
    for (int s = wave; s < ch * nsx; s += KW) {             // uniform over the wave: the shuffles below see every lane
        const int sy = s / nsx, sx = s - sy * nsx;
        const int y0 = sy * CELL, xv = sx * 64 + lane;
        const bool live = xv < wv;
        const bool first = xv == 0, last = xv == wv - 1;
        // A window of three rows rolls down the strip, the next row already under way: a row is q, the lane's float4, and the
        // columns left and right of it (l, r); -inf where the plane ends.  load() issues a row's loads (the first and last lane of
        // a wave, when the row goes on, load their side column themselves); side() completes it from the neighbours' registers
        struct Row { float4 q; float l, r; };
        auto load = [&](int y) {
            Row w{make_float4(ninf, ninf, ninf, ninf), ninf, ninf};
            if (y >= 0 && y < H && live) {                  // (the row test is uniform)
                const int v4 = y * wv + xv;
                w.q = p4[v4];
                if (lane == 0 && !first) w.l = pl[v4 * 4 - 1];
                if (lane == 63 && !last) w.r = pl[v4 * 4 + 4];
            }
            return w;
        };
        auto side = [&](Row& w) {
            const float sl = __shfl_up(w.q.w, 1), sr = __shfl_down(w.q.x, 1);
            w.l = first ? ninf : lane == 0 ? w.l : sl;
            w.r = last ? ninf : lane == 63 ? w.r : sr;
        };
        Row u = load(y0 - 1), c = load(y0), next = load(y0 + 1);
        side(u);
        side(c);
        float lv = ninf;                                    // the best qualifying pixel of this lane's 8 x 4
        int li = EMPTY;
#pragma unroll 1
        for (int j = 0; j < CELL; ++j) {
            Row d = next;
            if (j < CELL - 1) next = load(y0 + j + 2);
            side(d);
            const int y = y0 + j;
            const bool on = live && y < H;
            const int i0 = y * W + xv * 4;
            if (on) {
                argmax_take(c.q.x, i0 + 0, bv, bi);
                argmax_take(c.q.y, i0 + 1, bv, bi);
                argmax_take(c.q.z, i0 + 2, bv, bi);
                argmax_take(c.q.w, i0 + 3, bv, bi);
            }
            // (a) and (b); NaN fails peak8, a pixel off the plane is not `on`
            if (on & peak8(c.q.x, c.l, c.q.y, u.l, u.q.x, u.q.y, d.l, d.q.x, d.q.y) & (c.q.x != ninf)) better(c.q.x, i0 + 0, lv, li);
            if (on & peak8(c.q.y, c.q.x, c.q.z, u.q.x, u.q.y, u.q.z, d.q.x, d.q.y, d.q.z) & (c.q.y != ninf)) better(c.q.y, i0 + 1, lv, li);
            if (on & peak8(c.q.z, c.q.y, c.q.w, u.q.y, u.q.z, u.q.w, d.q.y, d.q.z, d.q.w) & (c.q.z != ninf)) better(c.q.z, i0 + 2, lv, li);
            if (on & peak8(c.q.w, c.q.z, c.r, u.q.z, u.q.w, u.r, d.q.z, d.q.w, d.r) & (c.q.w != ninf)) better(c.q.w, i0 + 3, lv, li);
            u = c;
            c = d;
        }
        // lanes 2j and 2j + 1 are one cell; the even lane writes its entry (a dead odd lane holds the empty marker)
        const float ov = __shfl_xor(lv, 1);
        const int oi = __shfl_xor(li, 1);
        better(ov, oi, lv, li);
        if (live && !(lane & 1)) {
            const int cell = sy * cw + (xv >> 1);
            tv[cell] = lv;
            ti[cell] = li;
        }
    }
    reduce_block(bv, bi, sv[0], si[0]);                     // (its barrier also publishes the table)
    if (threadIdx.x == 0)
        refine_keypoint([=](int yy, int xx) { return pl[yy * W + xx]; }, H, W, bi, row, irow);
    if (bi == EMPTY) bi = 0;                                // all-NaN / all -inf plane: refine_keypoint reports pixel 0
    int cx[ESAHRNET_MAX_CANDIDATES], cy[ESAHRNET_MAX_CANDIDATES];      // (m is a compile-time index below: registers)
    cx[0] = bi % W;
    cy[0] = bi / W;

    // ---- candidates 1 .. M-1 --------------------------------------------------------------------------------------------
#pragma unroll
    for (int m = 1; m < ESAHRNET_MAX_CANDIDATES; ++m) {
        if (m >= M) break;                                  // uniform over the workgroup
        // the cells the newest square touches (every thread is past the barrier behind its last read of the table)
        const int qx0 = max(cx[m - 1] - r, 0), qx1 = (int)min((long long)cx[m - 1] + r, (long long)W - 1);
        const int qy0 = max(cy[m - 1] - r, 0), qy1 = (int)min((long long)cy[m - 1] + r, (long long)H - 1);
        const int gx0 = qx0 / CELL, gy0 = qy0 / CELL, gw = qx1 / CELL - gx0 + 1, gh = qy1 / CELL - gy0 + 1;
        for (int g = wave; g < gw * gh; g += KW) {          // uniform over the wave
            const int gy = g / gw, ccx = gx0 + g - gy * gw, ccy = gy0 + gy;
            const int x = ccx * CELL + (lane & 7), y = ccy * CELL + (lane >> 3);
            const bool in = x < W && y < H;
            const int xc = in ? x : 0, yc = in ? y : 0;
            const int ya = (yc > 0 ? yc - 1 : yc) * W, yb = (yc < H - 1 ? yc + 1 : yc) * W, ym = yc * W;
            const int xa = xc > 0 ? xc - 1 : xc, xb = xc < W - 1 ? xc + 1 : xc;     // off the plane: the pixel's own row / column
            const float v = pl[ym + xc];
            const float a0 = pl[ya + xa], a1 = pl[ya + xc], a2 = pl[ya + xb], a3 = pl[ym + xa], a4 = pl[ym + xb],
                        a5 = pl[yb + xa], a6 = pl[yb + xc], a7 = pl[yb + xb];
            bool ok = in & peak8(v, a0, a1, a2, a3, a4, a5, a6, a7) & (v != ninf);
#pragma unroll
            for (int j = 0; j < m; ++j) {
                const int dx = abs(x - cx[j]), dy = abs(y - cy[j]);
                ok &= (dx > dy ? dx : dy) > r;
            }
            float lv = ok ? v : ninf;
            int li = ok ? ym + xc : EMPTY;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(lv, off);
                const int oi = __shfl_xor(li, off);
                better(ov, oi, lv, li);
            }
            if (lane == 0) {
                tv[ccy * cw + ccx] = lv;
                ti[ccy * cw + ccx] = li;
            }
        }
        __syncthreads();
        bv = ninf;
        bi = EMPTY;
        for (int t = threadIdx.x; t < ncells; t += KT) better(tv[t], ti[t], bv, bi);
        reduce_block(bv, bi, sv[m], si[m]);                 // (no NaN in the table: argmax_take is `better` there)
        if (bi == EMPTY) {                                  // no pixel qualifies (uniform): this row and the later ones
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

bool keypoints_candidates_onepass_eligible(const float* heat, int H, int W) {
    if (H <= 0 || W <= 0 || (reinterpret_cast<uintptr_t>(heat) & 15) || (W & 3)) return false;
    return (long long)((W + CELL - 1) / CELL) * ((H + CELL - 1) / CELL) <= kOnepassMaxCells;
}

int launch_keypoints_candidates_onepass(const float* heat, int planes, int H, int W, int M, int r, float* cand, int* cidx,
                                        hipStream_t stream) {
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || M < 1 || M > ESAHRNET_MAX_CANDIDATES || r < 0 ||
        !keypoints_candidates_onepass_eligible(heat, H, W))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(keypoints_candidates_onepass_kernel, dim3((unsigned)planes), dim3(KT), 0, stream, heat, H, W, M, r, cand,
                       cidx);
    return (int)hipGetLastError();
}

int launch_keypoints_candidates_auto(const float* heat, int planes, int H, int W, int M, int r, float* cand, int* cidx,
                                     hipStream_t stream) {
    if (M >= kOnepassFromM && keypoints_candidates_onepass_eligible(heat, H, W))
        return launch_keypoints_candidates_onepass(heat, planes, H, W, M, r, cand, cidx, stream);
    return launch_keypoints_candidates(heat, planes, H, W, M, r, cand, cidx, stream);
}

}  // namespace esa

extern "C" int esahrnet_keypoints_candidates_form(const void* heat_dev, int n, int k, int height, int width, int candidates,
                                                  int nms_radius, int form, void* cand_dev, void* cidx_dev,
                                                  esahrnet_stream stream) {
    // (the checks and the texts of esahrnet_keypoints_candidates, then the form's own)
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
    if (form < -1 || form > 1)
        return esa::set_error("keypoints_candidates: form=%d unknown (0: multi-sweep, 1: one sweep, -1: the fused paths' choice)", form);
    const float* heat = static_cast<const float*>(heat_dev);
    if (form == 1 && !esa::keypoints_candidates_onepass_eligible(heat, height, width))
        return esa::set_error("keypoints_candidates: form 1 (one sweep) needs heat_dev 16-byte aligned, a width that is a multiple "
                              "of 4 and at most %d cells of 8 x 8 pixels per plane (got %d x %d)", esa::kOnepassMaxCells, height,
                              width);
    auto* const launch = form == 1 ? esa::launch_keypoints_candidates_onepass
                       : form == 0 ? esa::launch_keypoints_candidates
                                   : esa::launch_keypoints_candidates_auto;
    const int rc = launch(heat, n * k, height, width, candidates, nms_radius, static_cast<float*>(cand_dev),
                          static_cast<int*>(cidx_dev), static_cast<hipStream_t>(stream));
    if (rc) return esa::set_error("keypoints_candidates: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}
