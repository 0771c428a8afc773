// keypoints_at.hip — the three decoders at pixels the caller names:  f32 [planes][H][W], int32 [planes][m] -> f32 [planes][m][3].
//
// Every other decoder here refines at the plane's arg-max, which it finds itself.  The reference's get_final(hm, coords) and
// get_final2(hm, coords) refine at the pixels they are handed (inference.py:136-169), and the runner-up search
// (keypoints_candidates.hip) knows the pixel of every candidate: these kernels take a pixel, at = row * W + column, for each of
// the m slots of a plane, and decode there.  One wave per slot; a slot's result depends on its plane and its pixel alone.
//
//   decoder 0   refine_keypoint (refine.h) at the pixel: the row keypoints.hip and keypoints_candidates.hip write for a peak
//               there.  That call is compiled here as it is there (no contraction pragma around it), so the bits are theirs.
//   decoder 1   get_final2.  The rescale factor is a quantity of the whole plane (raw maximum over blurred maximum,
//               inference.py:104-109), so final2.h's tile pass runs once per plane, whatever m; the finish of a slot reduces the
//               plane's tile records, evaluates the 13 blurred points around ITS pixel (blur_at) and ends in refine.h's
//               final2_finish, the guards and the Newton step of the arg-max decoder.  The third column is the raw value at
//               the pixel.  At the arg-max: the bits of keypoints_final2.hip / keypoints_final2_hess.hip.
//   decoder 2   the decoder-0 row at the pixel, then gaussfit.h's gaussfit_plane with the pixel as the window's centre (with
//               its covariance pass where cov or info is asked for), in one kernel.  At the arg-max: the bits of
//               keypoints_gaussfit.hip / keypoints_gaussfit_cov.hip.
//   outside     a pixel outside [0, H * W) (-1 is what cidx holds where there is no candidate) gives NaN in kp and in every
//               f64 output and status -1; nothing of the plane is read for it.
// Every output is written whole; heat and at are only read.  No allocation, no synchronisation with the host.
#include <cmath>
#include <cstdint>

#include "final2.h"
#include "gaussfit.h"
#include "kernels.h"
#include "refine.h"

#include "../../include/esahrnet.h"

namespace esa {
namespace {

__device__ __forceinline__ bool at_inside(int a, int H, int W) { return (unsigned)a < (unsigned)(H * W); }

// lane 0: the outputs of a slot whose pixel lies outside the plane (h3, c3, i3 / f8: the f64 outputs of 3 / 8 per slot, null where
// the call has none)
__device__ __forceinline__ void at_store_outside(size_t slot, float* kp, int* status, double* h3, double* f8, double* c3, double* i3) {
    const float nanf = __int_as_float(0x7fc00000);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    kp[slot * 3 + 0] = kp[slot * 3 + 1] = kp[slot * 3 + 2] = nanf;
    if (status) status[slot] = -1;
    if (h3) h3[slot * 3 + 0] = h3[slot * 3 + 1] = h3[slot * 3 + 2] = nan;
    if (c3) c3[slot * 3 + 0] = c3[slot * 3 + 1] = c3[slot * 3 + 2] = nan;
    if (i3) i3[slot * 3 + 0] = i3[slot * 3 + 1] = i3[slot * 3 + 2] = nan;
    if (f8)
        for (int j = 0; j < 8; ++j) f8[slot * 8 + j] = nan;
}

// decoder 0
__global__ __launch_bounds__(64) void at_final_kernel(const float* heat, const int* at, int H, int W, int m, float* kp,
                                                      int* status) {
    const size_t slot = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int a = at[slot];
    if (!at_inside(a, H, W)) {
        at_store_outside(slot, kp, status, nullptr, nullptr, nullptr, nullptr);
        return;
    }
    const float* pl = heat + (slot / (unsigned)m) * H * W;
    refine_keypoint([=](int yy, int xx) { return pl[yy * W + xx]; }, H, W, a, kp + slot * 3, nullptr);
    if (status) status[slot] = 0;
}

// decoder 1, behind final2_tile_kernel: final2_finish_kernel (final2.h) with the pixel given instead of reduced
template <bool HESS>
__global__ __launch_bounds__(64) void at_final2_kernel(const float* heat, const int* at, const float2* part, const float* bmax,
                                                       int ntiles, int H, int W, int m, float* kp, double* hess, int* status) {
#pragma clang fp contract(off)
    const size_t slot = blockIdx.x, plane = slot / (unsigned)m;
    const int a = at[slot];
    if (!at_inside(a, H, W)) {                             // (uniform over the wave)
        if (threadIdx.x == 0) at_store_outside(slot, kp, status, hess, nullptr, nullptr, nullptr);
        return;
    }
    float bv;
    int bi;
    reduce_tile_maxima(part + plane * ntiles, ntiles, bv, bi);      // bv: the plane's raw maximum (bi, its place, is not used)
    float bm = -INFINITY;
    for (int t = threadIdx.x; t < ntiles; t += 64) bm = max_nan(bm, bmax[plane * ntiles + t]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) bm = max_nan(bm, __shfl_xor(bm, off));
    const int px = a % W, py = a / W;
    const float* pl = heat + plane * H * W;
    final2_finish<HESS>(
        bv, a, bm, H, W,
        [&](int j) { return (float)blur_at(pl, H, W, py + final2_point_dy(j), px + final2_point_dx(j)); },
        [&] { return pl[a]; }, kp, nullptr, (int)slot, hess);
    if (status && threadIdx.x == 0) status[slot] = 0;
}

// decoder 2: lane 0 writes the decoder-0 row, then the wave fits around the same pixel
template <bool COV>
__global__ __launch_bounds__(64) void at_gaussfit_kernel(const float* heat, const int* at, int H, int W, int m, float* kp,
                                                         double* fit, int* status, double* hess, double* cov, double* info,
                                                         double cov_floor) {
    const size_t slot = blockIdx.x;
    const int a = at[slot];
    if (!at_inside(a, H, W)) {                             // (uniform over the wave)
        if (threadIdx.x == 0) at_store_outside(slot, kp, status, hess, fit, cov, info);
        return;
    }
    const float* pl = heat + (slot / (unsigned)m) * H * W;
    if (threadIdx.x == 0) refine_keypoint([=](int yy, int xx) { return pl[yy * W + xx]; }, H, W, a, kp + slot * 3, nullptr);
    gaussfit_plane<COV>([=](int yy, int xx) { return pl[(size_t)yy * W + xx]; }, slot, H, W, a, kp, fit, status, hess, cov, info,
                        cov_floor);
}

}  // namespace

// the launches of one call; every argument has been checked (kernels.h: the fused forward launches them too)
int launch_keypoints_at(const float* heat, int planes, int H, int W, const int* at, int m, int decoder, float* kp, double* hess,
                        double* fit, int* status, double* cov, double* info, double cov_floor, void* ws, hipStream_t stream) {
    const unsigned slots = (unsigned)((long long)planes * m);
    if (decoder == 0) {
        hipLaunchKernelGGL(at_final_kernel, dim3(slots), dim3(64), 0, stream, heat, at, H, W, m, kp, status);
        return (int)hipGetLastError();
    }
    if (decoder == 2) {
        auto kern = cov || info ? at_gaussfit_kernel<true> : at_gaussfit_kernel<false>;
        hipLaunchKernelGGL(kern, dim3(slots), dim3(64), 0, stream, heat, at, H, W, m, kp, fit, status, hess, cov, info, cov_floor);
        return (int)hipGetLastError();
    }
    const int ntiles = final2_tiles(H, W);                 // (the workspace of launch_final2, final2.h: tile records, then maxima)
    const size_t nt = (size_t)planes * ntiles;
    if (nt > 0x7fffffu) return (int)hipErrorInvalidValue;  // (check_at_args refuses it by name; the fused forward gets here without)
    float2* part = static_cast<float2*>(ws);
    float* bmax = reinterpret_cast<float*>(static_cast<char*>(ws) + ((nt * 8 + 255) & ~(size_t)255));
    hipLaunchKernelGGL(final2_tile_kernel<F2Nchw>, dim3((unsigned)nt), dim3(F2_T), 0, stream, F2Nchw{heat}, H, W,
                       (W + F2_TW - 1) / F2_TW, ntiles, part, bmax);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    auto kern = hess ? at_final2_kernel<true> : at_final2_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(slots), dim3(64), 0, stream, heat, at, part, bmax, ntiles, H, W, m, kp, hess, status);
    return (int)hipGetLastError();
}

size_t at_workspace_bytes(long long planes, int H, int W, int decoder) {
    return decoder == 1 ? final2_workspace_bytes(planes, H, W) : 0;
}

namespace {

// every refusal of esahrnet_keypoints_at, in the order include/esahrnet.h documents; `who` names the entry in the message
int check_at_args(const char* who, const void* heat_dev, int n, int k, int height, int width, const void* at_dev, int m, int decoder,
                  const void* kp_dev, const void* hess_dev, const void* fit_dev, const void* status_dev, const void* cov_dev,
                  const void* info_dev, double cov_floor, const void* ws_dev, size_t ws_bytes) {
    if (!heat_dev || !at_dev || !kp_dev) return set_error("%s: null argument", who);
    if (n <= 0 || k <= 0 || height <= 0 || width <= 0 || (long long)height * width > 0x7fffffffLL ||
        (long long)n * k > 0x7fffffffLL)
        return set_error("%s: bad shape %d x %d x %d x %d", who, n, k, height, width);
    if (m < 1 || (long long)n * k * m > 0x7fffffffLL)
        return set_error("%s: %d pixels per heat-map unsupported (at least 1, n * k * m at most 2^31 - 1)", who, m);
    if (decoder < 0 || decoder > 2) return set_error("%s: decoder=%d unknown (0: get_final, 1: get_final2, 2: gaussfit)", who, decoder);
    if (decoder == 0 && (hess_dev || fit_dev || cov_dev || info_dev))
        return set_error("%s: decoder 0 (get_final) writes no hess_dev, fit_dev, cov_dev or info_dev: pass NULL", who);
    if (decoder == 1 && (fit_dev || cov_dev || info_dev))
        return set_error("%s: decoder 1 (get_final2) writes no fit_dev, cov_dev or info_dev: pass NULL", who);
    if (decoder == 2 && !status_dev) return set_error("%s: decoder 2 (gaussfit) needs status_dev", who);
    if (!(cov_floor >= 0.0) || !std::isfinite(cov_floor))
        return set_error("%s: cov_floor must be a finite number >= 0 (got %g)", who, cov_floor);
    if ((reinterpret_cast<uintptr_t>(heat_dev) | reinterpret_cast<uintptr_t>(at_dev) | reinterpret_cast<uintptr_t>(kp_dev) |
         reinterpret_cast<uintptr_t>(status_dev)) & 3)
        return set_error("%s: heat_dev, at_dev, kp_dev and status_dev must be 4-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(hess_dev) | reinterpret_cast<uintptr_t>(fit_dev) | reinterpret_cast<uintptr_t>(cov_dev) |
         reinterpret_cast<uintptr_t>(info_dev)) & 7)
        return set_error("%s: hess_dev, fit_dev, cov_dev and info_dev must be 8-byte aligned", who);
    if (decoder == 1) {
        if ((long long)n * k * final2_tiles(height, width) > 0x7fffffLL)
            return set_error("%s: %d x %d planes of %d x %d: too many tiles for one launch", who, n, k, height, width);
        const size_t need = at_workspace_bytes((long long)n * k, height, width, decoder);
        if (!ws_dev || ws_bytes < need) return set_error("%s: workspace too small (%zu < %zu)", who, ws_dev ? ws_bytes : (size_t)0, need);
        if (reinterpret_cast<uintptr_t>(ws_dev) & 255) return set_error("%s: workspace must be 256-byte aligned", who);
    }
    return 0;
}

}  // namespace
}  // namespace esa

extern "C" int esahrnet_keypoints_at_workspace_bytes(int n, int k, int height, int width, int decoder, size_t* bytes) {
    if (!bytes) return esa::set_error("keypoints_at_workspace_bytes: null argument");
    if (n <= 0 || k <= 0 || height <= 0 || width <= 0 || (long long)height * width > 0x7fffffffLL)
        return esa::set_error("keypoints_at_workspace_bytes: bad shape %d x %d x %d x %d", n, k, height, width);
    if (decoder < 0 || decoder > 2)
        return esa::set_error("keypoints_at_workspace_bytes: decoder=%d unknown (0: get_final, 1: get_final2, 2: gaussfit)", decoder);
    *bytes = esa::at_workspace_bytes((long long)n * k, height, width, decoder);
    return 0;
}

extern "C" int esahrnet_keypoints_at(const void* heat_dev, int n, int k, int height, int width, const void* at_dev, int m, int decoder,
                                     void* kp_dev, void* hess_dev, void* fit_dev, void* status_dev, void* cov_dev, void* info_dev,
                                     double cov_floor, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    if (esa::check_at_args("keypoints_at", heat_dev, n, k, height, width, at_dev, m, decoder, kp_dev, hess_dev, fit_dev, status_dev,
                           cov_dev, info_dev, cov_floor, ws_dev, ws_bytes))
        return 1;
    const int rc = esa::launch_keypoints_at(static_cast<const float*>(heat_dev), n * k, height, width, static_cast<const int*>(at_dev), m,
                                            decoder, static_cast<float*>(kp_dev), static_cast<double*>(hess_dev),
                                            static_cast<double*>(fit_dev), static_cast<int*>(status_dev), static_cast<double*>(cov_dev),
                                            static_cast<double*>(info_dev), cov_floor, ws_dev, static_cast<hipStream_t>(stream));
    if (rc) return esa::set_error("keypoints_at: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

extern "C" int esahrnet_keypoints_candidates_refined(const void* heat_dev, int n, int k, int height, int width, int candidates,
                                                     int nms_radius, int decoder, void* cand_dev, void* cidx_dev, void* hess_dev,
                                                     void* fit_dev, void* status_dev, void* cov_dev, void* info_dev, double cov_floor,
                                                     void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    const char* who = "keypoints_candidates_refined";
    if (!heat_dev || !cand_dev || !cidx_dev) return esa::set_error("%s: null argument (cidx_dev is required here)", who);
    if (n <= 0 || k <= 0 || height <= 0 || width <= 0 || (long long)height * width > 0x7fffffffLL ||
        (long long)n * k > 0x7fffffffLL)
        return esa::set_error("%s: bad shape %d x %d x %d x %d", who, n, k, height, width);
    if (candidates < 1 || candidates > ESAHRNET_MAX_CANDIDATES)
        return esa::set_error("%s: %d candidates per heat-map unsupported (1..%d)", who, candidates, ESAHRNET_MAX_CANDIDATES);
    if (nms_radius < 0) return esa::set_error("%s: negative nms_radius %d", who, nms_radius);
    if (esa::check_at_args(who, heat_dev, n, k, height, width, cidx_dev, candidates, decoder, cand_dev, hess_dev, fit_dev, status_dev,
                           cov_dev, info_dev, cov_floor, ws_dev, ws_bytes))
        return 1;
    if (esahrnet_keypoints_candidates_form(heat_dev, n, k, height, width, candidates, nms_radius, -1, cand_dev, cidx_dev, stream))
        return 1;
    if (decoder == 0 && !status_dev) return 0;             // the candidate kernel's rows ARE decoder 0's: nothing to refine
    const int rc = esa::launch_keypoints_at(static_cast<const float*>(heat_dev), n * k, height, width, static_cast<const int*>(cidx_dev),
                                            candidates, decoder, static_cast<float*>(cand_dev), static_cast<double*>(hess_dev),
                                            static_cast<double*>(fit_dev), static_cast<int*>(status_dev), static_cast<double*>(cov_dev),
                                            static_cast<double*>(info_dev), cov_floor, ws_dev, static_cast<hipStream_t>(stream));
    if (rc) return esa::set_error("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    return 0;
}
