// keypoints_gaussfit.hip — the third decoder: a 2-D Gaussian fitted to the window around each plane's arg-max.
//
// The reference's test.py fits offset + A exp(-(a dx^2 + 2 b dx dy + c dy^2)) to a 13 x 13 window with scipy's curve_fit on the
// host (milliseconds per keypoint); here one wave (64 lanes) fits one (crop, keypoint) plane, after launch_keypoints has left
// the plane's arg-max index and its (x, y, peak) row.  The model is test.py's, parametrised by (a, b, c) instead of (sigma_x,
// sigma_y, theta): theta is undetermined when the sigmas are equal, the centre and the fitted function are the same.
// The window, the solver and the stores are gaussfit.h's gaussfit_plane; the kernels here differ in where the window is read:
// gaussfit_kernel from f32 NCHW heat-maps, gf_nhwc_fit_kernel from NHWC heat-maps that never left the workspace (seg_hrnet3
// under esahrnet_forward_keypoints_gaussfit).  Contraction is off at file scope, as in the header: the restatement has no fma.
#include "gaussfit.h"
#include "kernels.h"
#include "sb.h"

#pragma clang fp contract(off)

namespace esa {
namespace {

// idx_in: the arg-max launch_keypoints wrote (idx_dev, or status when the caller passed no idx_dev: it is read here before the
// status replaces it).  kp rows arrive holding launch_keypoints' (x, y, peak); an accepted fit replaces x and y.
__global__ __launch_bounds__(64) void gaussfit_kernel(const float* heat, const int* idx_in, int H, int W, float* kp, double* fit,
                                                      int* status, double* hess) {
    const size_t plane = blockIdx.x;
    const float* pl = heat + plane * H * W;
    gaussfit_plane([=](int yy, int xx) { return pl[(size_t)yy * W + xx]; }, plane, H, W, idx_in[plane], kp, fit, status, hess);
}

// The same fit on heat-maps x [N][H][W][Cp] (f32 or split-bf16 groups of 8 channels, sb.h), each value the bits
// keypoints_finish_nhwc_kernel reads: no NCHW copy is made.  idx_in and kp as above, from launch_keypoints_finish_nhwc.
template <bool F32>
__global__ __launch_bounds__(64) void gf_nhwc_fit_kernel(const char* x, int C, int Cp, const int* idx_in, int H, int W, float* kp,
                                                         double* fit, int* status, double* hess) {
    const size_t plane = blockIdx.x;
    const int n = (int)(blockIdx.x / (unsigned)C), c = (int)(blockIdx.x % (unsigned)C), j = c & 7;
    const char* img = x + (size_t)n * ((size_t)H * W * Cp * 4) + (c >> 3) * 32;
    gaussfit_plane([=](int yy, int xx) { return load1_fmt(img + ((size_t)yy * W + xx) * (Cp * 4), j, F32); }, plane, H, W,
                   idx_in[plane], kp, fit, status, hess);
}

}  // namespace

int launch_gaussfit_fit(const float* heat, const int* idx_in, int planes, int H, int W, float* kp, double* fit, int* status,
                        double* hess, hipStream_t stream) {
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(gaussfit_kernel, dim3((unsigned)planes), dim3(64), 0, stream, heat, idx_in, H, W, kp, fit, status, hess);
    return (int)hipGetLastError();
}

int launch_gaussfit_fit_nhwc(int fmt, const char* x, int N, int C, int H, int W, int Cp, const int* idx_in, float* kp, double* fit,
                             int* status, double* hess, hipStream_t stream) {
    const long long planes = (long long)N * C;
    if (N <= 0 || C < 1 || C > Cp || (Cp & 7) || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || planes > 0x7fffffffLL ||
        (fmt != FMT_SB && fmt != FMT_F32))
        return (int)hipErrorInvalidValue;
    auto kern = fmt == FMT_F32 ? gf_nhwc_fit_kernel<true> : gf_nhwc_fit_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)planes), dim3(64), 0, stream, x, C, Cp, idx_in, H, W, kp, fit, status, hess);
    return (int)hipGetLastError();
}

int launch_keypoints_gaussfit(const float* heat, int planes, int H, int W, float* kp, int* idx_out, double* fit, int* status,
                              double* hess, hipStream_t stream) {
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    int* idx = idx_out ? idx_out : status;
    const int rc = launch_keypoints(heat, planes, H, W, kp, idx, stream);
    if (rc) return rc;
    return launch_gaussfit_fit(heat, idx, planes, H, W, kp, fit, status, hess, stream);
}

}  // namespace esa
