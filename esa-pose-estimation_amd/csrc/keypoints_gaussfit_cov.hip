// keypoints_gaussfit_cov.hip — keypoints_gaussfit.hip's decoder with two more outputs: cov f64 [planes][3], the covariance of the
// fitted centre as scipy's curve_fit reports it (s^2 (J^T J)^-1, its (x0, y0) block, crop px^2), and info f64 [planes][3] = -cov^-1,
// which esahrnet_correspondences(mode 1) takes in hess_dev's place: w = rate (-info)^(1/2) = rate cov^(-1/2).  The same window, the
// same solver and the same stores (gaussfit.h gaussfit_plane, instantiated with its COV flag): kp, idx, fit, status and hess have
// the bits keypoints_gaussfit.hip gives, whose own kernels are not touched by this file.  Contraction is off, as there.
#include "gaussfit.h"
#include "kernels.h"
#include "sb.h"

#pragma clang fp contract(off)

namespace esa {
namespace {

// gaussfit_kernel (keypoints_gaussfit.hip) with the covariance pass behind the fit
__global__ __launch_bounds__(64) void gfcov_kernel(const float* heat, const int* idx_in, int H, int W, float* kp, double* fit,
                                                   int* status, double* hess, double* cov, double* info, double cov_floor) {
    const size_t plane = blockIdx.x;
    const float* pl = heat + plane * H * W;
    gaussfit_plane<true>([=](int yy, int xx) { return pl[(size_t)yy * W + xx]; }, plane, H, W, idx_in[plane], kp, fit, status, hess,
                         cov, info, cov_floor);
}

// gf_nhwc_fit_kernel (keypoints_gaussfit.hip) with the covariance pass behind the fit
template <bool F32>
__global__ __launch_bounds__(64) void gfcov_nhwc_kernel(const char* x, int C, int Cp, const int* idx_in, int H, int W, float* kp,
                                                        double* fit, int* status, double* hess, double* cov, double* info,
                                                        double cov_floor) {
    const size_t plane = blockIdx.x;
    const int n = (int)(blockIdx.x / (unsigned)C), c = (int)(blockIdx.x % (unsigned)C), j = c & 7;
    const char* img = x + (size_t)n * ((size_t)H * W * Cp * 4) + (c >> 3) * 32;
    gaussfit_plane<true>([=](int yy, int xx) { return load1_fmt(img + ((size_t)yy * W + xx) * (Cp * 4), j, F32); }, plane, H, W,
                         idx_in[plane], kp, fit, status, hess, cov, info, cov_floor);
}

}  // namespace

int launch_gaussfit_fit_cov(const float* heat, const int* idx_in, int planes, int H, int W, float* kp, double* fit, int* status,
                            double* hess, double* cov, double* info, double cov_floor, hipStream_t stream) {
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || !(cov_floor >= 0.0)) return (int)hipErrorInvalidValue;
    if (!cov && !info) return launch_gaussfit_fit(heat, idx_in, planes, H, W, kp, fit, status, hess, stream);
    hipLaunchKernelGGL(gfcov_kernel, dim3((unsigned)planes), dim3(64), 0, stream, heat, idx_in, H, W, kp, fit, status, hess, cov,
                       info, cov_floor);
    return (int)hipGetLastError();
}

int launch_gaussfit_fit_nhwc_cov(int fmt, const char* x, int N, int C, int H, int W, int Cp, const int* idx_in, float* kp,
                                 double* fit, int* status, double* hess, double* cov, double* info, double cov_floor,
                                 hipStream_t stream) {
    if (!(cov_floor >= 0.0)) return (int)hipErrorInvalidValue;
    if (!cov && !info) return launch_gaussfit_fit_nhwc(fmt, x, N, C, H, W, Cp, idx_in, kp, fit, status, hess, stream);
    const long long planes = (long long)N * C;
    if (N <= 0 || C < 1 || C > Cp || (Cp & 7) || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || planes > 0x7fffffffLL ||
        (fmt != FMT_SB && fmt != FMT_F32))
        return (int)hipErrorInvalidValue;
    auto kern = fmt == FMT_F32 ? gfcov_nhwc_kernel<true> : gfcov_nhwc_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)planes), dim3(64), 0, stream, x, C, Cp, idx_in, H, W, kp, fit, status, hess, cov, info,
                       cov_floor);
    return (int)hipGetLastError();
}

int launch_keypoints_gaussfit_cov(const float* heat, int planes, int H, int W, float* kp, int* idx_out, double* fit, int* status,
                                  double* hess, double* cov, double* info, double cov_floor, hipStream_t stream) {
    if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || !(cov_floor >= 0.0)) return (int)hipErrorInvalidValue;
    int* idx = idx_out ? idx_out : status;
    const int rc = launch_keypoints(heat, planes, H, W, kp, idx, stream);
    if (rc) return rc;
    return launch_gaussfit_fit_cov(heat, idx, planes, H, W, kp, fit, status, hess, cov, info, cov_floor, stream);
}

}  // namespace esa
