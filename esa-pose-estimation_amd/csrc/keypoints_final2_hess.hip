// keypoints_final2_hess.hip — keypoints_final2.hip's decoder with a third output: hess f64 [planes][3] = (dxx, dxy, dyy), the
// Hessian of the blurred, rescaled, clamped log heat-map at the peak, the values the Newton step uses (refine.h final2_newton);
// NaN x 3 where no step is taken.  The same tile pass and the same finish (final2.h), the finish instantiated with its HESS flag:
// kp and idx_out have the bits keypoints_final2.hip gives, whose own two kernels are not touched by this file.
#include "final2.h"

namespace esa {

int launch_keypoints_final2_hess(const float* heat, int planes, int H, int W, float* kp, int* idx_out, double* hess, void* ws,
                                 size_t ws_bytes, hipStream_t stream) {
    return launch_final2<F2Nchw, true>(F2Nchw{heat}, planes, H, W, kp, idx_out, ws, ws_bytes, stream, hess);
}

}  // namespace esa
