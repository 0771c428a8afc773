// keypoints_final2.hip — heat-maps -> keypoints with the reference's second decoder, get_final2 (inference.py:154-169):
// an 11x11 Gaussian blur of each plane rescaled to the plane's raw maximum (gaussian_blur, :96-111), np.maximum(., 1e-10),
// log, then one Newton step with the full 2x2 Hessian (taylor, :54-73).  f32 [planes][H][W] -> f32 [planes][3] = (x, y, raw
// peak) and the int32 arg-max index, the same layout and the same arg-max / peak bits as keypoints.hip.
//
// Two launches, the heat-maps are read once and the blurred planes never leave the chip:
//   tile pass   one workgroup per (plane, 32x64 tile): the tile and its 5-pixel halo (zeros outside the plane) go to LDS,
//               a row pass and a column pass in f64 (fixed tap order) give the blurred tile, rounded to f32; the workspace
//               receives the tile's first raw maximum (value, index), as the output layer's per-tile maxima do, and its
//               blurred maximum (NaN wins, as in np.max).
//   finish      one wave per plane: the first raw maximum over the tiles (reduce_tile_maxima: the arg-max and peak of
//               launch_keypoints), the blurred maximum, and the 13 blurred values the Newton step reads, each re-evaluated
//               from the raw plane (121 taps) by the tile pass's own function, so that they are the same f32 values.
// The kernels live in final2.h, templated on how a plane is read; this file instantiates them for NCHW f32 heat-maps,
// layout.hip for seg_hrnet3's NHWC heat-maps.
// Numerics (refine.h final2_newton): the restatement in tests/final2_ref.py.  No fma anywhere in this file: the host
// restatement sums in plain IEEE f64.
// With the Hessian as a third output the finish is another instantiation: keypoints_final2_hess.hip.
#include "final2.h"

namespace esa {

int final2_tiles(int H, int W) { return ((H + F2_TH - 1) / F2_TH) * ((W + F2_TW - 1) / F2_TW); }

size_t final2_workspace_bytes(long long planes, int H, int W) {
    const size_t nt = (size_t)planes * final2_tiles(H, W);
    return ((nt * 8 + 255) & ~(size_t)255) + ((nt * 4 + 255) & ~(size_t)255);
}

int launch_keypoints_final2(const float* heat, int planes, int H, int W, float* kp, int* idx_out, void* ws, size_t ws_bytes,
                            hipStream_t stream, double* hess) {
    if (hess) return launch_keypoints_final2_hess(heat, planes, H, W, kp, idx_out, hess, ws, ws_bytes, stream);
    return launch_final2(F2Nchw{heat}, planes, H, W, kp, idx_out, ws, ws_bytes, stream);
}

}  // namespace esa
