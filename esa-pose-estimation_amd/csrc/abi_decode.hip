// abi_decode.hip — the entries of include/esahrnet.h that take no handle: the stand-alone decoders (get_final, get_final2, the
// Gaussian fit), the loader's two steps (boxes, crops) and the correspondences.  Each checks its arguments, reports through
// esa::set_error and makes one launch; nothing here knows esahrnet_ctx (the units of plan.h keep every entry that does).  The
// test hooks on the launchers' process-wide state (esahrnet_debug_*) sit at the end.
//
// The argument checks that the handle-taking loader entries of loader.hip repeat word for word (esahrnet_frames_keypoints*,
// esahrnet_frames_correspondences) are defined here, in namespace esa, and declared in host_util.h: `who` names the
// entry in the message.
#include <cstdint>

#include "../../include/esahrnet.h"
#include "devstate.h"
#include "host_util.h"

namespace esa {

extern const int kFrontendMaxRows = 0xffffff;       // launch_crops_ex: one block per output row, m * scale of them

int check_boxes_args(const char* who, int m, int frame_h, int frame_w, int scale, int rule) {
    if (m <= 0) return set_error("%s: the number of boxes must be positive (got %d)", who, m);
    if (frame_h <= 0 || frame_w <= 0) return set_error("%s: bad frame size %d x %d", who, frame_h, frame_w);
    if (scale <= 0 || (long long)m * scale > kFrontendMaxRows)
        return set_error("%s: scale %d with %d boxes (scale positive, boxes * scale at most %d)", who, scale, m, kFrontendMaxRows);
    if (rule != 0 && rule != 1) return set_error("%s: rule=%d unknown (0: val, data_load_val.py; 1: train / demo, data_load4.py)", who, rule);
    return 0;
}

int check_crops_args(const char* who, int nframes, int pixel_format, float stdv) {
    if (nframes <= 0) return set_error("%s: the number of frames must be positive (got %d)", who, nframes);
    if (pixel_format != 0 && pixel_format != 1) return set_error("%s: pixel_format=%d unknown (0: gray8, 1: RGB8 interleaved)", who, pixel_format);
    if (!(stdv > 0.f)) return set_error("%s: stdv must be positive", who);
    return 0;
}

// what the _cov entries refuse about their three additions
int check_cov_args(const char* who, const void* cov_dev, const void* info_dev, double cov_floor) {
    if ((reinterpret_cast<uintptr_t>(cov_dev) | reinterpret_cast<uintptr_t>(info_dev)) & 7)
        return set_error("%s: cov_dev and info_dev must be 8-byte aligned", who);
    if (!(cov_floor >= 0.0)) return set_error("%s: cov_floor must be a number >= 0 (got %g)", who, cov_floor);
    return 0;
}

int check_corr_args(const char* who, int m, int k, int mode) {
    if (m <= 0) return set_error("%s: the number of crops must be positive (got %d)", who, m);
    if (k < 1 || k > 32) return set_error("%s: %d keypoints per crop unsupported (1..32: one wave per crop)", who, k);
    if (mode != 0 && mode != 1) return set_error("%s: mode=%d unknown (0: peak weights, 1: get_final2 Hessian weights)", who, mode);
    return 0;
}

}  // namespace esa

using esa::set_error;

// esahrnet_keypoints_gaussfit (with_cov false: cov_dev, info_dev and cov_floor unused, the launch without them) and
// esahrnet_keypoints_gaussfit_cov
static int keypoints_gaussfit(const char* who, bool with_cov, const void* heat_dev, int n, int k, int height, int width, void* kp_dev,
                              void* idx_dev, void* fit_dev, void* status_dev, void* hess_dev, void* cov_dev, void* info_dev,
                              double cov_floor, esahrnet_stream stream) {
    if (!heat_dev || !kp_dev || !status_dev) return set_error("%s: null argument", who);
    if (n <= 0 || k <= 0 || height <= 0 || width <= 0 || (long long)height * width > 0x7fffffffLL ||
        (long long)n * k > 0x7fffffffLL)
        return set_error("%s: bad shape %d x %d x %d x %d", who, n, k, height, width);
    if ((reinterpret_cast<uintptr_t>(heat_dev) | reinterpret_cast<uintptr_t>(kp_dev) | reinterpret_cast<uintptr_t>(idx_dev) |
         reinterpret_cast<uintptr_t>(status_dev)) & 3)
        return set_error("%s: heat_dev, kp_dev, idx_dev and status_dev must be 4-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(fit_dev) | reinterpret_cast<uintptr_t>(hess_dev)) & 7)
        return set_error("%s: fit_dev and hess_dev must be 8-byte aligned", who);
    if (with_cov && esa::check_cov_args(who, cov_dev, info_dev, cov_floor)) return 1;
    const float* heat = static_cast<const float*>(heat_dev);
    float* kp = static_cast<float*>(kp_dev);
    int *idx = static_cast<int*>(idx_dev), *status = static_cast<int*>(status_dev);
    double *fit = static_cast<double*>(fit_dev), *hess = static_cast<double*>(hess_dev);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = with_cov ? esa::launch_keypoints_gaussfit_cov(heat, n * k, height, width, kp, idx, fit, status, hess,
                                                                 static_cast<double*>(cov_dev), static_cast<double*>(info_dev),
                                                                 cov_floor, st)
                            : esa::launch_keypoints_gaussfit(heat, n * k, height, width, kp, idx, fit, status, hess, st);
    if (rc) return set_error("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    return 0;
}

extern "C" {

int esahrnet_keypoints_finish(const void* heat_dev, const void* part_dev, int ntiles, int n, int k, int height, int width,
                              void* kp_dev, void* idx_dev, esahrnet_stream stream) {
    if (!heat_dev || !part_dev || !kp_dev || n <= 0 || k <= 0 || ntiles <= 0) return set_error("keypoints_finish: bad argument");
    const int rc = esa::launch_keypoints_finish(static_cast<const float*>(heat_dev), static_cast<const float2*>(part_dev), ntiles,
                                                n * k, height, width, static_cast<float*>(kp_dev), static_cast<int*>(idx_dev),
                                                static_cast<hipStream_t>(stream));
    if (rc) return set_error("keypoints_finish: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

int esahrnet_keypoints_ex(const void* heat_dev, int n, int k, int height, int width, void* kp_dev, void* idx_dev,
                          esahrnet_stream stream) {
    if (!heat_dev || !kp_dev || n <= 0 || k <= 0) return set_error("keypoints: bad argument");
    const int rc = esa::launch_keypoints(static_cast<const float*>(heat_dev), n * k, height, width,
                                         static_cast<float*>(kp_dev), static_cast<int*>(idx_dev),
                                         static_cast<hipStream_t>(stream));
    if (rc) return set_error("keypoints: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

int esahrnet_keypoints(const void* heat_dev, int n, int k, int height, int width, void* kp_dev,
                       esahrnet_stream stream) {
    return esahrnet_keypoints_ex(heat_dev, n, k, height, width, kp_dev, nullptr, stream);
}

int esahrnet_keypoints_final2_workspace_bytes(int n, int k, int height, int width, size_t* bytes) {
    if (!bytes) return set_error("keypoints_final2_workspace_bytes: null argument");
    if (n <= 0 || k <= 0 || height <= 0 || width <= 0 || (long long)height * width > 0x7fffffffLL)
        return set_error("keypoints_final2_workspace_bytes: bad shape %d x %d x %d x %d", n, k, height, width);
    *bytes = esa::final2_workspace_bytes((long long)n * k, height, width);
    return 0;
}

int esahrnet_keypoints_final2(const void* heat_dev, int n, int k, int height, int width, void* kp_dev, void* idx_dev, void* ws_dev,
                              size_t ws_bytes, esahrnet_stream stream) {
    return esahrnet_keypoints_final2_hess(heat_dev, n, k, height, width, kp_dev, idx_dev, nullptr, ws_dev, ws_bytes, stream);
}

int esahrnet_keypoints_final2_hess(const void* heat_dev, int n, int k, int height, int width, void* kp_dev, void* idx_dev,
                                   void* hess_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    if (!heat_dev || !kp_dev || !ws_dev) return set_error("keypoints_final2: null argument");
    size_t need = 0;
    if (esahrnet_keypoints_final2_workspace_bytes(n, k, height, width, &need)) return 1;
    if ((long long)n * k * esa::final2_tiles(height, width) > 0x7fffffLL)
        return set_error("keypoints_final2: %d x %d planes of %d x %d: too many tiles for one launch", n, k, height, width);
    if (ws_bytes < need) return set_error("keypoints_final2: workspace too small (%zu < %zu)", ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(ws_dev) & 255) return set_error("keypoints_final2: workspace must be 256-byte aligned");
    const int rc = esa::launch_keypoints_final2(static_cast<const float*>(heat_dev), n * k, height, width, static_cast<float*>(kp_dev),
                                                static_cast<int*>(idx_dev), ws_dev, ws_bytes, static_cast<hipStream_t>(stream),
                                                static_cast<double*>(hess_dev));
    if (rc) return set_error("keypoints_final2: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

int esahrnet_keypoints_gaussfit(const void* heat_dev, int n, int k, int height, int width, void* kp_dev, void* idx_dev,
                                void* fit_dev, void* status_dev, void* hess_dev, esahrnet_stream stream) {
    return keypoints_gaussfit("keypoints_gaussfit", false, heat_dev, n, k, height, width, kp_dev, idx_dev, fit_dev, status_dev,
                              hess_dev, nullptr, nullptr, 0.0, stream);
}

int esahrnet_keypoints_gaussfit_cov(const void* heat_dev, int n, int k, int height, int width, void* kp_dev, void* idx_dev,
                                    void* fit_dev, void* status_dev, void* hess_dev, void* cov_dev, void* info_dev, double cov_floor,
                                    esahrnet_stream stream) {
    return keypoints_gaussfit("keypoints_gaussfit_cov", true, heat_dev, n, k, height, width, kp_dev, idx_dev, fit_dev, status_dev,
                              hess_dev, cov_dev, info_dev, cov_floor, stream);
}

int esahrnet_crops(const void* frames_dev, int n, int frame_h, int frame_w, const void* boxes_dev, int scale,
                   float mean, float stdv, void* out_dev, esahrnet_stream stream) {
    if (!frames_dev || !boxes_dev || !out_dev || n <= 0 || scale <= 0 || !(stdv > 0.f)) return set_error("crops: bad argument");
    const int rc = esa::launch_crops(static_cast<const unsigned char*>(frames_dev), static_cast<const int*>(boxes_dev),
                                     static_cast<float*>(out_dev), n, frame_h, frame_w, scale, mean, stdv,
                                     static_cast<hipStream_t>(stream));
    if (rc) return set_error("crops: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

int esahrnet_boxes(const void* det_boxes_dev, int m, int frame_h, int frame_w, int scale, int rule, void* crop_boxes_dev,
                   void* rates_dev, void* valid_dev, esahrnet_stream stream) {
    if (!det_boxes_dev || !crop_boxes_dev || !rates_dev || !valid_dev) return set_error("boxes: null argument");
    if (esa::check_boxes_args("boxes", m, frame_h, frame_w, scale, rule)) return 1;
    const int rc = esa::launch_boxes(static_cast<const int*>(det_boxes_dev), nullptr, 0, m, frame_h, frame_w, scale, rule,
                                     static_cast<int*>(crop_boxes_dev), static_cast<double*>(rates_dev),
                                     static_cast<int*>(valid_dev), static_cast<hipStream_t>(stream));
    if (rc) return set_error("boxes: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

int esahrnet_crops_ex(const void* frames_dev, int nframes, int frame_h, int frame_w, int pixel_format, const void* frame_idx_dev,
                      const void* crop_boxes_dev, const void* valid_dev, int m, int scale, float mean, float stdv, void* out_dev,
                      esahrnet_stream stream) {
    if (!frames_dev || !crop_boxes_dev || !out_dev) return set_error("crops_ex: null argument");
    if (esa::check_boxes_args("crops_ex", m, frame_h, frame_w, scale, 0) || esa::check_crops_args("crops_ex", nframes, pixel_format, stdv))
        return 1;
    if (!frame_idx_dev && m != nframes)
        return set_error("crops_ex: %d crops of %d frames need a frame index (NULL is the identity: crop i reads frame i)", m, nframes);
    const int rc = esa::launch_crops_ex(static_cast<const unsigned char*>(frames_dev), nframes, frame_h, frame_w, pixel_format,
                                        static_cast<const int*>(frame_idx_dev), static_cast<const int*>(crop_boxes_dev),
                                        static_cast<const int*>(valid_dev), static_cast<float*>(out_dev), m, scale, mean, stdv,
                                        static_cast<hipStream_t>(stream));
    if (rc) return set_error("crops_ex: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

int esahrnet_correspondences(const void* kp_dev, const void* hess_dev, const void* crop_boxes_dev, const void* rates_dev,
                             const void* valid_dev, int m, int k, double thresh, int min_k, int mode, void* count_dev,
                             void* order_dev, void* pts_dev, void* w_dev, esahrnet_stream stream) {
    if (!kp_dev || !crop_boxes_dev || !rates_dev || !valid_dev || !count_dev || !order_dev || !pts_dev || !w_dev)
        return set_error("correspondences: null argument");
    if (esa::check_corr_args("correspondences", m, k, mode)) return 1;
    if (mode == 1 && !hess_dev) return set_error("correspondences: mode 1 (Hessian weights) needs hess_dev (esahrnet_keypoints_final2_hess)");
    const int rc = esa::launch_correspond(static_cast<const float*>(kp_dev), static_cast<const double*>(hess_dev),
                                          static_cast<const int*>(crop_boxes_dev), static_cast<const double*>(rates_dev),
                                          static_cast<const int*>(valid_dev), m, k, thresh, min_k, mode, static_cast<int*>(count_dev),
                                          static_cast<int*>(order_dev), static_cast<double*>(pts_dev), static_cast<double*>(w_dev),
                                          static_cast<hipStream_t>(stream));
    if (rc) return set_error("correspondences: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

int esahrnet_correspondences_cand(const void* cand_dev, const void* hess_dev, const void* crop_boxes_dev, const void* rates_dev,
                                  const void* valid_dev, int m, int k, int candidates, double thresh, int min_k, int mode,
                                  void* count_dev, void* order_dev, void* cpts_dev, void* cw_dev, void* cpeak_dev,
                                  esahrnet_stream stream) {
    if (!cand_dev || !crop_boxes_dev || !rates_dev || !valid_dev || !count_dev || !order_dev || !cpts_dev || !cw_dev || !cpeak_dev ||
        (mode == 1 && !hess_dev))
        return set_error("correspondences_cand: null argument (hess_dev may be null with mode 0 only)");
    if (m <= 0) return set_error("correspondences_cand: the number of crops must be positive (got %d)", m);
    if (k < 1 || k > 32) return set_error("correspondences_cand: %d keypoints per crop unsupported (1..32: one wave per crop)", k);
    if (candidates < 1 || candidates > ESAHRNET_MAX_CANDIDATES)
        return set_error("correspondences_cand: %d candidates per keypoint unsupported (1..%d)", candidates, ESAHRNET_MAX_CANDIDATES);
    if (mode != 0 && mode != 1)
        return set_error("correspondences_cand: mode=%d unknown (0: peak weights, 1: Hessian weights)", mode);
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((at(cand_dev) | at(crop_boxes_dev) | at(valid_dev) | at(count_dev) | at(order_dev) | at(cpeak_dev)) & 3)
        return set_error("correspondences_cand: cand_dev, crop_boxes_dev, valid_dev, count_dev, order_dev and cpeak_dev must be 4-byte aligned");
    if (((mode == 1 ? at(hess_dev) : 0) | at(rates_dev) | at(cpts_dev) | at(cw_dev)) & 7)
        return set_error("correspondences_cand: hess_dev (mode 1), rates_dev, cpts_dev and cw_dev must be 8-byte aligned");
    const int rc = esa::launch_correspond_cand(static_cast<const float*>(cand_dev), mode == 1 ? static_cast<const double*>(hess_dev) : nullptr,
                                               static_cast<const int*>(crop_boxes_dev), static_cast<const double*>(rates_dev),
                                               static_cast<const int*>(valid_dev), m, k, candidates, thresh, min_k, mode,
                                               static_cast<int*>(count_dev), static_cast<int*>(order_dev), static_cast<double*>(cpts_dev),
                                               static_cast<double*>(cw_dev), static_cast<float*>(cpeak_dev),
                                               static_cast<hipStream_t>(stream));
    if (rc) return set_error("correspondences_cand: kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return 0;
}

// ---- the test hooks on the launchers' process-wide state (devstate.h, conv_s2c32.hip, conv_x6.hip) ------------------------
int esahrnet_debug_devstate(int* kernel_device_entries, int* devices) {
    esa::dev_state_counts(kernel_device_entries, devices);
    return 0;
}

int esahrnet_debug_set_launch_limit(long long bytes) {
    esa::set_stream_launch_limit(bytes);
    return 0;
}

int esahrnet_debug_set_x6_grid_limit(int workgroups) {
    esa::set_x6_grid_limit(workgroups);
    return 0;
}

int esahrnet_debug_set_cu_limit(int cus) {
    esa::set_cu_limit(cus);
    return 0;
}

}  // extern "C"
