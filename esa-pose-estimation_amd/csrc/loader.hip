// loader.hip — the loader on the device: detector boxes + frames -> crops (frontend.hip) -> the forward with a decoder -> keypoints,
// and the correspondences for the pose solver behind it (correspond.hip).  The entries esahrnet_frames_*.
#include "plan.h"

using namespace esa;

extern "C" {

// what the loader entries take besides the handle and the decoder's outputs
struct FramesArgs {
    const void* frames;
    int nframes, frame_h, frame_w, pixel_format;
    const void* det_boxes;
    const void* frame_idx;
    int m, scale, rule;
    float mean, stdv;
    void *crop_boxes, *rates, *valid;
    void* ws;
    size_t ws_bytes;
    esahrnet_stream stream;
};

static size_t frontend_crop_bytes(int m, int scale) { return pad256((size_t)m * scale * scale * sizeof(float)); }

// the loader's workspace: its crops, then the workspace of the forward with decoder `d` on them
static int frames_workspace_bytes(const char* who, esahrnet_handle h, int m, int scale, Decoder d, size_t* bytes, int refine = -1) {
    if (h->cfg.cin != 1)
        return set_error("%s: the loader makes 1-channel crops (data_load_val.py / data_load4.py); this handle takes %d channels", who,
                         h->cfg.cin);
    if (m <= 0 || scale <= 0 || (long long)m * scale > esa::kFrontendMaxRows)
        return set_error("%s: scale %d with %d boxes (both positive, boxes * scale at most %d)", who, scale, m, esa::kFrontendMaxRows);
    size_t fw = 0;
    if (forward_workspace_bytes(who, h, m, scale, scale, d, &fw, refine)) return 1;
    *bytes = frontend_crop_bytes(m, scale) + fw;
    return 0;
}

int esahrnet_frames_keypoints_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, size_t* bytes) {
    if (!h || !bytes) return set_error("frames_keypoints_workspace_bytes: null argument");
    if (decoder != 0 && decoder != 1) return set_error("frames_keypoints: decoder=%d unknown (0: get_final, 1: get_final2)", decoder);
    return frames_workspace_bytes("frames_keypoints", h, m, scale, decoder ? DEC_FINAL2 : DEC_FINAL, bytes);
}

int esahrnet_frames_keypoints_gaussfit_workspace_bytes(esahrnet_handle h, int m, int scale, size_t* bytes) {
    if (!h || !bytes) return set_error("frames_keypoints_gaussfit_workspace_bytes: null argument");
    return frames_workspace_bytes("frames_keypoints_gaussfit", h, m, scale, DEC_GAUSSFIT, bytes);
}

int esahrnet_frames_keypoints_candidates_workspace_bytes(esahrnet_handle h, int m, int scale, size_t* bytes) {
    if (!h || !bytes) return set_error("frames_keypoints_candidates_workspace_bytes: null argument");
    return frames_workspace_bytes("frames_keypoints_candidates", h, m, scale, DEC_CAND, bytes);
}

int esahrnet_frames_keypoints_candidates_refined_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, size_t* bytes) {
    if (!h || !bytes) return set_error("frames_keypoints_candidates_refined_workspace_bytes: null argument");
    if (check_refined_decoder("frames_keypoints_candidates_refined", decoder)) return 1;
    return frames_workspace_bytes("frames_keypoints_candidates_refined", h, m, scale, DEC_CAND, bytes, decoder);
}

// what every loader entry refuses about the frames and the boxes
static int check_frames_args(const char* who, const FramesArgs& a) {
    if (esa::check_boxes_args(who, a.m, a.frame_h, a.frame_w, a.scale, a.rule) ||
        esa::check_crops_args(who, a.nframes, a.pixel_format, a.stdv))
        return 1;
    if (!a.frame_idx && a.m != a.nframes)
        return set_error("%s: %d boxes on %d frames need a frame index (NULL is the identity: box i lies on frame i)", who, a.m, a.nframes);
    return 0;
}

// The loader entries after their argument checks (`who` names the caller in the messages): boxes -> crops at the head of the
// workspace -> forward + the decoder of `r` -> NaN rows for invalid crops.
static int frames_run(const char* who, esahrnet_handle h, const FramesArgs& a, const Request& r) {
    const hipStream_t st = static_cast<hipStream_t>(a.stream);
    const int* const frame_idx = static_cast<const int*>(a.frame_idx);
    int* const crop_boxes = static_cast<int*>(a.crop_boxes);
    int* const valid = static_cast<int*>(a.valid);
    int rc = esa::launch_boxes(static_cast<const int*>(a.det_boxes), frame_idx, a.nframes, a.m, a.frame_h, a.frame_w, a.scale, a.rule,
                               crop_boxes, static_cast<double*>(a.rates), valid, st);
    if (!rc)
        rc = esa::launch_crops_ex(static_cast<const unsigned char*>(a.frames), a.nframes, a.frame_h, a.frame_w, a.pixel_format,
                                  frame_idx, crop_boxes, valid, static_cast<float*>(a.ws), a.m, a.scale, a.mean, a.stdv, st);
    if (rc) return set_error("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    const size_t head = frontend_crop_bytes(a.m, a.scale);
    if (run_forward(h, a.ws, a.m, a.scale, a.scale, nullptr, nullptr, static_cast<char*>(a.ws) + head, a.ws_bytes - head, a.stream,
                    nullptr, &r))
        return 1;
    if (r.decoder == DEC_CAND && r.refine >= 0)     // every output of the refined candidates has K * M rows per crop
        rc = esa::launch_mark_invalid_refined(valid, a.m, h->cfg.num_keypoints * r.M, r.cand, r.cidx, r.status, r.hess, r.fit, r.cov,
                                              r.info, st);
    else if (r.decoder == DEC_CAND)                 // a crop's K * M candidate rows: the kp / idx rows of K * M keypoints
        rc = esa::launch_mark_invalid(valid, a.m, h->cfg.num_keypoints * r.M, r.cand, r.cidx, st);
    else if (r.decoder == DEC_GAUSSFIT)
        rc = esa::launch_mark_invalid_gaussfit_cov(valid, a.m, h->cfg.num_keypoints, r.kp, r.idx, r.fit, r.status, r.hess, r.cov,
                                                   r.info, st);
    else rc = esa::launch_mark_invalid(valid, a.m, h->cfg.num_keypoints, r.kp, r.idx, st);
    if (rc) return set_error("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    return 0;
}

// The five esahrnet_frames_keypoints* entries: everything that can be refused is refused here, before the first launch.
// abi_decoder: the `decoder` argument as given, of esahrnet_frames_keypoints (refused by its workspace query when unknown) or of
// the refined candidates' entry (`refined` says so: with an unknown decoder r.refine is the plain search's); unused by the others.
// Each entry keeps the order of its refusals: the _cov form checks its three additions before the handle's commit, and so do
// the candidates' forms with their decoder's arguments; the workspace is refused in the words of the entry's own query.
static int frames_keypoints(const char* who, bool with_cov, esahrnet_handle h, const FramesArgs& a, int abi_decoder,
                            const Request& r, bool refined = false) {
    const bool gaussfit = r.decoder == DEC_GAUSSFIT;
    if (!h || !a.frames || !a.det_boxes || !r.kp || (gaussfit && !r.status) || !a.crop_boxes || !a.rates || !a.valid || !a.ws)
        return set_error("%s: null argument", who);
    if (check_frames_args(who, a)) return 1;
    if (with_cov && esa::check_cov_args(who, r.cov, r.info, r.cov_floor)) return 1;
    if (refined ? check_refined_request(who, r, abi_decoder) : r.decoder == DEC_CAND && check_candidates_request(who, r)) return 1;
    if (!h->committed) return set_error("%s: esahrnet_commit has not been called", who);
    if (gaussfit && check_gaussfit_outputs(who, *h, r)) return 1;
    size_t need = 0;
    if (r.decoder == DEC_CAND ? frames_workspace_bytes(who, h, a.m, a.scale, DEC_CAND, &need, r.refine)
        : gaussfit ? esahrnet_frames_keypoints_gaussfit_workspace_bytes(h, a.m, a.scale, &need)
                 : esahrnet_frames_keypoints_workspace_bytes(h, a.m, a.scale, abi_decoder, &need))
        return 1;
    if (check_workspace(who, a.ws, a.ws_bytes, need)) return 1;
    return frames_run(who, h, a, r);
}

int esahrnet_frames_keypoints(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w, int pixel_format,
                              const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale, int rule, float mean,
                              float stdv, int decoder, void* kp_dev, void* idx_dev, void* crop_boxes_dev, void* rates_dev,
                              void* valid_dev, void* ws_dev, size_t ws_bytes, esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints", false, h, a, decoder,
                            make_request(decoder == 1 ? DEC_FINAL2 : DEC_FINAL, kp_dev, idx_dev));
}

int esahrnet_frames_keypoints_gaussfit(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                       int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                       int rule, float mean, float stdv, void* kp_dev, void* idx_dev, void* fit_dev, void* status_dev,
                                       void* hess_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* ws_dev,
                                       size_t ws_bytes, esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints_gaussfit", false, h, a, 0,
                            make_request(DEC_GAUSSFIT, kp_dev, idx_dev, hess_dev, fit_dev, status_dev));
}

int esahrnet_frames_keypoints_gaussfit_cov(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                           int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                           int rule, float mean, float stdv, void* kp_dev, void* idx_dev, void* fit_dev,
                                           void* status_dev, void* hess_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev,
                                           void* cov_dev, void* info_dev, double cov_floor, void* ws_dev, size_t ws_bytes,
                                           esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints_gaussfit_cov", true, h, a, 0,
                            make_request(DEC_GAUSSFIT, kp_dev, idx_dev, hess_dev, fit_dev, status_dev, cov_dev, info_dev, cov_floor));
}

int esahrnet_frames_keypoints_candidates(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                         int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                         int rule, float mean, float stdv, int candidates, int nms_radius, void* cand_dev,
                                         void* cidx_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* ws_dev,
                                         size_t ws_bytes, esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints_candidates", false, h, a, 0,
                            make_candidates_request(cand_dev, cidx_dev, candidates, nms_radius));
}

// esahrnet_frames_keypoints_candidates with the refined candidates' forward in the place of the plain one
int esahrnet_frames_keypoints_candidates_refined(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                                 int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m,
                                                 int scale, int rule, float mean, float stdv, int candidates, int nms_radius,
                                                 int decoder, void* cand_dev, void* cidx_dev, void* hess_dev, void* fit_dev,
                                                 void* status_dev, void* cov_dev, void* info_dev, double cov_floor,
                                                 void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* ws_dev, size_t ws_bytes,
                                                 esahrnet_stream stream) {
    const FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                       crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    return frames_keypoints("frames_keypoints_candidates_refined", false, h, a, decoder,
                            make_request(DEC_CAND, cand_dev, cidx_dev, hess_dev, fit_dev, status_dev, cov_dev, info_dev, cov_floor,
                                         candidates, nms_radius, decoder), true);
}

// ---- keypoints -> correspondences for the pose solver (correspond.hip) --------------------------------------------------
int esahrnet_frames_correspondences_workspace_bytes(esahrnet_handle h, int m, int scale, int decoder, int mode, size_t* bytes) {
    if (!h || !bytes) return set_error("frames_correspondences_workspace_bytes: null argument");
    if (esa::check_corr_args("frames_correspondences", m, h->cfg.num_keypoints, mode)) return 1;
    if (mode == 1 && decoder == 0)
        return set_error("frames_correspondences: mode 1 (Hessian weights) needs decoder 1: get_final (decoder 0) computes no Hessian");
    size_t fk = 0;
    if (esahrnet_frames_keypoints_workspace_bytes(h, m, scale, decoder, &fk)) return 1;
    *bytes = pad256(fk) + (mode == 1 ? pad256((size_t)m * h->cfg.num_keypoints * 3 * sizeof(double)) : 0);
    return 0;
}

int esahrnet_frames_correspondences(esahrnet_handle h, const void* frames_dev, int nframes, int frame_h, int frame_w,
                                    int pixel_format, const void* det_boxes_dev, const void* frame_idx_dev, int m, int scale,
                                    int rule, float mean, float stdv, int decoder, double thresh, int min_k, int mode, void* kp_dev,
                                    void* idx_dev, void* crop_boxes_dev, void* rates_dev, void* valid_dev, void* count_dev,
                                    void* order_dev, void* pts_dev, void* w_dev, void* ws_dev, size_t ws_bytes,
                                    esahrnet_stream stream) {
    const char* who = "frames_correspondences";
    if (!h || !frames_dev || !det_boxes_dev || !kp_dev || !crop_boxes_dev || !rates_dev || !valid_dev || !count_dev || !order_dev ||
        !pts_dev || !w_dev || !ws_dev)
        return set_error("%s: null argument", who);
    // everything that can be refused is refused here, before the first launch
    FramesArgs a{frames_dev, nframes, frame_h, frame_w, pixel_format, det_boxes_dev, frame_idx_dev, m, scale, rule, mean, stdv,
                 crop_boxes_dev, rates_dev, valid_dev, ws_dev, ws_bytes, stream};
    if (check_frames_args(who, a)) return 1;
    if (!h->committed) return set_error("%s: esahrnet_commit has not been called", who);
    size_t need = 0, fk = 0;
    if (esahrnet_frames_correspondences_workspace_bytes(h, m, scale, decoder, mode, &need) ||
        esahrnet_frames_keypoints_workspace_bytes(h, m, scale, decoder, &fk))
        return 1;
    if (check_workspace(who, ws_dev, ws_bytes, need)) return 1;
    a.ws_bytes = pad256(fk);                       // the loader's share; the Hessians of mode 1 lie behind it
    void* hess = mode == 1 ? static_cast<char*>(ws_dev) + a.ws_bytes : nullptr;
    if (frames_run(who, h, a, make_request(decoder == 1 ? DEC_FINAL2 : DEC_FINAL, kp_dev, idx_dev, hess))) return 1;
    const int rc = esa::launch_correspond(static_cast<const float*>(kp_dev), static_cast<const double*>(hess),
                                          static_cast<const int*>(crop_boxes_dev), static_cast<const double*>(rates_dev),
                                          static_cast<const int*>(valid_dev), m, h->cfg.num_keypoints, thresh, min_k, mode,
                                          static_cast<int*>(count_dev), static_cast<int*>(order_dev), static_cast<double*>(pts_dev),
                                          static_cast<double*>(w_dev), static_cast<hipStream_t>(stream));
    if (rc) return set_error("%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)rc));
    return 0;
}

}  // extern "C"
