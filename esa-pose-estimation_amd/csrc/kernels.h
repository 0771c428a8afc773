// kernels.h — host-side launchers of the HIP kernels (internal; the public ABI is include/esahrnet.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace esa {

// tensor formats of the internal activations (sb.h): split-bf16 NHWC, single bf16 NHWC, plain f32 NHWC, single fp16 NHWC
// (HF: the BF layout with IEEE binary16 elements — wherever a comment says "BF tensors" of a launcher that takes a
// format, HF tensors are served the same way by the fp16 instantiation of the same kernel)
enum { FMT_SB = 0, FMT_BF = 1, FMT_F32 = 2, FMT_HF = 3 };
inline bool fmt_half(int fmt) { return fmt == FMT_BF || fmt == FMT_HF; }       // 2 bytes per channel, channels padded to 64

// thread-local error text behind esahrnet_last_error() (plan.hip; abi_decode.hip and op_abi.hip report through it); returns 1 so
// that `return set_error(...)` reads well
int set_error(const char* fmt, ...);

// ---- implicit-GEMM convolution on MFMA (conv_mfma.hip) -------------------------------------
struct ConvParams {
    const char* x;      // SB input  [N][H][W][Cinp]
    char* y;            // SB output [N][OH][OW][Coutp]
    const char* res;    // SB residual (same shape as y) or nullptr
    const uint4* w;     // packed split-bf16 weights, fragment order (see pack_conv_weights)
    const float* bias;  // f32 [Coutp]
    int N, H, W, OH, OW;
    int Cinp, Coutp;    // multiples of 32
    int relu;
    int out_f32;        // 0: y is SB; 1: y is plain f32 NHWC [N][OH][OW][Coutp] (head terms t_b; FMT_BF: the stride-1 3x3
                        //    without residual only, conv_s2c32_f32out_kernel — seg_hrnet3's output layer)
    int fmt;            // FMT_SB; FMT_BF: x, y, res are BF tensors (single bf16, sb.h), Cinp / Coutp multiples of 64, weights
                        //    packed by pack_conv_weights_bf, served by the stream kernel (3x3) and conv1x1 only; FMT_F32: plain
                        //    f32 NHWC tensors, weights packed by pack_conv_weights_x6, served by conv_x6.hip (bf16x6 arithmetic)
    // multi-head form (stream kernel, stride 2 only): several convolutions of the SAME input evaluated in one launch —
    // w / bias are the members' packed weights / biases concatenated along cout, Coutp their total, and head h
    // (couts hb[h] .. hb[h+1]-1 of the concatenation, multiples of 32) goes to its own SB tensor yh[h] of
    // hb[h+1]-hb[h] channels with its own ReLU flag.  nheads <= 1: the plain form above (y, relu).
    int nheads;
    int x6_reload;      // FMT_F32, conv_x6.hip: 1 keeps the weight-reloading step loop where the launch would take the resident-
                        //    weights body (plan switch ESAHRNET_X6_RELOAD_WEIGHTS); same bits either way
    char* yh[3];
    int hb[4];
    int hrelu[3];
};
// multi-head stride-2 3x3 (see ConvParams); every head must satisfy conv_s2c32_supported on its own
bool conv_s2c32_multi_supported(const ConvParams& p);
int launch_conv_s2c32_multi(const ConvParams& p, hipStream_t stream);
// k in {1,3}, stride in {1,2}, pad = (k-1)/2.  Returns hipError_t as int.
int launch_conv(const ConvParams& p, int k, int stride, hipStream_t stream);
// name of the kernel launch_conv() runs for these parameters (only shapes / flags / res != nullptr are looked at)
const char* conv_kernel_name(const ConvParams& p, int k, int stride);
// 3x3 stride-2, Cinp == 32, no residual: weights in registers, one cout tile per wave (conv_s2c32.hip)
bool conv_s2c32_supported(const ConvParams& p);
int launch_conv_s2c32(const ConvParams& p, hipStream_t stream);
int launch_conv_s1w(const ConvParams& p, hipStream_t stream);
bool conv_is_stream_s1(const ConvParams& p);       // launch_conv(p, 3, 1) runs the stride-1 stream kernel
// 2..4 independent 3x3 convolutions of one stride (each one a stream-kernel launch on its own) as ONE launch
bool conv_jobs_supported(const ConvParams* ps, int n, int stride);
int launch_conv_jobs(const ConvParams* ps, int n, int stride, hipStream_t stream);
bool use_th16(const ConvParams& p);               // stride-1 stream kernel: 16-row tile, one workgroup per CU (conv_s2c32.hip)
void set_stream_launch_limit(long long bytes);     // test hook, see conv_s2c32.hip images_per_launch
// 1x1, Cinp in {64..384}: all input channels of 16 pixels in registers, weights streamed through LDS (conv1x1.hip)
bool conv1x1_supported(const ConvParams& p);
int launch_conv1x1(const ConvParams& p, hipStream_t stream);
// 2..6 independent 1x1 convolutions (split format, 64 / 128 / 256 input channels) as ONE launch
bool conv1x1_jobs_supported(const ConvParams* ps, int n);
int launch_conv1x1_jobs(const ConvParams* ps, int n, hipStream_t stream);
// bytes of the packed weight image for a conv with padded channel counts
size_t packed_weight_bytes(int coutp, int cinp, int k);
// host-side packing: w f32 [cout][cin][k][k] -> dst (packed_weight_bytes), zero padded
void pack_conv_weights(const float* w, int cout, int cin, int k, int coutp, int cinp, void* dst);
// BF mode: [cout16 tile][cin64 block][tap][K-step 0|1][lane][8 x bf16], lane l holding
// W[tile*16 + (l&15)][block*64 + step*32 + 8*(l>>4) + j] rounded to bf16 — same fragment count and order as the
// split format has for twice the channels per block
size_t packed_weight_bytes_bf(int coutp, int cinp, int k);
// half = true: fp16 elements (FMT_HF) in the same order
void pack_conv_weights_bf(const float* w, int cout, int cin, int k, int coutp, int cinp, void* dst, bool half = false);
// f32 -> IEEE binary16 bits on the host (round to nearest even, subnormals kept, inf beyond 65504 + half an ulp); is the
// rounded value finite?
uint16_t host_f16(float f);
bool host_f16_finite(float f);

// bf16x6 mode (conv_x6.hip): [cout16 tile][cin32 chunk][tap][term 0..2][lane][8 x bf16], every weight split exactly into
// three bf16 terms, K order inside a chunk as the staging threads load it (x6_chan_of_k)
size_t packed_weight_bytes_x6(int coutp, int cinp, int k);
void pack_conv_weights_x6(const float* w, int cout, int cin, int k, int coutp, int cinp, void* dst);
// 3x3 stride 1 / 2 and 1x1 on FMT_F32 tensors in bf16x6 arithmetic
bool conv_x6_supported(const ConvParams& p, int k, int stride);
int launch_conv_x6(const ConvParams& p, int k, int stride, hipStream_t stream);
const char* conv_x6_kernel_name(const ConvParams& p, int k, int stride);
// 2..6 independent convolutions of one kernel size and stride on FMT_F32 tensors as ONE launch (conv_x6_jobs_kernel)
bool conv_x6_jobs_supported(const ConvParams* ps, int n, int k, int stride);
int launch_conv_x6_jobs(const ConvParams* ps, int n, int k, int stride, hipStream_t stream);
void set_x6_grid_limit(int workgroups);            // test hook: workgroups per tile-stream launch (<= 0: the device's slots)
// 1x1 with all input channels of a wave's pixels in registers (<= 256 input channels, no residual); launch_conv_x6 routes here
bool conv1x1_x6_supported(const ConvParams& p);
int launch_conv1x1_x6(const ConvParams& p, hipStream_t stream);
int launch_conv1x1_x6_jobs(const ConvParams* ps, int n, hipStream_t stream);
// does launch_conv_x6_jobs(k = 1) run the register-resident 1x1 kernel (conv1x1_x6_jobs_kernel) for these members?
bool conv1x1_x6_jobs_supported(const ConvParams* ps, int n);

// ---- stem conv1: f32 NCHW -> SB, 3x3 s1, cin in {1..4}, cout = multiple of 32 (stem.hip) ---
struct StemParams {
    const float* x;     // f32 [N][cin][H][W]
    char* y;            // SB [N][H][W][cout]
    const float* w;     // f32 [cout/8][cin][9][8]  (repacked: 8 consecutive couts innermost)
    const float* bias;  // f32 [cout]
    int N, H, W, cin, cout;
    int relu;           // 0: raw conv output (seg_hrnet3 keeps the pre-BN conv1 tensor for its skip)
    int fmt;            // format of y (FMT_BF: cout = padded channel count, multiple of 64)
};
int launch_stem(const StemParams& p, hipStream_t stream);
// the same convolution + the per-channel (sum, max) of the output over slabs of pixels, in pool_partial's layout
// [N][slabs][cout][2] (cbam.hip); stem_pool_slabs: slabs per image, 0 = not available (needs cin 1, cout 64).  The partials
// are of the values the tensor holds (FMT_BF: rounded to bf16; FMT_SB: hi + lo)
int stem_pool_slabs(int cin, int cout, int H, int W);
int launch_stem_pool(const StemParams& p, float* pool, hipStream_t stream);

// ---- fused BasicBlock of the 32-channel branch (bblock32.hip) -------------------------------------
struct BlockParams {
    const char* x;      // SB [N][H][W][32]
    char* y;            // SB [N][H][W][32]
    const uint4* w1;    // packed 3x3 32->32 weights of conv1 / conv2 (pack_conv_weights)
    const uint4* w2;
    const float* bias1; // f32 [32]
    const float* bias2; // f32 [32]
    int N, H, W;
};
int launch_bblock32(const BlockParams& p, hipStream_t stream);

// ---- fused stem: conv1 (VALU, recomputed per tile) -> conv2 3x3 s2 (MFMA) (stem_fused.hip) -------
struct StemFusedParams {
    const float* x;     // f32 [N][cin][H][W]
    char* y;            // SB [N][OH][OW][Coutp]
    const float* w1;    // f32 [Cmid/8][cin][9][8]   (same image as StemParams::w)
    const float* bias1; // f32 [Cmid]
    const uint4* w2;    // packed conv2 weights (pack_conv_weights, k = 3)
    const float* bias2; // f32 [Coutp]
    int N, H, W, OH, OW, cin, Cmid, Coutp;
};
int launch_stem_fused(const StemFusedParams& p, hipStream_t stream);
// fp32-grade mode (conv_x6.hip): x f32 NCHW, y f32 NHWC, w1 = pack_stem_w1_x6 image (conv1 folded weights + bias, 640 floats),
// w2 = pack_conv_weights_x6 of conv2; cin == 1 only
bool stem_fused_x6_supported(int cin, int cmid, int coutp);
void pack_stem_w1_x6(const float* w, const float* b, float* dst);
int launch_stem_fused_x6(const StemFusedParams& p, hipStream_t stream);

// ---- cross-resolution fuse: y = relu?(sum_i up(x_i)) on SB tensors (fuse.hip) ---------------
struct FuseParams {
    const char* x[4];
    int h[4], w[4];     // source resolution of each term (== H,W for same-resolution terms)
    int nterms;
    char* y;
    int N, H, W, Cp;
    int relu;
    int fmt;            // format of all tensors
};
int launch_fuse(const FuseParams& p, hipStream_t stream);

// ---- head tail: up x2 (align_corners=True) + concat raw input + 3x3 conv -> f32 NCHW (head.hip)
struct FinalParams {
    const char* h3;     // SB [N][H/2][W/2][Cp]  (last_layer.3 output, K valid channels)
    const float* x0;    // f32 [N][cin][H][W]
    float* out;         // f32 [N][K][H][W]
    const float* w;     // f32 [K+cin][9][K]   (repacked: output channel innermost)
    const float* bias;  // f32 [K] (padded with zeros to 32)
    const uint4* wpk;   // MFMA path: split-bf16 fragments (pack_final_mfma), or nullptr -> VALU kernel
    int N, H, W, h, wd; // h,wd = resolution of h3
    int K, cin, Cp;
    int fmt;            // format of h3 (FMT_F32: VALU kernel only)
    float2* part;       // optional (MFMA kernel only): [N*K][final_part_tiles] (value, index bits) of every tile's first maximum;
                        // launch_final_kp: [N*K][final_kp_tiles], its scratch
};
int launch_final(const FinalParams& p, hipStream_t stream);
// keypoints without heat-maps, VALU output layer (final_kernel<KT, RPT, true> + final_kp_finish_kernel): kp f32 [N*K][3], idx_out int32
// [N*K] or nullptr, bit-identical to launch_final (VALU) + launch_keypoints; p.out is not used
int final_kp_tiles(int K, int cin, int H, int W);
int launch_final_kp(const FinalParams& p, float* kp, int* idx_out, hipStream_t stream);
// the Gaussian-fit decoder without heat-maps, VALU output layer (final_kernel<KT, RPT, true> + final_gf_finish_kernel): kp, idx_out
// (may be null), fit f64 [N*K][8] (may be null), status int32 [N*K], hess f64 [N*K][3] (may be null) bit-identical to launch_final
// (VALU) + launch_keypoints_gaussfit; p.part: [N*K][final_kp_tiles], p.out not used; cin <= 8
int launch_final_gf(const FinalParams& p, float* kp, int* idx_out, double* fit, int* status, double* hess, hipStream_t stream);
// the same with cov / info f64 [N*K][3] (gaussfit.h COV; final_gfcov_finish_kernel); both null: launch_final_gf's kernels
int launch_final_gf_cov(const FinalParams& p, float* kp, int* idx_out, double* fit, int* status, double* hess, double* cov,
                        double* info, double cov_floor, hipStream_t stream);
// get_final2 keypoints without heat-maps, VALU output layer (final2_valu_kernel + final2_valu_finish_kernel): kp / idx_out
// bit-identical to launch_final (VALU) + launch_keypoints_final2; p.part and bmax: [N*K][final2_valu_tiles] records, p.out
// not used; cin <= 8
int final2_valu_tiles(int H, int W);
// hess (may be null): f64 [N*K][3] = (dxx, dxy, dyy), the Hessian each step used, NaN x 3 where no step is taken
int launch_final2_kp(const FinalParams& p, float* bmax, float* kp, int* idx_out, hipStream_t stream, double* hess = nullptr);
// tiles per heat-map the MFMA output-layer kernel reports partial maxima for; 0: that kernel does not serve (K, cin)
int final_part_tiles(int K, int cin, int H, int W);
// (v, i) beats (bv, bi) if it is larger — NaN counting as larger than every number — or equal with a lower index
// (np.argmax / torch.max: first row-major maximum, first NaN)
__device__ __forceinline__ void argmax_take(float v, int i, float& bv, int& bi) {
    const bool vn = v != v, bn = bv != bv;
    if (v > bv || (vn && !bn) || ((v == bv || (vn && bn)) && i < bi)) { bv = v; bi = i; }
}
bool final_mfma_supported(int K, int cin);
size_t final_mfma_bytes(int K, int cin);
void pack_final_mfma(const float* w, int K, int cin, void* dst);

// ---- fused head: W0*x0 + sum up(t_b) + bias, ReLU, W3*(.) + bias, ReLU (head_fused.hip) ----------
struct HeadParams {
    const char* x0;     // SB [N][H][W][C0p]            stage-4 branch 0
    const char* t[3];   // f32 NHWC [N][th][tw][Ctp]    W_b * x_b on branch b's grid, b = 1..3
    char* y;            // SB [N][H][W][C3p]            last_layer[3..5] output
    const uint4* w0;    // packed [Ctp/16][C0p/32][hi|lo][64]   (pack_conv_weights, k = 1)
    const uint4* w3;    // packed [M3][Ctp/32][hi|lo][64]       (pack_head_w3, permuted K order)
    const float* bias0; // f32 [Ctp]
    const float* bias3; // f32 [C3p]
    int N, H, W;
    int th[3], tw[3];
    int C0p, Ctp, C3p, K;
    bool valu;          // launch_head_bf: the first-generation form (VALU interpolation) instead of the matrix-core one
    bool hf;            // launch_head_bf: x0, t[b] and y are HF tensors, w0 / w3 packed with half = true (matrix-core form only)
};
int launch_head(const HeadParams& p, hipStream_t stream);
bool head_fused_supported(int H, int W, const int th[3], const int tw[3], int C0p, int K);
size_t head_w3_bytes(int K, int Ctp);
void pack_head_w3(const float* w, int K, int Ct, int Ctp, void* dst);
// bf16 mode (head_fused_bf.hip): x0, t[b] and y are BF tensors; w0 = pack_conv_weights_bf(k = 1) of the branch-0 slice
// [Ctp/16][C0p/64][K-step][64], w3 = pack_head_w3_bf [M3][Ctp/32][64] (one bf16 fragment per chunk)
int launch_head_bf(const HeadParams& p, hipStream_t stream);
bool head_fused_bf_supported(int H, int W, const int th[3], const int tw[3], int C0p, int K);
// the calibration form (esahrnet_forward_stats_h0): the matrix-core kernel of launch_head_bf with the range of h0 — which is
// rounded in registers and never stored — beside it.  part: head_bf_range_tiles(H, W) * N partials of 8 bytes, rec: N
// esahrnet_stats_record (max_abs, max and n_ge_f16max filled, taken BEFORE the rounding; the rest zero).  Not for p.valu.
int head_bf_range_tiles(int H, int W);
int launch_head_bf_range(const HeadParams& p, void* part, void* rec, hipStream_t stream);
size_t head_w3_bf_bytes(int K, int Ctp);
void pack_head_w3_bf(const float* w, int K, int Ct, int Ctp, void* dst, bool half = false);     // half: fp16 elements (FMT_HF)

// fp32-grade mode (head_x6.hip): x0, t[b] and y are f32 NHWC tensors; w0 / w3 = pack_conv_weights_x6(k = 1) of the branch-0
// slice of last_layer[0] and of last_layer[3] (cout padded to 16 or 32)
int launch_head_x6(const HeadParams& p, hipStream_t stream);
bool head_x6_supported(int H, int W, const int th[3], const int tw[3], int C0p, int K);

// ---- second-generation fused head: bilinear up-sampling on the matrix cores (head_t.hip, head_fused2.hip)
constexpr int HT_PAD = 1;       // T layout: stored column = x + HT_PAD
struct HeadTParams {
    const char* x;      // SB [N][h][w][Cinp]                      branch b activations
    char* t;            // T layout [N][h][Ctp/32][hi|lo][32][XP] bf16   t_b = W_b * x_b
    const uint4* wt;    // packed [Ctp/16][Cinp/32][hi|lo][64]     (pack_conv_weights, k = 1)
    int N, h, w, Cinp, Ctp, XP;
};
int launch_head_t(const HeadTParams& p, hipStream_t stream);
int head_t_xp(int w);                       // row pitch (pixels) of the T layout for a w-pixel row
bool head_t_supported(int Cinp);
struct Head2Params {
    const char* x0;     // SB [N][H][W][C0p]            stage-4 branch 0
    const char* x1;     // SB [N][th0][tw0][C1p]        stage-4 branch 1
    const char* t2;     // T layout, branch 2
    const char* t3;     // T layout, branch 3
    char* y;            // SB [N][H][W][C3p]
    const uint4* w0;    // packed [Ctp/16][C0p/32][hi|lo][64]
    const uint4* w1;    // packed [Ctp/16][C1p/32][hi|lo][64]
    const uint4* w3;    // packed [M3][Ctp/32][hi|lo][64]  (pack_head_w3)
    const float* bias0; // f32 [Ctp]
    const float* bias3; // f32 [C3p]
    int N, H, W;
    int th[3], tw[3];   // grids of branches 1..3
    int xp2, xp3;       // T-layout row pitches
    int C0p, C1p, Ctp, C3p, K;
};
int launch_head2(const Head2Params& p, bool ulo, hipStream_t stream);
bool head_fused2_supported(int H, int W, const int th[3], const int tw[3], int C0p, int C1p, int K, bool* ulo);

// ---- CBAM attention of the seg_hrnet3 variant + slice re-sampling (cbam.hip) --------------------
int launch_pool_partial(const char* x, float* partial, int N, int HW, int Cp, int P, hipStream_t s, int fmt = FMT_SB);
int launch_ca_mlp(const float* partial, const float* w0, const float* w2, float* ca, int N, int HW, int C,
                  int Cp, int Cr, int P, hipStream_t s);
int launch_cbam_maps(const char* x, const float* ca, float* maps, int N, int HW, int C, int Cp, hipStream_t s, int fmt = FMT_SB);
struct CbamApplyParams {
    const char* x;      // SB [N][H][W][Cp]
    const char* res;    // SB same shape or nullptr
    const float* ca;    // f32 [N][Cp]   channel attention
    const float* maps;  // f32 [N][H][W][2]  (mean_c, max_c) of ca*x
    const float* w_sa;  // f32 [2][7][7]
    char* y;            // SB, pixel pitch y_pix_bytes, written at channel offset y_c0 (multiple of 8)
    int N, H, W, Cp, y_pix_bytes, y_c0, relu;
    int C;              // real channels (cbam_spatial only: it forms the maps itself and ignores `maps`)
    int fmt = FMT_SB;   // FMT_SB, FMT_F32 or FMT_BF (x, res and y alike; BF: 8 channels = 16 bytes, y_pix_bytes = Cp * 2)
};
int launch_cbam_apply(const CbamApplyParams& p, hipStream_t s);
// maps + apply in one pass (no `maps` tensor); Cp / 8 must be a power of two <= 32
bool cbam_spatial_supported(int Cp);
int launch_cbam_spatial(const CbamApplyParams& p, hipStream_t s);
// one launch for the same CBAM step of up to four tensors (the branches of an HRModule at one depth)
enum { CBAM_POOL = 0, CBAM_MLP = 1, CBAM_MAPS = 2, CBAM_APPLY = 3, CBAM_SPATIAL = 4 };
constexpr int CBAM_MAXJOBS = 4;
struct CbamJob {
    int kind;
    CbamApplyParams ap;         // every kind: x, N, H, W, Cp, C (+ the rest for APPLY / SPATIAL; ca for MAPS)
    float* partial;             // POOL (out), MLP (in)
    const float* w0; const float* w2; float* ca;        // MLP
    float* maps;                // MAPS (out)
    int HW, P, Cr;
    int tiles_x, tiles_y;       // filled by the launcher
};
struct CbamJobs { CbamJob j[CBAM_MAXJOBS]; int start[CBAM_MAXJOBS + 1]; int n; };
int launch_cbam_jobs(const CbamJob* jobs, int n, hipStream_t s);
// workgroups job `q` needs (the grid its own launch would use; fills tiles_x / tiles_y); -1: no CBAM kernel serves it.  The
// predicates are those of every CBAM launcher, single or merged, and depend on the shape, never on the batch.
long long cbam_job_blocks(CbamJob& q);
struct ResampleParams {
    const char* x;      // SB [N][h][w][Cp_src]
    char* y;            // SB [N][H][W][..], pixel pitch y_pix_bytes, channel offset y_c0 (multiple of 8)
    int N, h, w, H, W, C, Cp_src, y_pix_bytes, y_c0;
    int align;          // 1: align_corners=True, 0: False (irrelevant when h==H && w==W: copy)
    int fmt = FMT_SB;   // FMT_SB, FMT_F32 or FMT_BF (x and y alike)
};
int launch_resample_slice(const ResampleParams& p, hipStream_t s);
int launch_zero_slice(char* y, long long npix, int y_pix_bytes, int c0, int nchan, hipStream_t s, int fmt = FMT_SB);

// ---- seg_hrnet3 head: low-resolution branches' share of last_layer[0] (head_gather.hip) ----
struct GatherParams {
    const char* z[2];   // SB [N][h][w][zpix / 4]: the nine 1x1 products per output channel, channel (cout/8)*72 + tap*8 + cout%8
    char* y;            // SB [N][H][W][Cp]
    int N, H, W, C, Cp;                 // C real output channels, Cp padded (the padding is written as zeros)
    int h[2], w[2], zpix[2];
    int R[2], Cc[2], ngroups, nreal, gpw;      // filled by the launcher
};
bool head_gather_supported(int H, int W, const int* h, const int* w, int Cp);
int launch_head_gather(GatherParams p, hipStream_t stream, int fmt = FMT_SB);      // fmt of y: FMT_SB or FMT_F32 (z is plain f32 in both)

// ---- arg-max + log-quadratic refine (keypoints.hip) ----------------------------------------
// idx_out: optional int32 [planes], the flat index (row * W + column) of the arg-max
int launch_keypoints(const float* heat, int planes, int H, int W, float* kp, int* idx_out, hipStream_t stream);
// the M best peaks per plane (keypoints_candidates.hip): cand f32 [planes][M][3], cidx int32 [planes][M] or nullptr; row 0 is
// launch_keypoints' row, rows m >= 1 the best local maxima at Chebyshev distance > r from every earlier one (NaN x 3, -1: none)
int launch_keypoints_candidates(const float* heat, int planes, int H, int W, int M, int r, float* cand, int* cidx,
                                hipStream_t stream);
// the same bits from one sweep and a table of per-cell bests (keypoints_candidates_onepass.hip), on eligible planes: heat 16-byte
// aligned, W a multiple of 4, at most kOnepassMaxCells cells of 8 x 8 pixels; hipErrorInvalidValue on any other plane
constexpr int kOnepassMaxCells = 4096;
// launch_keypoints_candidates_auto (the fused paths, form -1) runs the one-sweep kernel on an eligible plane from this M on: its
// slowest window beat the multi-sweep kernel's fastest at M = 2, 3 and 4; at M = 1, where there is no runner-up to find, its
// sweep costs twice the multi-sweep kernel's
constexpr int kOnepassFromM = 2;
bool keypoints_candidates_onepass_eligible(const float* heat, int H, int W);
int launch_keypoints_candidates_onepass(const float* heat, int planes, int H, int W, int M, int r, float* cand, int* cidx,
                                        hipStream_t stream);
int launch_keypoints_candidates_auto(const float* heat, int planes, int H, int W, int M, int r, float* cand, int* cidx,
                                     hipStream_t stream);
// same result from the per-tile maxima of the output-layer kernel (FinalParams::part, `ntiles` pairs per plane)
int launch_keypoints_finish(const float* heat, const float2* part, int ntiles, int planes, int H, int W, float* kp, int* idx_out,
                            hipStream_t stream);
// the same finish on NHWC heat-maps x [N][H][W][Cp] (fmt FMT_SB or FMT_F32) that were never converted to NCHW; part from
// launch_tile_max, planes = N * C
int launch_keypoints_finish_nhwc(int fmt, const char* x, int N, int C, int H, int W, int Cp, const float2* part, int ntiles,
                                 float* kp, int* idx_out, hipStream_t stream);

// ---- get_final2: 11x11 Gaussian blur, rescale, log, full-Hessian Newton step (keypoints_final2.hip) -------------------
// Same kp / idx_out layout, arg-max and peak as launch_keypoints.  ws: final2_workspace_bytes, 256-byte aligned (per-tile
// maxima of the raw and of the blurred planes; the blurred planes themselves are never stored).
int final2_tiles(int H, int W);
size_t final2_workspace_bytes(long long planes, int H, int W);
// hess (may be null): f64 [planes][3] = (dxx, dxy, dyy) of the blurred log heat-map, the values the step uses; NaN x 3 where no
// step is taken.  A template flag of the finish: with hess == nullptr the kernels launched are the ones without it.
int launch_keypoints_final2(const float* heat, int planes, int H, int W, float* kp, int* idx_out, void* ws, size_t ws_bytes,
                            hipStream_t stream, double* hess = nullptr);
// the same decoder on NHWC heat-maps x [N][H][W][Cp] (fmt FMT_SB or FMT_F32) that were never converted to NCHW: seg_hrnet3
// under esahrnet_forward_keypoints_final2; planes = N * C, ws as above
int launch_keypoints_final2_nhwc(int fmt, const char* x, int N, int C, int H, int W, int Cp, float* kp, int* idx_out, void* ws,
                                 size_t ws_bytes, hipStream_t stream, double* hess = nullptr);

// launch_keypoints_final2 with hess (not null), keypoints_final2_hess.hip: the same tile pass, the finish instantiated with
// the Hessian output
int launch_keypoints_final2_hess(const float* heat, int planes, int H, int W, float* kp, int* idx_out, double* hess, void* ws,
                                 size_t ws_bytes, hipStream_t stream);

// ---- the third decoder: a 2-D Gaussian fitted to the 13 x 13 window around the arg-max (keypoints_gaussfit.hip) -----------
// launch_keypoints (unchanged: kp rows and the arg-max index), then gaussfit_kernel, one wave per plane: fit f64 [planes][8] =
// (A, x0, y0, a, b, c, off, cost), status int32 [planes] (0 accepted, 1 / 2 / 3 rejected), hess f64 [planes][3] = (-2a, -2b,
// -2c); fit, hess and idx_out may be null (without idx_out the index passes through status).  An accepted fit replaces x, y.
int launch_keypoints_gaussfit(const float* heat, int planes, int H, int W, float* kp, int* idx_out, double* fit, int* status,
                              double* hess, hipStream_t stream);
// the fit alone (gaussfit_kernel): idx_in int32 [planes] and the kp rows as launch_keypoints / launch_keypoints_finish left them
int launch_gaussfit_fit(const float* heat, const int* idx_in, int planes, int H, int W, float* kp, double* fit, int* status,
                        double* hess, hipStream_t stream);
// the fit alone on NHWC heat-maps x [N][H][W][Cp] (fmt FMT_SB or FMT_F32) behind launch_keypoints_finish_nhwc; planes = N * C
int launch_gaussfit_fit_nhwc(int fmt, const char* x, int N, int C, int H, int W, int Cp, const int* idx_in, float* kp, double* fit,
                             int* status, double* hess, hipStream_t stream);
// the three with the covariance of the fitted centre (keypoints_gaussfit_cov.hip; gaussfit.h COV): cov f64 [planes][3] = s^2 (J^T
// J)^-1's (x0, y0) block, crop px^2, and info f64 [planes][3] = -cov^-1, NaN x 3 also where cov[0] < cov_floor (either may be null;
// both null: the launches above, nothing else).  kp, idx, fit, status, hess: the bits of the launches above.  cov_floor >= 0.
int launch_keypoints_gaussfit_cov(const float* heat, int planes, int H, int W, float* kp, int* idx_out, double* fit, int* status,
                                  double* hess, double* cov, double* info, double cov_floor, hipStream_t stream);
int launch_gaussfit_fit_cov(const float* heat, const int* idx_in, int planes, int H, int W, float* kp, double* fit, int* status,
                            double* hess, double* cov, double* info, double cov_floor, hipStream_t stream);
int launch_gaussfit_fit_nhwc_cov(int fmt, const char* x, int N, int C, int H, int W, int Cp, const int* idx_in, float* kp,
                                 double* fit, int* status, double* hess, double* cov, double* info, double cov_floor,
                                 hipStream_t stream);

// ---- crop + edge-pad + 8-bit bilinear resize + normalise: u8 frames -> f32 [N][1][S][S] (crops.hip) ----
int launch_crops(const unsigned char* frames, const int* boxes, float* out, int N, int FH, int FW, int S,
                 float mean, float std_, hipStream_t s);

// ---- the loader on the device (frontend.hip) ------------------------------------------------------------------------
// det int32 [m][4] detector boxes (x, y, x2, y2) -> crop int32 [m][4] (x_new, y_new, w_new, h_new), rates f64 [m], valid
// int32 [m]; rule 0: data_load_val.py:127-158, 1: data_load4.py:112-141.  frame_idx (may be null): a crop whose frame index
// is outside [0, nframes) is invalid too.
int launch_boxes(const int* det, const int* frame_idx, int nframes, int m, int FH, int FW, int S, int rule, int* crop,
                 double* rates, int* valid, hipStream_t s);
// launch_crops with a frame index per crop (null: identity), rgb = 1: RGB8 interleaved frames reduced by PIL's convert('L'),
// and zeros for crops with valid[i] == 0 (valid may be null), a frame index out of range or a box outside the frame.
// m * S <= 2^24 - 1 (one block per output row)
int launch_crops_ex(const unsigned char* frames, int nframes, int FH, int FW, int rgb, const int* frame_idx, const int* boxes,
                    const int* valid, float* out, int m, int S, float mean, float std_, hipStream_t s);
// kp f32 [m][K][3] -> NaN and idx int32 [m][K] (may be null) -> -1 in the rows with valid[i] == 0
int launch_mark_invalid(const int* valid, int m, int K, float* kp, int* idx, hipStream_t s);
// the same for the Gaussian-fit decoder's outputs: also fit f64 [m][K][8] and hess f64 [m][K][3] (may be null) -> NaN, status
// int32 [m][K] -> -1
int launch_mark_invalid_gaussfit(const int* valid, int m, int K, float* kp, int* idx, double* fit, int* status, double* hess,
                                 hipStream_t s);
// the same plus cov and info f64 [m][K][3] (may be null) -> NaN (mark_invalid_gfcov_kernel)
int launch_mark_invalid_gaussfit_cov(const int* valid, int m, int K, float* kp, int* idx, double* fit, int* status, double* hess,
                                     double* cov, double* info, hipStream_t s);
// the refined candidates' outputs (mark_invalid_refined_kernel), one thread per slot of [m][K * M]: cand f32 [..][3] -> NaN; cidx
// and status int32 [..] -> -1; hess, cov, info f64 [..][3] and fit f64 [..][8] -> NaN.  Every pointer but cand may be null
int launch_mark_invalid_refined(const int* valid, int m, int slots, float* cand, int* cidx, int* status, double* hess, double* fit,
                                double* cov, double* info, hipStream_t s);

// ---- the decoders at caller-given pixels (keypoints_at.hip): heat f32 [planes][H][W], at int32 [planes][m] -> kp f32
// [planes][m][3]; decoder 0 get_final, 1 get_final2 (ws: at_workspace_bytes, 256-byte aligned), 2 the Gaussian fit (status not
// null).  hess, fit, cov, info (f64) and status may be null where the decoder allows it; every argument has been checked
size_t at_workspace_bytes(long long planes, int H, int W, int decoder);
int launch_keypoints_at(const float* heat, int planes, int H, int W, const int* at, int m, int decoder, float* kp, double* hess,
                        double* fit, int* status, double* cov, double* info, double cov_floor, void* ws, hipStream_t stream);

// ---- keypoints -> the record the pose solver consumes (correspond.hip, correspond.h) ----------------------------------
// kp f32 [m][K][3], hess f64 [m][K][3] (mode 1; may be null in mode 0), crop / rates / valid as launch_boxes wrote them ->
// count int32 [m], order int32 [m][K], pts f64 [m][K][2], w f64 [m][K][3].  K <= 32 (one wave per crop).
int launch_correspond(const float* kp, const double* hess, const int* crop, const double* rates, const int* valid, int m, int K,
                      double thresh, int min_k, int mode, int* count, int* order, double* pts, double* w, hipStream_t s);
// the same on candidate rows: cand f32 [m][K][M][3], hess f64 [m][K][M][3] (mode 1) -> count, order as above (selection by
// candidate 0), cpts f64 [m][K][M][2], cw f64 [m][K][M][3], cpeak f32 [m][K][M] in rank order.  K <= 32, M <= 4.
int launch_correspond_cand(const float* cand, const double* hess, const int* crop, const double* rates, const int* valid, int m, int K,
                           int M, double thresh, int min_k, int mode, int* count, int* order, double* cpts, double* cw, float* cpeak,
                           hipStream_t s);

// ---- layout conversion f32 NCHW <-> SB (layout.hip) ----------------------------------------
int launch_nchw_to_sb(const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s);
int launch_sb_to_nchw(const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s);
// the same for BF tensors (single bf16 NHWC, sb.h)
int launch_nchw_to_bf(const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s);
int launch_bf_to_nchw(const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s);
// for HF tensors (single fp16 NHWC: rounded to nearest even and saturated on the way in, exact on the way out)
int launch_nchw_to_hf(const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s);
int launch_hf_to_nchw(const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s);
// and for F32 tensors (plain f32 NHWC)
int launch_nchw_to_f32(const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s);
int launch_f32_to_nchw(const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s);
// by format code
int launch_nchw_to_fmt(int fmt, const float* x, int N, int C, int H, int W, char* y, int Cp, hipStream_t s);
int launch_fmt_to_nchw(int fmt, const char* x, int N, int C, int H, int W, int Cp, float* y, hipStream_t s);
// FMT_HF only: the same conversion times `scale`, a power of two (esahrnet_tap_read under fp16 scale exponents)
int launch_hf_to_nchw_scaled(const char* x, int N, int C, int H, int W, int Cp, float* y, float scale, hipStream_t s);
// f32 / SB (fmt) NHWC heat-maps -> f32 NCHW plus each tile's first maximum, part [N*C][to_nchw_part_tiles(H, W)] (value,
// index bits) as keypoints_finish reads it; C <= 32
int to_nchw_part_tiles(int H, int W);
int launch_to_nchw_part(int fmt, const char* x, int N, int C, int H, int W, int Cp, float* y, float2* part, hipStream_t s);
// the same per-tile maxima without the NCHW copy
int launch_tile_max(int fmt, const char* x, int N, int C, int H, int W, int Cp, float2* part, hipStream_t s);

// ---- stats.hip: the activation range report (esahrnet_stats_record, include/esahrnet.h) ----------------------------------
// One tensor to scan: x [N][H][W][Cp] in format fmt (HW = H * W pixels, real channels 0..C-1), or, fmt == STATS_NCHW, plain f32
// [N][C][H][W] (Cp unused).  Its N records go to records[row * N + image].
constexpr int STATS_NCHW = -1;
struct StatsJob {
    const void* x;
    int fmt, C, Cp, HW, row;
};
// partial records per image the scan of such a tensor leaves (a function of the shape alone); 0: a shape it does not serve
int stats_parts(int fmt, int C, int Cp, int HW);
// scan + finish of njobs tensors of N images; partials: room for sum_j stats_parts(job j) * N records, 8-byte aligned
int launch_stats(const StatsJob* jobs, int njobs, int N, void* partials, void* records, hipStream_t stream);

// ---- diff.hip: the precision report (esahrnet_diff_record, include/esahrnet.h) --------------------------------------------
// One pair of tensors to compare: a [N][H][W][cp_a] in fmt_a (FMT_SB .. FMT_HF), stored times 2^-e, against b [N][H][W][cp_b]
// in FMT_F32; or fmt_a == fmt_b == STATS_NCHW: plain f32 [N][C][H][W] on both sides.  Real channels 0..C-1, HW pixels.  Its N
// records go to records[row * N + image].
struct DiffJob {
    const void* a;
    int fmt_a, cp_a;
    const void* b;
    int fmt_b, cp_b;
    int C, HW, e, row;
};
// partial records per image (a function of the shape alone); 0: a pair the scan does not serve
int diff_parts(int fmt_a, int cp_a, int fmt_b, int cp_b, int C, int HW);
// scan + finish of njobs pairs of N images; partials: room for sum_j diff_parts(job j) * N records, 8-byte aligned
int launch_diff(const DiffJob* jobs, int njobs, int N, void* partials, void* records, hipStream_t stream);

}  // namespace esa
