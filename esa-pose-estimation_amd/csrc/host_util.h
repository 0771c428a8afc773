// host_util.h — what the host files behind the C-ABI share (plan.h's units: the entries that take a handle; op_abi.hip: the
// stand-alone operator entries): the rule from a precision code to a tensor format, the plan switches' reading of the environment, uploads,
// and the scoped owner of a stand-alone entry's device memory.  Private to csrc; nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels.h"

#pragma GCC visibility push(hidden)       // shared between the library's own files: the library exports none of it
namespace esa {

inline int pad32(int c) { return (c + 31) & ~31; }
inline int pad64(int c) { return (c + 63) & ~63; }
inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }      // byte counts inside a workspace

static constexpr int POOL_SLABS = 64;              // CBAM's pooled partials: slabs per image (fewer where the image has fewer pixels)
static constexpr int STEM_POOL_SLABS_MAX = 1024;   // pooled partials of the raw stem tensor: slabs reserved per image

// an ESAHRNET_<NAME> switch: on unless unset, empty or "0"
inline bool env_on(const char* name) {
    const char* e = getenv(name);
    return e && e[0] && strcmp(e, "0") != 0;
}

// The tensor format of a precision code (0: split-bf16 'bf16x3', 1: bf16, 2: fp32-grade 'bf16x6', 3: fp16): the FMT_* code, the
// bytes of a stored channel, the multiple channel counts are padded to, and the packing of a convolution's weights.  The one
// statement of that rule; which precisions an entry serves is the entry's own business.
struct Format {
    int fmt = FMT_SB;
    bool half = false;          // 2 bytes per channel, channels padded to 64 (single bf16, sb.h "BF", or single fp16, "HF")
    bool hf = false;            // ... and the element type is fp16
    bool x6 = false;            // plain f32 tensors, bf16x6 arithmetic
    int eb = 4, cm = 32;        // bytes per stored channel; channel multiple
    Format() = default;
    explicit Format(int precision)
        : fmt(precision == 1 ? FMT_BF : precision == 2 ? FMT_F32 : precision == 3 ? FMT_HF : FMT_SB), half(fmt_half(fmt)),
          hf(fmt == FMT_HF), x6(fmt == FMT_F32), eb(half ? 2 : 4), cm(half ? 64 : 32) {}
    int pad(int c) const { return half ? pad64(c) : pad32(c); }
    size_t wbytes(int coutp, int cinp, int k) const {
        return half ? packed_weight_bytes_bf(coutp, cinp, k) : x6 ? packed_weight_bytes_x6(coutp, cinp, k) : packed_weight_bytes(coutp, cinp, k);
    }
    // w [cout][cin][k][k] packed for the format (wbytes(coutp, cinp, k) bytes)
    std::vector<char> pack(const float* w, int cout, int cin, int k, int coutp, int cinp) const {
        std::vector<char> p(wbytes(coutp, cinp, k), 0);
        if (half) pack_conv_weights_bf(w, cout, cin, k, coutp, cinp, p.data(), hf);
        else if (x6) pack_conv_weights_x6(w, cout, cin, k, coutp, cinp, p.data());
        else pack_conv_weights(w, cout, cin, k, coutp, cinp, p.data());
        return p;
    }
};

#define HIP_OK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return esa::set_error("%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// host vector -> a fresh device buffer.  Non-zero: an error is set; *dev may hold a buffer all the same (the caller frees it)
template <typename T>
int upload(const std::vector<T>& host, void** dev) {
    HIP_OK(hipMalloc(dev, host.size() * sizeof(T)));
    HIP_OK(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// what an entry refuses about its workspace of at least `need` bytes (`who` names the entry)
inline int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (ws_bytes < need) return set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    if (reinterpret_cast<uintptr_t>(ws) & 255) return set_error("%s: workspace must be 256-byte aligned", who);
    return 0;
}

// abi_decode.hip: the argument checks its handle-free entries share with the loader entries (`who` names the entry)
extern const int kFrontendMaxRows;
int check_boxes_args(const char* who, int m, int frame_h, int frame_w, int scale, int rule);
int check_crops_args(const char* who, int nframes, int pixel_format, float stdv);
int check_cov_args(const char* who, const void* cov_dev, const void* info_dev, double cov_floor);
int check_corr_args(const char* who, int m, int k, int mode);

// plan.hip: what esahrnet_commit and the plan share with the stand-alone entries
std::vector<float> pack_stem_w(const float* w, int cout, int cin, int coutp);
bool conv_group_mergeable(int fmt, const ConvParams* ps, int n, int k, int stride);
void conv_group_kernel_name(char* out, size_t cap, int fmt, const ConvParams* ps, int n, int k, int stride);

// The device memory of one stand-alone entry, bound to the entry's stream: alloc() and upload() hand out buffers, leaving the
// scope frees them all.  Two rules hold:
//   * a scope that has handed out nothing and enqueued nothing calls no HIP function (the host tests call the entries'
//     refusals on machines without a GPU);
//   * on every path where work may have been enqueued the stream is synchronised before any buffer is freed: by finish() at
//     the end of an entry, and by the destructor on every earlier exit once a buffer has been handed out (an entry enqueues
//     only on buffers of its scope, or goes straight to finish()).
class DevScope {
public:
    DevScope(const char* who, hipStream_t stream) : who_(who), stream_(stream) {}
    DevScope(const DevScope&) = delete;
    DevScope& operator=(const DevScope&) = delete;
    ~DevScope() {
        if (!bufs_.empty() && !synced_) (void)hipStreamSynchronize(stream_);
        for (void* p : bufs_) (void)hipFree(p);
    }
    hipStream_t stream() const { return stream_; }
    // *out: `bytes` of device memory.  Non-zero: "<who>: hipMalloc failed" is set
    template <typename P>
    int alloc(P** out, size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return set_error("%s: hipMalloc failed", who_);
        bufs_.push_back(p);
        *out = static_cast<P*>(p);
        return 0;
    }
    // *out: a device copy of `host`.  Non-zero: upload's error is set
    template <typename T, typename P>
    int upload(const std::vector<T>& host, P** out) {
        void* p = nullptr;
        const int rc = esa::upload(host, &p);
        if (p) bufs_.push_back(p);
        *out = static_cast<P*>(p);
        return rc;
    }
    // The common tail of an entry: synchronise, then report the launches' first error `rc`, then the error of the copies the
    // entry made of its own buffers (`copy_what` names them), then the synchronisation's.
    int finish(int rc, hipError_t copy_error = hipSuccess, const char* copy_what = "") {
        const hipError_t se = hipStreamSynchronize(stream_);
        synced_ = true;
        if (rc) return set_error("%s: launch failed: %s", who_, hipGetErrorString((hipError_t)rc));
        if (copy_error != hipSuccess) return set_error("%s: %s: %s", who_, copy_what, hipGetErrorString(copy_error));
        if (se != hipSuccess) return set_error("%s: %s", who_, hipGetErrorString(se));
        return 0;
    }

private:
    const char* who_;
    hipStream_t stream_;
    std::vector<void*> bufs_;
    bool synced_ = false;
};

}  // namespace esa
#pragma GCC visibility pop
