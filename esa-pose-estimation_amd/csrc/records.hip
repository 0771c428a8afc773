// records.hip — the packed records of the device path, after the all-gather of a sharded batch (parallel.gather_records).
//
// A packed record is field-major: field 0 of every crop, then field 1 of every crop, ... (inference.record_fields: b_f bytes
// per crop and field, every b_f a positive multiple of 4), so field f of a record laid out for m crops starts at
//     off_f(m) = m * (b_0 + ... + b_{f-1}).
// A rank's record is therefore no slice of the batch's record.  all_gather_into_tensor leaves `world` blocks behind, each
// laid out for n_max = ceil(n_total / world) crops; rank r's block holds its shard in the first hi_r - lo_r crop slots of
// every field.  The shard rule is parallel.shard_bounds: a contiguous split, the first n_total % world ranks get one crop
// more,
//     base = n_total / world, extra = n_total % world, lo_r = r * base + min(r, extra), hi_r = lo_r + base + (r < extra).
// The kernel recomputes it from world and n_total (no table is uploaded) and writes the record of the whole batch:
//     out[off_f(n_total) + i * b_f ... + b_f] = block_r[off_f(n_max) + (i - lo_r) * b_f ... + b_f],   lo_r <= i < hi_r.
//
// gather_records_kernel: blockIdx.y = field, a grid-stride loop over the field's n_total * b_f / 4 dwords; one dword load
// and one dword store per element, both per-lane (vector) accesses in plain C++.  Every dword of `out` is written exactly
// once.  Only slots j < hi_r - lo_r of a block are read: its padding slots, and the whole block of a rank without crops, may
// be uninitialised memory.  The field sizes travel by value in the kernel arguments.
#include <cstdint>

#include "../../include/esahrnet.h"
#include "kernels.h"

namespace esa {
namespace {

constexpr int kMaxFields = 16;

struct RecordFields {
    int dwords[kMaxFields];          // b_f / 4
};

__global__ __launch_bounds__(256) void gather_records_kernel(const uint32_t* gathered, int world, int n_total, int n_max,
                                                             RecordFields fields, int nfields, uint32_t* out) {
    const int f = blockIdx.y;
    unsigned long long before = 0, all = 0;                 // dwords per crop of the fields in front of f, and of all fields
    int bw = 0;
#pragma unroll
    for (int g = 0; g < kMaxFields; ++g) {
        const int d = g < nfields ? fields.dwords[g] : 0;
        before += g < f ? (unsigned long long)d : 0ull;
        all += (unsigned long long)d;
        bw = g == f ? d : bw;
    }
    const unsigned long long ubw = (unsigned long long)bw;
    const unsigned long long block = all * (unsigned long long)n_max;            // dwords of one rank's block
    const unsigned long long src_field = before * (unsigned long long)n_max;
    const unsigned long long dst_field = before * (unsigned long long)n_total;
    const unsigned long long count = ubw * (unsigned long long)n_total;
    const int base = n_total / world, extra = n_total % world;
    const int split = extra * (base + 1);                   // crops of the ranks that hold base + 1
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < count;
         t += (unsigned long long)gridDim.x * blockDim.x) {
        const int i = (int)(t / ubw);                       // global crop
        const unsigned long long e = t - (unsigned long long)i * ubw;
        int r, lo;
        if (i < split) {
            r = i / (base + 1);
            lo = r * (base + 1);
        } else {                                            // base >= 1 here: split <= i < n_total = world * base + extra
            r = extra + (i - split) / base;
            lo = r * base + extra;
        }
        const unsigned long long j = (unsigned long long)(i - lo);   // < hi_r - lo_r: never a padding slot
        out[dst_field + t] = gathered[(unsigned long long)r * block + src_field + j * ubw + e];
    }
}

}  // namespace
}  // namespace esa

extern "C" int esahrnet_gather_records(const void* gathered_dev, int world, int n_total, const int* field_bytes, int nfields,
                                       void* out_dev, esahrnet_stream stream) {
    using esa::set_error;
    if (!gathered_dev || !out_dev || !field_bytes) return set_error("gather_records: null argument");
    if (world < 1) return set_error("gather_records: world = %d (at least 1)", world);
    if (n_total < 1) return set_error("gather_records: n_total = %d (at least 1 crop)", n_total);
    if (nfields < 1 || nfields > esa::kMaxFields)
        return set_error("gather_records: %d fields (1..%d)", nfields, esa::kMaxFields);
    if ((reinterpret_cast<uintptr_t>(gathered_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 7)
        return set_error("gather_records: gathered_dev and out_dev must be 8-byte aligned");
    esa::RecordFields fields = {};
    long long per_crop = 0, widest = 0;
    for (int f = 0; f < nfields; ++f) {
        if (field_bytes[f] < 4 || field_bytes[f] % 4)
            return set_error("gather_records: field %d has %d bytes per crop (a positive multiple of 4)", f, field_bytes[f]);
        fields.dwords[f] = field_bytes[f] / 4;
        per_crop += field_bytes[f];
        widest = field_bytes[f] > widest ? field_bytes[f] : widest;
    }
    const int n_max = (int)(((long long)n_total + world - 1) / world);
    if (per_crop * n_max > 0x7fffffffLL)
        return set_error("gather_records: a block of %d crops x %lld bytes exceeds 2^31 - 1 bytes", n_max, per_crop);
    const long long dwords = widest / 4 * n_total;          // of the largest field
    long long gx = (dwords + 255) / 256;
    gx = gx > 1024 ? 1024 : gx;
    hipLaunchKernelGGL(esa::gather_records_kernel, dim3((unsigned)gx, (unsigned)nfields), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint32_t*>(gathered_dev), world, n_total, n_max, fields,
                       nfields, static_cast<uint32_t*>(out_dev));
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return set_error("gather_records: kernel launch failed: %s", hipGetErrorString(rc));
    return 0;
}
