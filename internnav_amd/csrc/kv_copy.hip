// Row ranges of the System-2 KV cache between the engine's cache slots and caller-owned tensors, all layers and sequences in one launch
// (gfx950).
//
// The engine keeps K/V of layer l in one tensor per layer, bf16 [B_max * S_max, kv_w]: the rows of cache slot b start at b * S_max.
// A caller keeps a sequence's rows layer-major, [layers, n, kv_w] (rows contiguous, any layer stride). Per (layer, sequence) the copy is
// one contiguous run of n_rows * row_bytes bytes on both sides, so the kernel is a plain 16-byte vector memcpy: workgroup (x, s, l)
// grid-strides over the 16-byte units of pair (l, s). Bit copy, no arithmetic. Device tables only: graph capturable.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;           // 16-byte units in flight per thread and iteration
constexpr int kMaxBlocksX = 2048;    // grid cap over all (layer, sequence) pairs; the rest is grid-strided

__global__ __launch_bounds__(kThreads) void kv_copy_kernel(const int64_t* __restrict__ layer_base, const int64_t* __restrict__ seq,
                                                           long engine_rows, long row_bytes, int to_engine) {
    const int s = blockIdx.y, l = blockIdx.z;
    const int64_t* e = seq + 4 * s;
    const long row0 = e[2], n_rows = e[3];
    if (row0 < 0 || n_rows <= 0 || row0 + n_rows > engine_rows) return;   // the host validates; a bad entry copies nothing
    int4* eng = reinterpret_cast<int4*>(layer_base[l] + row0 * row_bytes);
    int4* usr = reinterpret_cast<int4*>(e[0] + (long)l * e[1]);
    const int4* src = to_engine ? usr : eng;
    int4* dst = to_engine ? eng : usr;
    const long n = n_rows * row_bytes / 16;
    const long step = (long)gridDim.x * kThreads;
    long i = (long)blockIdx.x * kThreads + threadIdx.x;
    for (; i + (kUnroll - 1) * step < n; i += kUnroll * step) {
        int4 v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = src[i + u * step];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) dst[i + u * step] = v[u];
    }
    for (; i < n; i += step) dst[i] = src[i];
}

}  // namespace

int ina_launch_kv_copy(int to_engine, const int64_t* layer_base, int n_layers, const int64_t* seq, int n_seq, long engine_rows, long row_bytes,
                       long max_rows, hipStream_t stream) {
    INA_REQUIRE(layer_base && seq && n_layers > 0 && n_layers <= 65535 && n_seq > 0 && n_seq <= 65535 && engine_rows > 0 && max_rows > 0,
                "kv_copy: bad arguments layers=%d seqs=%d engine_rows=%ld max_rows=%ld", n_layers, n_seq, engine_rows, max_rows);
    INA_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0, "kv_copy: row_bytes=%ld must be a positive multiple of 16", row_bytes);
    INA_REQUIRE(to_engine == 0 || to_engine == 1, "kv_copy: direction %d (0 export, 1 import)", to_engine);
    const long units = max_rows * row_bytes / 16;
    const long pairs = (long)n_layers * n_seq;
    long bx = (units + (long)kThreads * kUnroll - 1) / ((long)kThreads * kUnroll);
    bx = std::max(1L, std::min(bx, std::max(1L, kMaxBlocksX / pairs)));
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, 2.0 * (double)pairs * max_rows * row_bytes, stream);
    hipLaunchKernelGGL(kv_copy_kernel, dim3((unsigned)bx, n_seq, n_layers), dim3(kThreads), 0, stream, layer_base, seq, engine_rows, row_bytes,
                       to_engine);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
