// Visual-memory rows of the NavDPNet former's token buffer, gathered from a per-env ring of cached frame tokens in one launch (gfx950).
//
// A rollout keeps, per env, the final-LayerNorm tokens (fp32, WITHOUT former_pe) of its last `depth` frames in a ring: frame slot s of env e is
// ring[(e * depth + s) * ntok * C ...]. Each step tokenises only the new frame (fresh, compact over the n stepped envs); this kernel
//   * writes the new frame into ring slot head[i] of env env[i], and
//   * builds memory slots 0 .. M-1 of launch row i in the token buffer: slot j (M-1 = newest) holds the frame pushed (M-1-j) * stride pushes
//     ago, or the blank-frame tokens when env[i] has fewer pushes since its reset (count[i], the push of this step included), + pe[j * ntok + p],
//     rounded to bf16 - what the RGB tower's final LayerNorm writes when it runs over the whole window (norm.hip: t += P, then the bf16 store).
// Slot M-1 reads `fresh`, never the ring slot written in the same launch; an older slot sits (M-1-j) * stride <= depth - 1 pushes back, so it
// never aliases ring slot head[i] either: no ordering hazard inside the launch. Rows of every operand are contiguous (C floats / C bf16), so a
// workgroup (row chunk, slot, launch row) moves one contiguous run in 16-byte units. Memory-bound: 4 + 4 bytes read and 2 written per element.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunkRows = 32;   // token rows per workgroup: 32 x 384 / 8 = 1536 units, 6 per thread

__global__ __launch_bounds__(kThreads) void memory_gather_kernel(bf16* __restrict__ out, long out_env_stride, float* __restrict__ ring,
                                                                 const float* __restrict__ fresh, const float* __restrict__ blank,
                                                                 const float* __restrict__ pe, const int32_t* __restrict__ env,
                                                                 const int32_t* __restrict__ head, const int32_t* __restrict__ count, int M,
                                                                 int ntok, int C, int depth, int stride, int max_envs) {
    const int i = blockIdx.z, j = blockIdx.y;
    const int e = env[i], h = head[i], c = count[i];
    const long frame = (long)ntok * C;
    const long lo = (long)blockIdx.x * kChunkRows * C;
    const long hi = lo + (long)kChunkRows * C < frame ? lo + (long)kChunkRows * C : frame;
    bf16* dst = out + (long)i * out_env_stride + (long)j * frame;
    const float* pj = pe + (long)j * frame;
    if (e < 0 || e >= max_envs || h < 0 || h >= depth || c < 1) {   // the host validates the plan; a bad entry poisons its rows, it never
        const bf16 nan = (bf16)__builtin_nanf("");                   // reads or writes outside the ring
        const bf16x8 n8 = {nan, nan, nan, nan, nan, nan, nan, nan};
        for (long o = lo + (long)threadIdx.x * 8; o < hi; o += (long)kThreads * 8) *reinterpret_cast<bf16x8*>(dst + o) = n8;
        return;
    }
    const int back = (M - 1 - j) * stride;
    const bool newest = j == M - 1;
    const float* src;
    if (newest) src = fresh + (long)i * frame;
    else if (back < c) src = ring + ((long)e * depth + (h - back + depth) % depth) * frame;
    else src = blank;
    float* keep = newest ? ring + ((long)e * depth + h) * frame : nullptr;
    for (long o = lo + (long)threadIdx.x * 8; o < hi; o += (long)kThreads * 8) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(src + o), a1 = *reinterpret_cast<const f32x4*>(src + o + 4);
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(pj + o), p1 = *reinterpret_cast<const f32x4*>(pj + o + 4);
        if (keep) {
            *reinterpret_cast<f32x4*>(keep + o) = a0;
            *reinterpret_cast<f32x4*>(keep + o + 4) = a1;
        }
        const f32x4 s0 = a0 + p0, s1 = a1 + p1;
        const bf16x8 v = {(bf16)s0[0], (bf16)s0[1], (bf16)s0[2], (bf16)s0[3], (bf16)s1[0], (bf16)s1[1], (bf16)s1[2], (bf16)s1[3]};
        *reinterpret_cast<bf16x8*>(dst + o) = v;
    }
}

}  // namespace

int ina_launch_memory_gather(void* out, long out_env_stride, float* ring, const float* fresh, const float* blank, const float* pe,
                             const int32_t* env, const int32_t* head, const int32_t* count, int n, int max_envs, int M, int ntok, int C, int depth,
                             int stride, hipStream_t stream) {
    INA_REQUIRE(out && ring && fresh && blank && pe && env && head && count, "memory_gather: null argument");
    INA_REQUIRE(n > 0 && n <= 65535 && max_envs >= n && M > 0 && M <= 65535 && ntok > 0 && stride > 0,
                "memory_gather: bad arguments n=%d max_envs=%d M=%d ntok=%d stride=%d", n, max_envs, M, ntok, stride);
    INA_REQUIRE(C > 0 && C % 8 == 0, "memory_gather: C=%d must be a positive multiple of 8 (16-byte units)", C);
    INA_REQUIRE(depth == (M - 1) * stride + 1, "memory_gather: ring depth %d, (M - 1) * stride + 1 = %d", depth, (M - 1) * stride + 1);
    INA_REQUIRE(out_env_stride >= (long)M * ntok * C && out_env_stride % 8 == 0, "memory_gather: out_env_stride=%ld (elements) below M * ntok * C "
                "or not a multiple of 8", out_env_stride);
    auto al16 = [](const void* q) { return ((uintptr_t)q % 16) == 0; };
    INA_REQUIRE(al16(out) && al16(ring) && al16(fresh) && al16(blank) && al16(pe), "memory_gather: every tensor must be 16-byte aligned");
    const double elems = (double)n * M * ntok * C;
    InaProfScope prof(INA_PROF_ELEMENTWISE, elems, elems * 10.0 + (double)n * ntok * C * 4.0, stream);
    const dim3 grid((ntok + kChunkRows - 1) / kChunkRows, M, n);
    hipLaunchKernelGGL(memory_gather_kernel, grid, dim3(kThreads), 0, stream, reinterpret_cast<bf16*>(out), out_env_stride, ring, fresh, blank, pe,
                       env, head, count, M, ntok, C, depth, stride, max_envs);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
