// Repetition penalty of greedy System-2 decoding (gfx950): what HF generate() applies on every greedy step when the checkpoint's
// generation_config.json sets repetition_penalty (RepetitionPenaltyLogitsProcessor over prompt + answer so far).
//   token_seen_set       per sequence, the bitmap of the token ids seen so far (prompt, image placeholders included), built in LDS
//   argmax_penalty_rows  argmax_rows (rope.hip) over the penalised logits, X untouched; optionally marks the chosen token as seen,
//                        so a chain of decode steps needs no host work and no extra launch between steps
// Token t is bit t & 31 of word t >> 5. One workgroup per row in both kernels: the row's bitmap has ONE writer, no global atomics.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kUnroll = 4;           // 16-byte logit loads in flight per thread in argmax_penalty_rows
constexpr int kSeenMaxWords = 8192;   // LDS bitmap of token_seen_set: 32 KiB = 262144 tokens (Qwen2.5-VL: 152064 tokens = 4752 words, 19 KB)

__global__ __launch_bounds__(kThreads) void token_seen_set_kernel(uint32_t* __restrict__ seen, int ld_words, const int32_t* __restrict__ ids,
                                                                  int ld_ids, const int32_t* __restrict__ lens, int n) {
    __shared__ uint32_t bits[kSeenMaxWords];
    const int r = blockIdx.x;
    const int nw = (n + 31) >> 5;                                   // <= kSeenMaxWords and <= ld_words (host check)
    for (int w = threadIdx.x; w < nw; w += kThreads) bits[w] = 0u;
    __syncthreads();
    const int32_t* row = ids + (size_t)r * ld_ids;
    int len = lens[r];
    len = len < ld_ids ? len : ld_ids;                              // never past the row
    for (int i = threadIdx.x; i < len; i += kThreads) {
        const int t = row[i];
        if ((unsigned)t < (unsigned)n) atomicOr(&bits[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    uint32_t* out = seen + (size_t)r * ld_words;
    const int full = n >> 5;                                        // words all of whose bits are tokens
    for (int w = threadIdx.x; w < full; w += kThreads) out[w] = bits[w];
    if ((n & 31) && threadIdx.x == 0) {                             // last word: the bits beyond n keep what they hold
        const uint32_t m = (1u << (n & 31)) - 1u;
        out[full] = (out[full] & ~m) | bits[full];
    }
}

__device__ __forceinline__ float penalised(float x, float penalty) { return x < 0.f ? x * penalty : x / penalty; }   // IEEE fp32 division

// one 16-byte vector of logits (index 4j .. 4j + 3) against the running best of a thread; w = the bitmap word that holds its four bits
__device__ __forceinline__ void select4(f32x4 v, uint32_t w, int j, float penalty, float& best, int& idx) {
    const uint32_t b = (w >> ((4 * j) & 31)) & 15u;
    if (b) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((b >> q) & 1u) v[q] = penalised(v[q], penalty);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (v[q] > best) { best = v[q]; idx = 4 * j + q; }   // ascending index: the first maximum is kept
}

// The selection of argmax_kernel (rope.hip) over y: first maximum, NaN never selected, no entry above -inf gives 0. The four logits of a
// 16-byte vector share one bitmap word (4j .. 4j+3 lie in word j >> 3). The division runs only in waves that meet a seen token.
__global__ __launch_bounds__(kThreads) void argmax_penalty_kernel(const float* __restrict__ X, int ldx, int n, uint32_t* seen, int ld_words,
                                                                  float penalty, int mark, int32_t* __restrict__ out) {
    __shared__ float bv[16];
    __shared__ int bi[16];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* x = X + (size_t)r * ldx;
    uint32_t* sr = seen + (size_t)r * ld_words;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    const int n4 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? (n >> 2) : 0;
    // kUnroll vectors and their bitmap words are loaded before any of them is used (a loop with one vector and one word per iteration
    // measured 1.295 x argmax_kernel at 7 rows of 152064 logits; the figures of this form are in profiles/rep_penalty_b7.txt)
    int j = threadIdx.x;
    for (; j + (kUnroll - 1) * kThreads < n4; j += kUnroll * kThreads) {
        f32x4 v[kUnroll];
        uint32_t w[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            v[u] = *reinterpret_cast<const f32x4*>(x + 4 * (j + u * kThreads));
            w[u] = sr[(j + u * kThreads) >> 3];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) select4(v[u], w[u], j + u * kThreads, penalty, best, idx);   // ascending index per thread
    }
    for (; j < n4; j += kThreads) select4(*reinterpret_cast<const f32x4*>(x + 4 * j), sr[j >> 3], j, penalty, best, idx);
    for (int j = n4 * 4 + threadIdx.x; j < n; j += kThreads) {
        float v = x[j];
        if ((sr[j >> 5] >> (j & 31)) & 1u) v = penalised(v, penalty);
        if (v > best || (v == best && j < idx)) { best = v; idx = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = idx; }
    __syncthreads();                                              // every read of the row's bitmap lies in front of this barrier
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
        const int tok = best > -INFINITY ? idx : 0;
        out[r] = tok;
        if (mark) sr[tok >> 5] |= 1u << (tok & 31);               // plain read-modify-write: this workgroup is the row's only writer
    }
}

}  // namespace

int ina_launch_token_seen_set(uint32_t* seen, int ld_words, const int32_t* ids, int ld_ids, const int32_t* lens, int rows, int n, hipStream_t stream) {
    INA_REQUIRE(seen && ids && lens, "token_seen_set: seen, ids and lens required");
    INA_REQUIRE(rows > 0 && n > 0 && ld_ids > 0, "token_seen_set: bad arguments rows=%d n=%d ld_ids=%d", rows, n, ld_ids);
    INA_REQUIRE((long)ld_words * 32 >= (long)n, "token_seen_set: ld_words=%d holds fewer than n=%d bits", ld_words, n);
    INA_REQUIRE(n <= kSeenMaxWords * 32, "token_seen_set: a vocabulary of %d tokens exceeds the %d-token LDS bitmap", n, kSeenMaxWords * 32);
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, (double)rows * (4.0 * ld_ids + n / 8.0), stream);
    hipLaunchKernelGGL(token_seen_set_kernel, dim3(rows), dim3(kThreads), 0, stream, seen, ld_words, ids, ld_ids, lens, n);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}

int ina_launch_argmax_penalty(const float* X, int ldx, int rows, int n, uint32_t* seen, int ld_words, float penalty, int mark, int32_t* out,
                              hipStream_t stream) {
    INA_REQUIRE(X && seen && out, "argmax_penalty_rows: X, seen and out required");
    INA_REQUIRE(rows > 0 && n > 0 && (ldx >= n || rows == 1), "argmax_penalty_rows: bad arguments rows=%d n=%d ldx=%d", rows, n, ldx);
    INA_REQUIRE((long)ld_words * 32 >= (long)n, "argmax_penalty_rows: ld_words=%d holds fewer than n=%d bits", ld_words, n);
    INA_REQUIRE(isfinite(penalty) && penalty > 0.f, "argmax_penalty_rows: repetition penalty %g is not a strictly positive finite float", (double)penalty);
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, (double)rows * (4.0 * n + n / 8.0), stream);
    hipLaunchKernelGGL(argmax_penalty_kernel, dim3(rows), dim3(kThreads), 0, stream, X, ldx, n, seen, ld_words, penalty, mark, out);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
