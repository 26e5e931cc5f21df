// Repetition penalty of greedy System-2 decoding (gfx950): what HF generate() applies on every greedy step when the checkpoint's
// generation_config.json sets repetition_penalty (RepetitionPenaltyLogitsProcessor over prompt + answer so far).
//   token_seen_set       per sequence, the bitmap of the token ids seen so far (prompt, image placeholders included), built in LDS
//   argmax_penalty_rows  argmax_rows (rope.hip) over the penalised logits, X untouched; optionally marks the chosen token as seen,
//                        so a chain of decode steps needs no host work and no extra launch between steps
// Token t is bit t & 31 of word t >> 5. One workgroup per row in both kernels: the row's bitmap has ONE writer, no global atomics.
// The penalty, the selection order and the walk over a row are those of vocab_row.h, shared with the other token-pick kernels.
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "vocab_row.h"

namespace {

constexpr int kThreads = VR_THREADS;
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

struct Pick { float best; int idx; };   // a thread's running first maximum

// one 16-byte vector of logits (index 4j .. 4j + 3) and its four seen bits against the running best of a thread
__device__ __forceinline__ Pick select4(Pick t, f32x4 v, uint32_t b, int j, float penalty) {
    vr_penalise4(v, b, penalty);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (v[q] > t.best) { t.best = v[q]; t.idx = 4 * j + q; }   // ascending index: the first maximum is kept
    return t;
}

// The selection of argmax_kernel (rope.hip) over y: first maximum, NaN never selected, no entry above -inf gives 0 (vr_first_max); the
// row is walked as vocab_row.h lays out.
__global__ __launch_bounds__(kThreads) void argmax_penalty_kernel(const float* __restrict__ X, int ldx, int n, uint32_t* seen, int ld_words,
                                                                  float penalty, int mark, int32_t* __restrict__ out) {
    const int r = blockIdx.x;
    uint32_t* sr = seen + (size_t)r * ld_words;
    const Pick t = vr_walk<VR_UNROLL, true>(
        X + (size_t)r * ldx, n, sr, Pick{-INFINITY, 0x7fffffff},
        [=](Pick t, int j, f32x4 v, uint32_t b) { return select4(t, v, b, j, penalty); },
        [=](Pick t, int i, float v, bool s) {
            if (s) v = penalised(v, penalty);
            if (vr_before(v, i, t.best, t.idx)) { t.best = v; t.idx = i; }
            return t;
        });
    const int tok = vr_first_max(t.best, t.idx);                  // every read of the row's bitmap lies in front of its barrier
    if (threadIdx.x == 0) {
        out[r] = tok;
        if (mark) vr_mark(sr, tok);
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
