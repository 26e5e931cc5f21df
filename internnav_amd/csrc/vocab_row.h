// One workgroup on one fp32 vocabulary row (gfx950), defined once for the five kernels that end a System-2 decode step: argmax_kernel
// (rope.hip), argmax_penalty_kernel (decode_penalty.hip), logprob_kernel (decode_logprob.hip), sample_kernel (decode_sample.hip) and
// beam_topm_kernel (decode_beam.hip). They promise each other bit-equal token ids and bit-equal penalised values; that holds because the
// pieces below exist once:
//   the shape       VR_THREADS threads per row; the row is read as 16-byte vectors of 4 logits when its base is 16-byte aligned, otherwise
//                   (and for the n % 4 tail) one logit at a time
//   the seen set    token t is bit t & 31 of word t >> 5 of the row's bitmap; the four logits of vector j (4j .. 4j + 3) share word j >> 3.
//                   A row's bitmap has ONE writer, its own workgroup: no global atomics
//   the penalty     penalised(): HF's RepetitionPenaltyLogitsProcessor on one value
//   the order       vr_before(): value descending, index ascending, NaN never ahead
//   the walk        vr_walk(): thread t takes vectors t, t + VR_THREADS, ... and then logits 4 * n4 + t, ... of the tail - ascending index per
//                   thread, vectors before tail: the per-thread order that the fp64-bound models of tests/decode_penalty_ref.py,
//                   tests/logprob_ref.py, tests/sample_ref.py and tests/beam_ref.py restate (change them together with this file).
//                   vr_walk_wave(): the same walk with loop bounds that are uniform over a wave, for callbacks that use wave shuffles.
//                   argmax_kernel walks with kUnroll = 1: the yardstick that tools/rep_penalty_step.py holds the penalised selection to
//   the reduction   vr_first_max(): the first maximum of the workgroup, for the two kernels that reduce nothing else
// What is NOT here is each kernel's own: its running state, its callbacks, a reduction that carries more than (value, index), the output
// writes. The pieces are plain inlined functions on the caller's registers: nothing is kept between calls.
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr int VR_THREADS = 1024;                   // threads of a row's workgroup
constexpr int VR_WAVES = VR_THREADS / INA_WAVE;    // 16: one LDS slot per wave in a block reduction
// 16-byte logit loads (and their bitmap words) in flight per thread: vr_round loads kUnroll vectors and their bitmap words before any of
// them is used. The row (152064 logits = 594 KiB) is a single latency-bound stream for one workgroup: a loop with one vector and one word per
// iteration measured 1.295 x argmax_kernel at 7 rows of 152064 logits in argmax_penalty_kernel; the figures of this form are in
// profiles/rep_penalty_b7.txt.
constexpr int VR_UNROLL = 4;

__device__ __forceinline__ float penalised(float x, float penalty) { return x < 0.f ? x * penalty : x / penalty; }   // IEEE fp32 division

// is token i in the row's seen set
__device__ __forceinline__ bool vr_seen(const uint32_t* sr, int i) { return (sr[i >> 5] >> (i & 31)) & 1u; }
// the seen bits of the logits 4j .. 4j + 3 (bit q: logit 4j + q), from w = word j >> 3 of the bitmap
__device__ __forceinline__ uint32_t vr_seen4(uint32_t w, int j) { return (w >> ((4 * j) & 31)) & 15u; }
// plain read-modify-write: the workgroup is the row's only writer (call it from ONE thread, behind every read of the bitmap)
__device__ __forceinline__ void vr_mark(uint32_t* sr, int tok) { sr[tok >> 5] |= 1u << (tok & 31); }

// the penalty on the lanes of a vector whose bit of b is set; the division runs only in waves that meet a seen token
__device__ __forceinline__ void vr_penalise4(f32x4& v, uint32_t b, float penalty) {
    if (b) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((b >> q) & 1u) v[q] = penalised(v[q], penalty);
    }
}

// the selection order: is (av, ai) ahead of (bv, bi) - value descending, index ascending; a NaN is never ahead of anything
__device__ __forceinline__ bool vr_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// The callables of the walks take the thread's running state BY VALUE and return the new one, st = f4(st, j, v, bits). With callables that
// update captured variables through references the compiler carried such a variable twice through the loop (two equal chains of selects it does
// not merge): 21.7 against 17.6 us in argmax_kernel, 2.2 % in logprob_kernel. beam_topm_kernel is the other way round (profiles/vocab_row_ab.txt).
// vectors j, j + VR_THREADS, ... (kUnroll of them, all inside the row) and their bitmap words, loaded before f4 runs on any of them
template <int kUnroll, bool kSeen, typename St, typename F4>
__device__ __forceinline__ St vr_round(const float* x, const uint32_t* sr, int j, St st, F4 f4) {
    f32x4 v[kUnroll];
    uint32_t w[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        v[u] = *reinterpret_cast<const f32x4*>(x + 4 * (j + u * VR_THREADS));
        w[u] = kSeen ? sr[(j + u * VR_THREADS) >> 3] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) st = f4(st, j + u * VR_THREADS, v[u], vr_seen4(w[u], j + u * VR_THREADS));   // ascending index per thread
    return st;
}

// One walk over the row x[0 .. n): st = f4(st, j, f32x4 of the logits 4j .. 4j + 3, their four seen bits) for this thread's vectors, then
// st = f1(st, i, logit, seen bit) for its logits of the tail (a row whose base is not 16-byte aligned is all tail). Without kSeen sr is not
// read and every bit is 0. Returns the thread's final state.
template <int kUnroll, bool kSeen, typename St, typename F4, typename F1>
__device__ __forceinline__ St vr_walk(const float* x, int n, const uint32_t* sr, St st, F4 f4, F1 f1) {
    const int n4 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? (n >> 2) : 0;
    int j = threadIdx.x;
    for (; j + (kUnroll - 1) * VR_THREADS < n4; j += kUnroll * VR_THREADS) st = vr_round<kUnroll, kSeen>(x, sr, j, st, f4);
    if constexpr (kUnroll > 1) for (; j < n4; j += VR_THREADS) st = vr_round<1, kSeen>(x, sr, j, st, f4);
    for (int i = n4 * 4 + threadIdx.x; i < n; i += VR_THREADS) st = f1(st, i, x[i], kSeen && vr_seen(sr, i));
    return st;
}

// the logits 4j .. 4j + 3 as they lie in memory and their seen bits, for any j: at or beyond n NaN (= not there), seen bit 0 and no access
template <bool kSeen>
__device__ __forceinline__ void vr_load_padded(const float* x, int n, const uint32_t* sr, int j, f32x4& v, uint32_t& b) {
    const int i0 = 4 * j;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && i0 + 3 < n) {
        v = *reinterpret_cast<const f32x4*>(x + i0);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (i0 + q < n) ? x[i0 + q] : NAN;
    }
    b = (kSeen && i0 < n) ? vr_seen4(sr[j >> 3], j) : 0u;         // 4j < n: the word exists
}

// The whole-wave form of the walk: f4 only. Thread t takes vectors t, t + VR_THREADS, ...; the 64 vectors of a CHUNK (256 token ids) lie
// in one wave, and a wave runs f4 on whole chunks - the wave's last lane decides every loop bound, lanes beyond the row see NaN - so f4 may
// use wave shuffles. Rows that are not aligned, the last rounds and the n % 4 tail come through vr_load_padded.
template <int kUnroll, bool kSeen, typename St, typename F4>
__device__ __forceinline__ St vr_walk_wave(const float* x, int n, const uint32_t* sr, St st, F4 f4) {
    const int n4 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? (n >> 2) : 0;     // whole vectors of an aligned row: 16-byte loads without a branch
    const int nq = (n + 3) >> 2;
    int j = threadIdx.x;
    for (; (j | 63) + (kUnroll - 1) * VR_THREADS < n4; j += kUnroll * VR_THREADS) st = vr_round<kUnroll, kSeen>(x, sr, j, st, f4);
    for (; (j & ~63) < nq; j += VR_THREADS) {
        f32x4 v;
        uint32_t b;
        vr_load_padded<kSeen>(x, n, sr, j, v, b);
        st = f4(st, j, v, b);
    }
    return st;
}

// The first maximum of the workgroup's (best, idx) pairs in the order of vr_before: wave butterfly, VR_WAVES slots in LDS, a scan by thread 0.
// The result is valid in thread 0 only; no entry above -inf (all -inf, all NaN) gives 0, as torch.argmax does for all -inf, so that the
// result is always an index of the row. Contains one barrier: what the workgroup read in front of the call lies in front of what thread 0
// does behind it. The wave slots are static LDS of this function: one call per kernel, or a barrier between two calls.
__device__ __forceinline__ int vr_first_max(float best, int idx) {
    __shared__ float bv[VR_WAVES];
    __shared__ int bi[VR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(idx, o);
        if (vr_before(ov, oi, best, idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < VR_WAVES; ++w)
            if (vr_before(bv[w], bi[w], best, idx)) { best = bv[w]; idx = bi[w]; }
    }
    return best > -INFINITY ? idx : 0;   // no entry above -inf: idx is the start value or whichever -inf a scalar tail met
}

}  // namespace
