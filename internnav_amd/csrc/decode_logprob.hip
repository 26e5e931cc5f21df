// Per-token log-probability of System-2 decoding (gfx950): log-softmax of a vocabulary row at ONE index, fused with the selection the greedy
// chain already runs (argmax_rows, rope.hip / argmax_penalty_rows, decode_penalty.hip) - what HF returns through
// generate(output_scores=True) + compute_transition_scores(normalize_logits=True), without a [B, vocab] tensor leaving the device.
//   logprob_rows   per row r, with y = x or the repetition-penalised row (penalised() of vocab_row.h over the bits of `seen`):
//                  tok     = target[r], or (target == NULL) the selection of argmax_rows over y - the same total order (value descending,
//                            index ascending, NaN never greater), so the ids are bit-equal to those kernels whatever the reduction shape
//                  logprob = y[tok] - max(y) - log sum exp(y - max(y))        (fp32; torch.log_softmax(y, -1)[tok])
//                  margin  = y[tok] - max of y over the OTHER indices          (the "top-2 margin"; >= 0 when tok was selected)
// X is only read. One workgroup per row, walked as vocab_row.h lays out: the row's bitmap has ONE writer (mark), no global atomics.
//
// Math: expf / logf of the device library (NOT the __expf / __logf fast intrinsics); the bound model of tests/logprob_ref.py assumes 2 ulp.
// One pass, online: a thread keeps (best, idx, second, sum) with sum = sum exp(y - best) over what it has seen; when a 16-byte vector raises
// best the sum is rescaled ONCE by expf(old - new) before the vector's four terms are added.
//
// Summation shape (mirrored by tests/logprob_ref.py; change both together):
//   LOGPROB_THREADS = 1024         threads of a row's workgroup (VR_THREADS)
//   LOGPROB_VEC = 4                logits per 16-byte vector; a thread's terms are added sequentially in the order of vr_walk (vocab_row.h):
//                                  at most one rescale per vector (acc4), per logit on the one-by-one path (acc1)
//   LOGPROB_WAVE = 64              a wave's 64 sums are scaled once to the wave's maximum, then added in a 6-level butterfly
//   LOGPROB_WAVES = 16             the 16 wave sums are scaled once to the row's maximum and added sequentially by thread 0
// Conventions: a NaN anywhere in the row -> NaN logprob; -inf entries contribute 0; an all -inf row -> tok 0 (selection), NaN logprob.
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "vocab_row.h"

namespace {

constexpr int kThreads = VR_THREADS;
constexpr int kWaves = VR_WAVES;

struct Run {
    float best;      // largest y so far (never NaN)
    int idx;         // its first index
    float second;    // largest y at any other index
    float sum;       // sum exp(y - best) over every y so far: NaN once a NaN was met, 0 while best is -inf
};

// exp(m - M) for two maxima m <= M; equal maxima (both -inf included) scale by exactly 1, a sum that belongs to m = -inf is 0 or NaN and stays so
__device__ __forceinline__ float scale_to(float m, float M) { return m == M ? 1.f : expf(m - M); }

__device__ __forceinline__ void take(float v, int j, Run& t) {
    if (v > t.best) { t.second = t.best; t.best = v; t.idx = j; }
    else if (v > t.second) t.second = v;
}

// the sum moves from maximum m to the raised t.best; m = -inf: expf(-inf) = 0 and the sum (0 or NaN) keeps its value
__device__ __forceinline__ void rescale(float m, Run& t) {
    if (t.best > m) t.sum *= expf(m - t.best);
}

// one term: a -inf logit adds exp(-inf) = 0, a NaN logit NaN. While best is still -inf (only -inf / NaN so far) the reference point is 0, so that
// -inf - (-inf) never appears
__device__ __forceinline__ float ref_point(float best) { return best > -INFINITY ? best : 0.f; }

// one 16-byte vector of logits (index 4j .. 4j + 3) and its four seen bits: at most one rescale
__device__ __forceinline__ void acc4(f32x4 v, uint32_t b, int j, float penalty, Run& t) {
    vr_penalise4(v, b, penalty);
    const float m = t.best;
#pragma unroll
    for (int q = 0; q < 4; ++q) take(v[q], 4 * j + q, t);    // ascending index: the first maximum is kept
    rescale(m, t);
    const float c = ref_point(t.best);
#pragma unroll
    for (int q = 0; q < 4; ++q) t.sum += expf(v[q] - c);
}

// the n % 4 tail and rows that are not 16-byte aligned: one logit per step, at most one rescale per logit
__device__ __forceinline__ void acc1(float v, int i, Run& t) {
    const float m = t.best;
    take(v, i, t);                                                // ascending per thread as well: strict > keeps the first maximum
    rescale(m, t);
    t.sum += expf(v - ref_point(t.best));
}

template <bool kSeen>
__global__ __launch_bounds__(kThreads) void logprob_kernel(const float* __restrict__ X, int ldx, int n, uint32_t* seen, int ld_words, float penalty,
                                                           int mark, const int32_t* __restrict__ target, int32_t* __restrict__ tok,
                                                           float* __restrict__ logprob, float* __restrict__ margin) {
    __shared__ float bv[kWaves], b2[kWaves], bs[kWaves];
    __shared__ int bi[kWaves];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int tgt = 0;
    if (target) {
        tgt = target[r];
        if ((unsigned)tgt >= (unsigned)n) {                       // ignored label (HF's -100): the row is not even read
            if (threadIdx.x == 0) {
                tok[r] = tgt;
                logprob[r] = 0.f;
                if (margin) margin[r] = 0.f;
            }
            return;                                               // (uniform over the workgroup: no barrier is skipped by a part of it)
        }
    }
    const float* x = X + (size_t)r * ldx;
    uint32_t* sr = kSeen ? seen + (size_t)r * ld_words : nullptr;
    Run t = vr_walk<VR_UNROLL, kSeen>(
        x, n, sr, Run{-INFINITY, 0x7fffffff, -INFINITY, 0.f},
        [=](Run t, int j, f32x4 v, uint32_t b) { acc4(v, b, j, penalty, t); return t; },
        [=](Run t, int i, float v, bool seen_i) { acc1(seen_i ? penalised(v, penalty) : v, i, t); return t; });
    // wave: the selection first (every lane ends with the wave's best / idx / second), then each lane's sum scaled once to the wave's best
    const float own = t.best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(t.best, o), o2 = __shfl_xor(t.second, o);
        const int oi = __shfl_xor(t.idx, o);
        if (vr_before(ov, oi, t.best, t.idx)) { t.second = fmaxf(t.best, o2); t.best = ov; t.idx = oi; }
        else t.second = fmaxf(t.second, ov);                      // (the loser's second is never above its best)
    }
    t.sum = wave_sum(t.sum * scale_to(own, t.best));
    if (lane == 0) { bv[wave] = t.best; bi[wave] = t.idx; b2[wave] = t.second; bs[wave] = t.sum; }
    __syncthreads();                                              // every read of the row's bitmap by the loops lies in front of this barrier
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) {
            if (vr_before(bv[w], bi[w], t.best, t.idx)) { t.second = fmaxf(t.best, b2[w]); t.best = bv[w]; t.idx = bi[w]; }
            else t.second = fmaxf(t.second, bv[w]);
        }
        float s = 0.f;
        for (int w = 0; w < kWaves; ++w) s += bs[w] * scale_to(bv[w], t.best);
        const int k = target ? tgt : (t.best > -INFINITY ? t.idx : 0);
        float yk = x[k];
        if (kSeen && vr_seen(sr, k)) yk = penalised(yk, penalty);
        tok[r] = k;
        logprob[r] = (yk - t.best) - logf(s);                     // all -inf: -inf - (-inf) = NaN; s >= 1 otherwise (the maximum's own term)
        if (margin) margin[r] = yk - (k == t.idx ? t.second : t.best);
        if (kSeen && mark) vr_mark(sr, k);
    }
}

}  // namespace

int ina_launch_logprob(const float* X, int ldx, int rows, int n, uint32_t* seen, int ld_words, float penalty, int mark, const int32_t* target,
                       int32_t* tok, float* logprob, float* margin, hipStream_t stream) {
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, (double)rows * (4.0 * n + (seen ? n / 8.0 : 0.0)), stream);
    if (seen)
        hipLaunchKernelGGL(logprob_kernel<true>, dim3(rows), dim3(kThreads), 0, stream, X, ldx, n, seen, ld_words, penalty, mark, target, tok, logprob, margin);
    else
        hipLaunchKernelGGL(logprob_kernel<false>, dim3(rows), dim3(kThreads), 0, stream, X, ldx, n, seen, ld_words, 1.f, 0, target, tok, logprob, margin);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
