// Sampling step of System-2 decoding (gfx950): temperature, top-k, top-p and the draw in ONE launch that takes the place of the argmax /
// logprob launch - HF generate(do_sample=True) with its processors in HF's order (repetition penalty, temperature, top-k, top-p), without a
// [rows, vocab] tensor leaving the device and without a random number generated here: the uniforms come from the host.
//   sample_rows   per output row r (logits row s = src ? src[r] : r; seen set, u and the outputs are indexed by r):
//     1. y = x[s], or the repetition-penalised row (penalised() of vocab_row.h over the bits of seen[r]); z = y / T, one IEEE fp32
//        division (bit-equal to torch's scores / temperature). -0 counts as +0. NaN entries are never kept.
//     2. top-k (top_k > 0): with k = min(top_k, entries that are not NaN) and v_k the k-th largest z, keep z >= v_k; ties at v_k all stay.
//     3. top-p (top_p < 1) over what top-k kept, with masses p_i = exp(z_i - max z) / sum: a VALUE v is kept iff the mass of the kept
//        entries with z > v is < top_p * (the whole kept mass) - i.e. iff the mass at or below v is > 1 - top_p. Equal values stay or go
//        together; the maximum always stays. top_p == 1 switches the step off (zero-mass entries stay in the kept set).
//        thr[r] = the smallest kept value, n_kept[r] = the number of entries with z >= thr[r].
//     4. draw: q_i = p_i / (kept mass); tok[r] = the first kept index j in ascending token id whose inclusive cumulative q exceeds u[r].
//     5. logprob[r] = log q_tok = (z_tok - max z) - log(kept mass): the log-softmax of HF's processed scores at the draw.
//   Conventions: -inf entries have mass 0 (and are never drawn); a row with nothing above -inf, or a src outside [0, x_rows) (never
//   accessed), gives tok 0, logprob NaN, n_kept 0, thr NaN; with a +inf maximum the +inf entries share the mass. u outside [0, 1) is clamped.
//   X is only read. mark != 0 sets the drawn token's bit in seen[r]. One workgroup per row: the row's bitmap has ONE writer.
//
// Determinism: every sum that feeds a result is an INTEGER sum. An entry's mass is w = expf(z - max z) (the device library's expf, not the
// fast intrinsic) scaled to fixed point, m = trunc(w * 2^44) as uint64: at most 2^18 entries of at most 2^44 stay below 2^62. Histogram
// adds (64-bit LDS atomics) and scans of integers do not depend on the order of arrival, so two launches give the same bits.
//
// Shape (mirrored by the bound model of tests/sample_ref.py; change both together):
//   SAMPLE_THREADS = 1024 (VR_THREADS), SAMPLE_MASS_BITS = 44; a row is walked in quads of 4 logits by vr_walk_wave (vocab_row.h)
//   Every pass walks the penalised logits y; z = y / T is monotone in y, so selections run on the keys of y, a threshold found there is taken
//   to z by one division and back to the lowest y that reaches it by a 32-step bisection - the same kept set as a selection on z, and only
//   the entries whose mass is needed pay for the division and the expf.
//   pass 0     max, min and count of the entries that are not NaN
//   top-k      radix select on the monotone uint32 image of y, digits of 11 | 11 | 10 bits from the top: a pass histograms COUNTS of the entries
//              that match the prefix found so far; a block-wide suffix scan finds the digit that holds the k-th largest
//   top-p      the same select over MASSES of the entries top-k kept: the digit in which the mass above crosses ceil(top_p * kept mass)
//   draw       pass A sums the kept mass of every chunk of 256 consecutive token ids (the 64 quads of one wave) and the kept count; a
//              block-wide prefix scan over the (at most 1024) chunks finds the one that holds floor(u * mass) + 1; one wave walks that
//              chunk again with a 64-lane integer scan
//   behind a top-k   the last level of its select also lists the entries in or above the bin it found (at most 1024, with the token id);
//              when that list holds everything top-k kept, top-p and the draw run on it - thread t on candidate t, masses above a key and up
//              to a token id as integer sums over the list - and the row is not walked again. A list that overflows, or a tie in z that
//              reaches below its lowest key, takes the passes above
//   A step that is switched off costs no pass: (top_k 0, top_p 1) is pass 0 + draw; (top_k 50, any top_p) is pass 0 + 3.
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "vocab_row.h"

namespace {

constexpr int kThreads = VR_THREADS;
constexpr int kWaves = VR_WAVES;
constexpr int kBins = 2048;                        // 11-bit digits: two bins per thread in the scan
constexpr float kMassScale = 17592186044416.f;    // 2^44
constexpr int kCand = 1024;                        // entries of the candidate list behind a top-k: one per thread

typedef unsigned long long u64;

// monotone image of a float that is not NaN: a < b  <=>  key(a) < key(b) (callers turn -0 into +0 first)
__device__ __forceinline__ uint32_t key_of(float z) {
    const uint32_t b = __float_as_uint(z);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

struct Row {
    const float* x;
    const uint32_t* sr;
    int n;
    float penalty, T;
};

// y of a loaded vector: the penalised logits (-0 -> +0: one key per value). The selections run on y - z = y / T is monotone in y, so the k-th
// largest z is (the k-th largest y) / T and a threshold in z is a threshold in y (`lowest_key_reaching`) - and only the entries whose mass is
// needed pay for the division and the expf.
__device__ __forceinline__ void finish(f32x4 v, uint32_t b, float penalty, float (&z)[4]) {
    vr_penalise4(v, b, penalty);
#pragma unroll
    for (int q = 0; q < 4; ++q) z[q] = v[q] == 0.f ? 0.f : v[q];
}

// z of a penalised logit: one IEEE fp32 division (-0 -> +0)
__device__ __forceinline__ float z_of(float y, float T) {
    const float z = y / T;
    return z == 0.f ? 0.f : z;
}

// the smallest key K in [lo, hi] with z_of(value_of(K)) >= v, given that hi has it: the y-image of "z >= v" (z is monotone in y; every key
// between two keys of numbers is the key of a number)
__device__ __forceinline__ uint32_t lowest_key_reaching(float v, uint32_t lo, uint32_t hi, float T) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (z_of(value_of(mid), T) >= v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// One pass over the row: st = f(st, j, y) for every quad j, in the whole-wave form of the walk (vocab_row.h): a wave runs f on whole chunks
// of 64 quads (256 token ids; lanes beyond the row see NaN), so f may use wave shuffles. The thread's running state goes through f by value.
template <bool kSeen, typename St, typename F>
__device__ __forceinline__ St for_quads(const Row& R, St st, F f) {
    const float penalty = R.penalty;
    return vr_walk_wave<VR_UNROLL, kSeen>(R.x, R.n, R.sr, st, [=](St st, int j, f32x4 v, uint32_t b) {
        float z[4];
        finish(v, b, penalty, z);
        return f(st, j, z);
    });
}

struct NoState {};      // the state of a pass that keeps nothing per thread
struct Span { float mx, mn; uint32_t cnt; };   // pass 0

__device__ __forceinline__ u64 mass_of(float y, float T, float M) {
    const float z = z_of(y, T);
    const float w = z == M ? 1.f : expf(z - M);                   // (a +inf maximum: inf - inf never appears)
    return (u64)(w * kMassScale);                                 // exact scaling by a power of two, then truncation
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum of v over the threads with a HIGHER (kAbove) or a LOWER thread id (wt: kWaves words of LDS); contains two barriers
template <bool kAbove>
__device__ __forceinline__ u64 block_sum_beyond(u64 v, u64* wt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = kAbove ? __shfl_down(inc, o) : __shfl_up(inc, o);
        if (kAbove ? lane + o < 64 : lane >= o) inc += y;
    }
    __syncthreads();                                              // (wt may still be read from the previous call)
    if (lane == (kAbove ? 0 : 63)) wt[wave] = inc;
    __syncthreads();
    u64 s = inc - v;
    for (int w = 0; w < kWaves; ++w)
        if (kAbove ? w > wave : w < wave) s += wt[w];
    return s;
}

struct Shared {
    u64 hist[kBins];     // a select's histogram; in the draw, the kept mass of chunk c at [c] (at most 1024 chunks)
    u64 wt[kWaves];
    uint32_t wcount[kWaves];
    float wmax[kWaves], wmin[kWaves];
    u64 sel_above, total;
    uint32_t sel_bin;
    // candidate list behind a top-k (filled by the last level of its select): token id, y and mass of the entries at or above the
    // select's last bin, in the order of arrival - everything computed from it is an integer sum or a minimum, so the order does not show
    int32_t cand_idx[kCand];
    float cand_y[kCand];
    u64 cand_m[kCand];
    uint32_t n_cand, n_kept, min_key;
};

// Radix select over the keys of y >= floor_key (and not NaN): the key K with above(K) < target <= above(K) + h(K), where h(K) is the count
// (kMass false) or the mass (kMass true) of the entries with key K and above(K) that of the entries with a larger key. The caller
// guarantees 1 <= target <= the total of the counts; for masses the target is ceil(top_p * the total), known once level 0 has its histogram:
// the mass above a kept value is < top_p * total  <=>  < ceil(top_p * total). Every thread returns K.
// kCollect (count select): the last level also appends every entry whose key lies in or above the bin found so far to the candidate list
// (S.n_cand counts them all, the list holds the first kCand).
template <bool kSeen, bool kMass, bool kCollect>
__device__ uint32_t radix_select(const Row& R, float M, uint32_t floor_key, u64 target, float top_p, Shared& S) {
    uint32_t prefix = 0;          // the digits found so far, in place
    u64 above = 0;                // h of everything above the prefix's range
    int hi = 32;                  // bits [hi, 32) of the key are fixed
#pragma unroll 1
    for (int level = 0; level < 3; ++level) {
        const int bits = level < 2 ? 11 : 10, shift = hi - bits;
        S.hist[2 * threadIdx.x] = 0;
        S.hist[2 * threadIdx.x + 1] = 0;
        if (threadIdx.x == 0) { S.sel_bin = 0; S.sel_above = above; }
        __syncthreads();
        for_quads<kSeen>(R, NoState{}, [&](NoState st, int j, const float (&z)[4]) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (z[q] != z[q]) continue;
                const uint32_t k = key_of(z[q]);
                if (kCollect && level == 2 && (k >> 10) >= (prefix >> 10)) {
                    const uint32_t slot = atomicAdd(&S.n_cand, 1u);
                    if (slot < (uint32_t)kCand) { S.cand_idx[slot] = 4 * j + q; S.cand_y[slot] = z[q]; }
                }
                if (k < floor_key || (hi < 32 && (k >> hi) != (prefix >> hi))) continue;
                const u64 h = kMass ? mass_of(z[q], R.T, M) : 1ull;
                if (h) atomicAdd(&S.hist[(k >> shift) & ((1u << bits) - 1u)], h);
            }
            return st;
        });
        __syncthreads();
        const u64 h0 = S.hist[2 * threadIdx.x], h1 = S.hist[2 * threadIdx.x + 1];
        const u64 a1 = above + block_sum_beyond<true>(h0 + h1, S.wt), a0 = a1 + h1;       // above bin 2t + 1, above bin 2t
        if (kMass && level == 0) {
            if (threadIdx.x == 0) S.total = a0 + h0;
            __syncthreads();
            const u64 Wk = S.total;                               // >= 2^44: the maximum's own mass
            const u64 lim = (u64)ceil((double)top_p * (double)Wk);
            target = lim > Wk ? Wk : (lim < 1 ? 1 : lim);
        }
        if (a1 < target && target <= a1 + h1) { S.sel_bin = 2 * threadIdx.x + 1; S.sel_above = a1; }
        else if (a0 < target && target <= a0 + h0) { S.sel_bin = 2 * threadIdx.x; S.sel_above = a0; }
        __syncthreads();
        prefix |= S.sel_bin << shift;
        above = S.sel_above;
        hi = shift;
        __syncthreads();                                          // (sel_* are reset by the next level)
    }
    return prefix;
}

template <bool kSeen>
__global__ __launch_bounds__(kThreads) void sample_kernel(const float* __restrict__ X, int ldx, int x_rows, int n, uint32_t* seen, int ld_words,
                                                          float penalty, int mark, float T, int top_k, float top_p, const float* __restrict__ U,
                                                          const int32_t* __restrict__ src, int32_t* __restrict__ tok, float* __restrict__ logprob,
                                                          int32_t* __restrict__ n_kept, float* __restrict__ thr) {
    __shared__ Shared S;
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = src ? src[r] : r;
    if (threadIdx.x == 0) {                                       // what a row without a draw returns; a draw overwrites it behind a barrier
        tok[r] = 0;
        logprob[r] = NAN;
        if (n_kept) n_kept[r] = 0;
        if (thr) thr[r] = NAN;
    }
    if ((unsigned)s >= (unsigned)x_rows) return;                  // (uniform over the workgroup: no barrier is skipped by a part of it)
    uint32_t* sr = kSeen ? seen + (size_t)r * ld_words : nullptr;
    Row R;
    R.x = X + (size_t)s * ldx;
    R.sr = sr;
    R.n = n;
    R.penalty = penalty;
    R.T = T;

    // ---- pass 0: maximum, minimum, number of entries that are not NaN
    const Span sp = for_quads<kSeen>(R, Span{-INFINITY, INFINITY, 0u}, [](Span t, int, const float (&z)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (z[q] == z[q]) { t.mx = fmaxf(t.mx, z[q]); t.mn = fminf(t.mn, z[q]); ++t.cnt; }
        return t;
    });
    float mx = sp.mx, mn = sp.mn;
    uint32_t cnt = sp.cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o));
        mn = fminf(mn, __shfl_xor(mn, o));
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) { S.wmax[wave] = mx; S.wmin[wave] = mn; S.wcount[wave] = cnt; }
    __syncthreads();
    cnt = 0;
    for (int w = 0; w < kWaves; ++w) { mx = fmaxf(mx, S.wmax[w]); mn = fminf(mn, S.wmin[w]); cnt += S.wcount[w]; }
    const float M = z_of(mx, T);                                  // max z = (max y) / T
    if (!(M > -INFINITY)) return;                                 // nothing above -inf (uniform)
    __syncthreads();                                              // (the wave slots are used again below)

    // ---- top-k, then top-p over what it kept: selections on the keys of y, thresholds taken to z and back
    const uint32_t key_min = key_of(mn);
    uint32_t floor_key = key_min;                                 // an entry is kept iff its key is >= floor_key
    float thr_z = z_of(mn, T);
    if (top_k > 0 && (uint32_t)top_k < cnt) {
        if (threadIdx.x == 0) S.n_cand = 0;                       // (the select starts with a barrier)
        const uint32_t kk = radix_select<kSeen, false, true>(R, M, 0u, (u64)top_k, 1.f, S);
        thr_z = z_of(value_of(kk), T);                            // v_k
        floor_key = lowest_key_reaching(thr_z, key_min, kk, T);   // ties at v_k in z all stay
        // ---- the short way: everything top-k kept is in the candidate list (it fits, and no tie in z reaches below the list's lowest
        //      key) - top-p and the draw run on the list, thread t on candidate t, without another pass over the row
        const uint32_t N = S.n_cand;
        if (N <= (uint32_t)kCand && floor_key >= (kk & ~1023u)) {
            const int t = threadIdx.x;
            const bool have = (uint32_t)t < N;
            const float yt = have ? S.cand_y[t] : 0.f;
            const int it = have ? S.cand_idx[t] : 0;
            const uint32_t kt = key_of(yt);
            u64 mt = (have && kt >= floor_key) ? mass_of(yt, T, M) : 0;
            S.cand_m[t] = mt;
            if (t == 0) { S.min_key = key_of(mx); S.n_kept = 0; } // (the maximum always stays: the mass above it is 0)
            __syncthreads();
            if (top_p < 1.f) {
                u64 Wk = 0, above = 0;
                for (uint32_t c = 0; c < N; ++c) {
                    const u64 mc = S.cand_m[c];
                    Wk += mc;
                    if (key_of(S.cand_y[c]) > kt) above += mc;
                }
                const u64 lim = (u64)ceil((double)top_p * (double)Wk);
                const u64 limit = lim > Wk ? Wk : (lim < 1 ? 1 : lim);
                if (have && kt >= floor_key && above < limit) atomicMin(&S.min_key, kt);
                __syncthreads();
                const uint32_t kp = S.min_key;
                thr_z = z_of(value_of(kp), T);
                floor_key = lowest_key_reaching(thr_z, floor_key, kp, T);
                if (kt < floor_key) mt = 0;
                S.cand_m[t] = mt;                                 // (every read of the old masses lies in front of the barrier above)
            }
            const bool kept = have && kt >= floor_key;
            if (kept) atomicAdd(&S.n_kept, 1u);
            __syncthreads();
            u64 W = 0, cum = 0;                                   // cum: the kept mass at token ids <= this candidate's
            for (uint32_t c = 0; c < N; ++c) {
                const u64 mc = S.cand_m[c];
                W += mc;
                if (S.cand_idx[c] <= it) cum += mc;
            }
            float u = U[r];
            u = u >= 0.f ? u : 0.f;                                // (NaN -> 0)
            const double tw = floor((double)u * (double)W);
            u64 target = tw >= (double)W ? W : (u64)tw + 1;
            target = target > W ? W : target;
            if (t == 0) {
                if (n_kept) n_kept[r] = (int32_t)S.n_kept;
                if (thr) thr[r] = thr_z;
            }
            if (kept && mt > 0 && cum - mt < target && target <= cum) {      // one candidate holds the target
                tok[r] = it;
                const float Wf = (float)((double)W * (1.0 / 17592186044416.0));
                const float zt = z_of(yt, T);
                logprob[r] = (zt == M ? 0.f : zt - M) - logf(Wf);
                if (kSeen && mark) vr_mark(sr, it);                // behind every read of the bitmap
            }
            return;
        }
    }
    if (top_p < 1.f) {
        const uint32_t kp = radix_select<kSeen, true, false>(R, M, floor_key, 0, top_p, S);
        thr_z = z_of(value_of(kp), T);
        floor_key = lowest_key_reaching(thr_z, floor_key, kp, T); // the entries that share the value in z stay together
    }

    // ---- draw, pass A: the kept mass of every chunk of 256 token ids (a wave's 64 quads), and the kept count
    S.hist[threadIdx.x] = 0;                                      // (chunks beyond the row)
    if (threadIdx.x == 0) { S.sel_bin = 0; S.sel_above = 0; }
    __syncthreads();
    cnt = for_quads<kSeen>(R, 0u, [&](uint32_t c, int j, const float (&z)[4]) {
        u64 m = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (z[q] == z[q] && key_of(z[q]) >= floor_key) { m += mass_of(z[q], T, M); ++c; }
        m = wave_sum_u64(m);
        if (lane == 0) S.hist[j >> 6] = m;
        return c;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) S.wcount[wave] = cnt;
    __syncthreads();                                              // every read of the row's bitmap by the passes lies in front of this barrier
    const u64 cm = S.hist[threadIdx.x];                           // thread c: chunk c
    const u64 below = block_sum_beyond<false>(cm, S.wt);
    if (threadIdx.x == kThreads - 1) S.total = below + cm;
    __syncthreads();
    const u64 W = S.total;                                        // >= 2^44: the maximum is kept
    // the first id whose inclusive cumulative mass exceeds u * W = the first with cumulative mass >= floor(u * W) + 1
    float u = U[r];
    u = u >= 0.f ? u : 0.f;                                        // (NaN -> 0)
    const double tw = floor((double)u * (double)W);
    u64 target = tw >= (double)W ? W : (u64)tw + 1;
    target = target > W ? W : target;
    if (below < target && target <= below + cm) { S.sel_bin = threadIdx.x; S.sel_above = below; }      // one chunk holds the target
    __syncthreads();
    if (wave != 0) return;                                        // (no barrier follows)
    if (lane == 0) {
        cnt = 0;
        for (int w = 0; w < kWaves; ++w) cnt += S.wcount[w];
        if (n_kept) n_kept[r] = (int32_t)cnt;
        if (thr) thr[r] = thr_z;
    }

    // ---- draw, pass B: one wave walks the chunk that holds the target with a 64-lane integer scan
    const int j = (int)S.sel_bin * 64 + lane;
    const u64 run = S.sel_above;
    f32x4 vq;
    uint32_t bq;
    vr_load_padded<kSeen>(R.x, n, sr, j, vq, bq);
    float z[4];
    finish(vq, bq, penalty, z);
    u64 mq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) mq[q] = (z[q] == z[q] && key_of(z[q]) >= floor_key) ? mass_of(z[q], T, M) : 0;
    const u64 own = mq[0] + mq[1] + mq[2] + mq[3];
    u64 inc = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    const u64 hit = __ballot(run + inc >= target);                // not empty: the chunk's mass reaches the target
    if (hit && lane == __ffsll((long long)hit) - 1) {
        u64 c = run + inc - own + mq[0];                          // (no indexing by a run-time q: the quad stays in registers)
        int q = 0;
        float yq = z[0];
        if (c < target) {
            c += mq[1]; q = 1; yq = z[1];
            if (c < target) {
                c += mq[2]; q = 2; yq = z[2];
                if (c < target) { q = 3; yq = z[3]; }
            }
        }
        const int t = 4 * j + q;                                  // its mass is > 0: a kept entry, t < n
        tok[r] = t;
        const float Wf = (float)((double)W * (1.0 / 17592186044416.0));
        const float zt = z_of(yq, T);
        logprob[r] = (zt == M ? 0.f : zt - M) - logf(Wf);
        if (kSeen && mark) vr_mark(sr, t);
    }
}

}  // namespace

int ina_launch_sample(const float* X, int ldx, int x_rows, int rows, int n, uint32_t* seen, int ld_words, float penalty, int mark, float temperature,
                      int top_k, float top_p, const float* u, const int32_t* src, int32_t* tok, float* logprob, int32_t* n_kept, float* thr,
                      hipStream_t stream) {
    const int passes = 2 + (top_k > 0 ? 3 : 0) + (top_p < 1.f ? 3 : 0);
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, (double)rows * passes * (4.0 * n + (seen ? n / 8.0 : 0.0)), stream);
    if (seen)
        hipLaunchKernelGGL(sample_kernel<true>, dim3(rows), dim3(kThreads), 0, stream, X, ldx, x_rows, n, seen, ld_words, penalty, mark, temperature,
                           top_k, top_p, u, src, tok, logprob, n_kept, thr);
    else
        hipLaunchKernelGGL(sample_kernel<false>, dim3(rows), dim3(kThreads), 0, stream, X, ldx, x_rows, n, seen, ld_words, 1.f, 0, temperature, top_k,
                           top_p, u, src, tok, logprob, n_kept, thr);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
