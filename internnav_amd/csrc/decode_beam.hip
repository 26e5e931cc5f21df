// Beam search of System-2 decoding (gfx950): the three launches that take the place of the selection launch when generate(num_beams=K) decodes
// the K hypotheses of every prompt behind the prompt's one cache slot - transformers' GenerationMixin._beam_search without a host round trip
// between the steps and without a [rows, vocab] tensor leaving the device.
//   beam_topm_rows   per output row r (logits row s = src ? src[r] : r): y = log_softmax(x[s]) in fp32, the repetition penalty ON y as HF's beam
//                    search applies it (seen ? (y < 0 ? y * p : y / p) : y), acc = y + run_score[r]; the M <= 32 best entries by (acc descending,
//                    token id ascending) go to cand_score / cand_tok [r, M]. The global top M of a prompt takes at most M from any row.
//                    Conventions: a NaN logit counts as -inf (never ahead of a number); a row without a number has every y = -inf; an acc that
//                    is NaN (a NaN / +inf run_score) counts as -inf; -inf entries fill up in id order; a src outside [0, x_rows) is never
//                    accessed and gives scores -inf, ids 0 .. M-1. X and seen are only read.
//   beam_step        the bookkeeping, one workgroup per prompt: merges the K sorted lists into the prompt's M candidates (step 0: row 0 only),
//                    then the running set, the finished set, the early-stop heuristic flag and `done` in HF's fp32 sentinel arithmetic
//                    (tests/beam_ref.py restates the rules; the file's docstring lists them). A done prompt is frozen: nothing of it is written.
//   beam_reorder     in front of the next pass: for every layer the first t tail rows of row r of the destination tail set come from row
//                    parent[r] of the source set (16-byte vector copy, kv_copy.hip's form), seen'[r] = seen[parent[r]] | bit(next_tok[r]),
//                    state'[r] = state[parent[r]]. A parent outside [0, rows) copies nothing for its row.
// No atomics anywhere: two launches on the same inputs give the same bits. No workspace.
//
// beam_topm_rows, one workgroup of 1024 threads per row, three walks over the row (the second and third come out of the L2; order, penalty
// and selection order are those of vocab_row.h):
//   1. the maximum (exact)       2. s = sum expf(x - max)      3. every thread keeps the two best acc of its own entries
// then M rounds: the best head of the 1024 threads (wave butterfly, 16 wave slots in LDS, one barrier per round) is the next candidate; its
// owner moves its second entry up, and once both are gone walks its own ~150 entries again for the next two behind the candidate just
// emitted (rare: a thread that owns three of a row's best M; rows of ties or of -inf, whose best ids lie side by side, take it every round).
// Summation shape (mirrored by the bound model of tests/beam_ref.py; change both together):
//   BEAM_THREADS = 1024 (VR_THREADS); a thread adds the terms of its entries in the order of vr_walk (vocab_row.h): 16-byte vectors of an
//   aligned row, then one logit per step. A wave's 64 sums: 6-level butterfly; the 16 wave sums: added in order. expf / logf of the device
//   library (not the fast intrinsics). y = (x - max) - logf(s), the penalty one multiplication or IEEE division, acc = y + run_score: one
//   rounding each, contraction off - an entry's acc has the same bits whichever walk computes it.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "vocab_row.h"

namespace {

constexpr int kThreads = VR_THREADS;
constexpr int kWaves = VR_WAVES;
constexpr int kMaxM = 32;
constexpr int kMaxK = 8;
constexpr int kNone = 0x7fffffff;    // id of an empty slot: behind every real entry of the same value
constexpr float kSent = -1.0e9f;     // HF's sentinel

__device__ __forceinline__ float clean(float v) { return v != v ? -INFINITY : v; }

// One walk over the row (vocab_row.h): f(index, logit, seen bit) for this thread's entries, in ascending index. f keeps its results in captured
// variables, the walk carries no state: with scan_top2's candidates carried by value the kernel measured 59.4 against 56.5 us (M = 4)
struct NoState {};
template <bool kSeen, typename F>
__device__ __forceinline__ void for_entries(const float* __restrict__ x, int n, const uint32_t* __restrict__ sr, F f) {
    vr_walk<VR_UNROLL, kSeen>(
        x, n, sr, NoState{},
        [&](NoState st, int j, f32x4 v, uint32_t b) {
#pragma unroll
            for (int q = 0; q < 4; ++q) f(4 * j + q, v[q], (b >> q) & 1u);
            return st;
        },
        [&](NoState st, int i, float v, bool seen_i) { f(i, v, seen_i); return st; });
}

// acc of one entry (x already clean): the same bits in every walk
__device__ __forceinline__ float acc_of(float x, bool seen, float mx, float ls, float penalty, float run) {
#pragma clang fp contract(off)
    float y = mx > -INFINITY ? (x - mx) - ls : -INFINITY;
    if (seen) y = penalised(y, penalty);
    const float a = y + run;
    return a != a ? -INFINITY : a;
}

struct Ent {
    float v;
    int i;
};

// the two best of this thread's entries behind (bv, bi) in the order (bounded), or of all of them
template <bool kSeen>
__device__ __forceinline__ int scan_top2(const float* __restrict__ x, int n, const uint32_t* __restrict__ sr, float mx, float ls, float penalty, float run,
                                         bool bounded, float bv, int bi, Ent& e1, Ent& e2) {
    e1 = {-INFINITY, kNone};
    e2 = {-INFINITY, kNone};
    int own = 0;
    for_entries<kSeen>(x, n, sr, [&](int i, float v, bool s) {
        const float a = acc_of(clean(v), s, mx, ls, penalty, run);
        ++own;
        if (bounded && !vr_before(bv, bi, a, i)) return;
        if (vr_before(a, i, e1.v, e1.i)) { e2 = e1; e1 = {a, i}; }
        else if (vr_before(a, i, e2.v, e2.i)) e2 = {a, i};
    });
    return own;
}

template <bool kSeen>
__global__ __launch_bounds__(kThreads) void beam_topm_kernel(const float* __restrict__ X, int ldx, int x_rows, int n, const uint32_t* __restrict__ seen,
                                                             int ld_words, float penalty, const float* __restrict__ run_score,
                                                             const int32_t* __restrict__ src, int M, float* __restrict__ cand_score,
                                                             int32_t* __restrict__ cand_tok) {
    __shared__ float wv[2][kWaves];
    __shared__ int wi[2][kWaves];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = src ? src[r] : r;
    if ((unsigned)s >= (unsigned)x_rows) {                        // (uniform over the workgroup: no barrier is skipped by a part of it)
        if ((int)threadIdx.x < M) { cand_score[(size_t)r * M + threadIdx.x] = -INFINITY; cand_tok[(size_t)r * M + threadIdx.x] = threadIdx.x; }
        return;
    }
    const float* x = X + (size_t)s * ldx;
    const uint32_t* sr = kSeen ? seen + (size_t)r * ld_words : nullptr;
    const float run = run_score[r];

    // ---- 1: the row's maximum
    float mx = -INFINITY;
    for_entries<false>(x, n, nullptr, [&](int, float v, bool) { mx = fmaxf(mx, clean(v)); });
    mx = wave_max(mx);
    if (lane == 0) wv[0][wave] = mx;
    __syncthreads();
    for (int w = 0; w < kWaves; ++w) mx = fmaxf(mx, wv[0][w]);
    // ---- 2: s = sum exp(x - max); a row without a number keeps ls = 0 and gets y = -inf from acc_of
    float ls = 0.f;
    if (mx > -INFINITY) {                                         // (uniform)
        float sum = 0.f;
        for_entries<false>(x, n, nullptr, [&](int, float v, bool) { sum += expf(clean(v) - mx); });
        sum = wave_sum(sum);
        if (lane == 0) wv[1][wave] = sum;
        __syncthreads();
        sum = 0.f;
        for (int w = 0; w < kWaves; ++w) sum += wv[1][w];        // every thread adds the 16 wave sums in the same order
        ls = logf(sum);
    }
    __syncthreads();                                              // (the wave slots are used again below)
    // ---- 3: the two best acc of every thread's own entries
    Ent e1, e2;
    const int own = scan_top2<kSeen>(x, n, sr, mx, ls, penalty, run, false, 0.f, 0, e1, e2);
    int popped = 0;
    // ---- M rounds: the best head is the next candidate
    for (int k = 0; k < M; ++k) {
        float v = e1.v;
        int i = e1.i;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o);
            const int oi = __shfl_xor(i, o);
            if (vr_before(ov, oi, v, i)) { v = ov; i = oi; }
        }
        if (lane == 0) { wv[k & 1][wave] = v; wi[k & 1][wave] = i; }
        __syncthreads();                                          // (slot set k & 1 is written again two barriers from here)
        v = wv[k & 1][0];
        i = wi[k & 1][0];
        for (int w = 1; w < kWaves; ++w)
            if (vr_before(wv[k & 1][w], wi[k & 1][w], v, i)) { v = wv[k & 1][w]; i = wi[k & 1][w]; }
        if (threadIdx.x == 0) { cand_score[(size_t)r * M + k] = v; cand_tok[(size_t)r * M + k] = i == kNone ? 0 : i; }
        if (i != kNone && e1.i == i) {                            // the owner: ids are unique
            ++popped;
            e1 = e2;
            e2 = {-INFINITY, kNone};
            if (e1.i == kNone && popped < own && k + 1 < M) scan_top2<kSeen>(x, n, sr, mx, ls, penalty, run, true, v, i, e1, e2);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------- beam_step
struct StepArgs {
    const float* cand_score;
    const int32_t* cand_tok;
    int K, M, T, step, max_new, early, n_eos;
    float lenpow, hyppow;
    const int32_t* eos;
    float* run_score;
    int32_t *next_tok, *parent;
    const int32_t* hist_in;
    int32_t* hist_out;
    const float* ts_in;
    float* ts_out;
    int32_t* fin_tok;
    float *fin_ts, *fin_score;
    int32_t *fin_len, *fin_flag, *heur, *done;
};

constexpr int kStepThreads = 64;

__global__ __launch_bounds__(kStepThreads) void beam_step_kernel(StepArgs a) {
#pragma clang fp contract(off)
    __shared__ float c_s[kMaxM], rs[kMaxM], ms[kMaxK + kMaxM], old_run[kMaxK], n_score[kMaxK], o_score[kMaxK], m_score[kMaxK];
    __shared__ int c_beam[kMaxM], c_tok[kMaxM], c_hit[kMaxM], ptr[kMaxK], sel[kMaxK], msel[kMaxK], o_len[kMaxK], o_flag[kMaxK];
    const int b = blockIdx.x, K = a.K, M = a.M, T = a.T, j = a.step, L = a.step + 1, tid = threadIdx.x;
    const int r0 = b * K;
    if (j > 0 && a.done[b]) return;                               // frozen (uniform over the workgroup)
    if (tid == 0) {
        const bool last = L == a.max_new;
        const bool flag = j == 0 ? true : a.heur[b] != 0;
        for (int k = 0; k < K; ++k) {
            old_run[k] = j == 0 ? (k == 0 ? 0.f : kSent) : a.run_score[r0 + k];
            o_score[k] = j == 0 ? kSent : a.fin_score[r0 + k];
            o_len[k] = j == 0 ? 0 : a.fin_len[r0 + k];
            o_flag[k] = j == 0 ? 0 : a.fin_flag[r0 + k];
            ptr[k] = 0;
        }
        // the prompt's M candidates: a K-way merge of the rows' sorted lists; equal scores: the lower beam first (beam * V + token ascending)
        const int rows = j == 0 ? 1 : K;
        for (int i = 0; i < M; ++i) {
            int best = -1;
            float bv = 0.f;
            for (int k = 0; k < rows; ++k) {
                if (ptr[k] >= M) continue;
                const float v = a.cand_score[(size_t)(r0 + k) * M + ptr[k]];
                if (best < 0 || v > bv) { best = k; bv = v; }
            }
            c_s[i] = bv;
            c_beam[i] = best;
            c_tok[i] = a.cand_tok[(size_t)(r0 + best) * M + ptr[best]];
            ++ptr[best];
        }
        bool full = true, all_hit = true;
        for (int k = 0; k < K; ++k) full = full && o_flag[k] != 0;
        const bool full_early = full && a.early == 1;
        for (int i = 0; i < M; ++i) {
            bool hit = last;
            for (int e = 0; e < a.n_eos; ++e) hit = hit || c_tok[i] == a.eos[e];
            c_hit[i] = hit;
            all_hit = all_hit && hit;
            rs[i] = c_s[i] + (hit ? kSent : -0.f);
            float v = c_s[i] / a.lenpow;
            v = v + (full_early ? kSent : 0.f);
            v = v + (!flag ? kSent : 0.f);
            v = v + (!(hit && i < K) ? kSent : 0.f);
            ms[K + i] = v;
        }
        for (int k = 0; k < K; ++k) ms[k] = o_score[k];
        // next running set: the K best by rs, ties by position
        uint32_t taken = 0;
        for (int k = 0; k < K; ++k) {
            int best = -1;
            for (int i = 0; i < M; ++i)
                if (!((taken >> i) & 1u) && (best < 0 || rs[i] > rs[best])) best = i;
            taken |= 1u << best;
            sel[k] = best;
            n_score[k] = rs[best];
        }
        // finished set: old entries first, then the candidates; the K best stay, ties by position
        unsigned long long mt = 0;
        bool now_full = true;
        float worst = INFINITY;
        for (int k = 0; k < K; ++k) {
            int best = -1;
            for (int i = 0; i < K + M; ++i)
                if (!((mt >> i) & 1ull) && (best < 0 || ms[i] > ms[best])) best = i;
            mt |= 1ull << best;
            msel[k] = best;
            m_score[k] = ms[best];
            worst = fminf(worst, ms[best]);
            now_full = now_full && (best < K ? o_flag[best] != 0 : (c_hit[best - K] && best - K < K));
        }
        // heuristic flag and done
        const float bestrun = n_score[0] / a.hyppow;
        bool better = false;
        for (int k = 0; k < K; ++k) {
            const int i = msel[k];
            const bool fin = i < K ? o_flag[i] != 0 : (c_hit[i - K] && i - K < K);
            better = better || bestrun > (fin ? worst : kSent);
        }
        const bool nflag = flag && better;
        a.heur[b] = nflag;
        a.done[b] = !nflag || (a.early == 1 && now_full) || all_hit;
    }
    __syncthreads();
    // running rows: histories gathered by parent (the other buffer of the pair), the new token appended
    for (int e = tid; e < K * L; e += kStepThreads) {
        const int k = e / L, t = e % L, i = sel[k], p = r0 + c_beam[i];
        const size_t o = (size_t)(r0 + k) * T + t;
        if (t < j) {
            a.hist_out[o] = a.hist_in[(size_t)p * T + t];
            a.ts_out[o] = a.ts_in[(size_t)p * T + t];
        } else {
            a.hist_out[o] = c_tok[i];
            a.ts_out[o] = c_s[i] == -INFINITY ? -INFINITY : c_s[i] - old_run[c_beam[i]];
        }
    }
    if (tid < K) {
        const int i = sel[tid];
        a.next_tok[r0 + tid] = c_tok[i];
        a.parent[r0 + tid] = r0 + c_beam[i];
        a.run_score[r0 + tid] = n_score[tid];
    }
    // finished rows in place, from the last to the first: an old entry only ever moves down (the old set is sorted and stays in order)
    for (int d = K - 1; d >= 0; --d) {
        const int i = msel[d];
        int32_t* ft = a.fin_tok + (size_t)(r0 + d) * T;
        float* fs = a.fin_ts + (size_t)(r0 + d) * T;
        if (i < K) {
            if (i != d)
                for (int t = tid; t < T; t += kStepThreads) {
                    ft[t] = a.fin_tok[(size_t)(r0 + i) * T + t];
                    fs[t] = a.fin_ts[(size_t)(r0 + i) * T + t];
                }
        } else {
            const int c = i - K, p = r0 + c_beam[c];
            for (int t = tid; t < L; t += kStepThreads) {
                ft[t] = t < j ? a.hist_in[(size_t)p * T + t] : c_tok[c];
                fs[t] = t < j ? a.ts_in[(size_t)p * T + t] : (c_s[c] == -INFINITY ? -INFINITY : c_s[c] - old_run[c_beam[c]]);
            }
        }
        if (tid == 0) {
            a.fin_score[r0 + d] = m_score[d];
            a.fin_len[r0 + d] = i < K ? o_len[i] : L;
            a.fin_flag[r0 + d] = i < K ? o_flag[i] : (c_hit[i - K] && i - K < K);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------- beam_reorder
constexpr int kCopyThreads = 256;

__global__ __launch_bounds__(kCopyThreads) void beam_reorder_kernel(const int64_t* __restrict__ src_base, const int64_t* __restrict__ dst_base, int n_layers,
                                                                    const int32_t* __restrict__ parent, int rows, long T, long t, long row_bytes,
                                                                    const uint32_t* __restrict__ seen_src, uint32_t* __restrict__ seen_dst, int ld_words,
                                                                    const int32_t* __restrict__ next_tok, int n, const int32_t* __restrict__ state_src,
                                                                    int32_t* __restrict__ state_dst) {
    const int r = blockIdx.x, l = blockIdx.y;
    const int p = parent[r];
    if ((unsigned)p >= (unsigned)rows) return;                    // copies nothing, accesses nothing
    if (l < n_layers) {
        const int4* s = reinterpret_cast<const int4*>(src_base[l] + (long)p * T * row_bytes);
        int4* d = reinterpret_cast<int4*>(dst_base[l] + (long)r * T * row_bytes);
        const long units = t * row_bytes / 16;
        for (long i = threadIdx.x; i < units; i += kCopyThreads) d[i] = s[i];
        return;
    }
    if (seen_src) {
        const int tok = next_tok[r];
        const bool mark = (unsigned)tok < (unsigned)n;
        for (int w = threadIdx.x; w < ld_words; w += kCopyThreads) {
            uint32_t v = seen_src[(size_t)p * ld_words + w];
            if (mark && w == (tok >> 5)) v |= 1u << (tok & 31);
            seen_dst[(size_t)r * ld_words + w] = v;
        }
    }
    if (state_src && threadIdx.x == 0) state_dst[r] = state_src[p];
}

}  // namespace

int ina_launch_beam_topm(const float* X, int ldx, int x_rows, int rows, int n, const uint32_t* seen, int ld_words, float penalty, const float* run_score,
                         const int32_t* src, int M, float* cand_score, int32_t* cand_tok, hipStream_t stream) {
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, (double)rows * (3.0 * 4.0 * n + (seen ? n / 8.0 : 0.0)), stream);
    if (seen)
        hipLaunchKernelGGL(beam_topm_kernel<true>, dim3(rows), dim3(kThreads), 0, stream, X, ldx, x_rows, n, seen, ld_words, penalty, run_score, src, M,
                           cand_score, cand_tok);
    else
        hipLaunchKernelGGL(beam_topm_kernel<false>, dim3(rows), dim3(kThreads), 0, stream, X, ldx, x_rows, n, seen, ld_words, 1.f, run_score, src, M,
                           cand_score, cand_tok);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}

int ina_launch_beam_step(const float* cand_score, const int32_t* cand_tok, int B, int K, int M, int T, int step, int max_new, float lenpow, float hyppow,
                         int early, const int32_t* eos, int n_eos, float* run_score, int32_t* next_tok, int32_t* parent, const int32_t* hist_in,
                         int32_t* hist_out, const float* ts_in, float* ts_out, int32_t* fin_tok, float* fin_ts, float* fin_score, int32_t* fin_len,
                         int32_t* fin_flag, int32_t* heur, int32_t* done, hipStream_t stream) {
    StepArgs a = {cand_score, cand_tok, K, M, T, step, max_new, early, n_eos, lenpow, hyppow, eos, run_score, next_tok, parent, hist_in, hist_out,
                  ts_in, ts_out, fin_tok, fin_ts, fin_score, fin_len, fin_flag, heur, done};
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, (double)B * K * (8.0 * M + 16.0 * T), stream);
    hipLaunchKernelGGL(beam_step_kernel, dim3(B), dim3(kStepThreads), 0, stream, a);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}

int ina_launch_beam_reorder(const int64_t* src_base, const int64_t* dst_base, int n_layers, const int32_t* parent, int rows, int T, int t, long row_bytes,
                            const uint32_t* seen_src, uint32_t* seen_dst, int ld_words, const int32_t* next_tok, int n, const int32_t* state_src,
                            int32_t* state_dst, hipStream_t stream) {
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, 2.0 * rows * ((double)n_layers * t * row_bytes + (seen_src ? 4.0 * ld_words : 0.0)), stream);
    hipLaunchKernelGGL(beam_reorder_kernel, dim3(rows, n_layers + 1), dim3(kCopyThreads), 0, stream, src_base, dst_base, n_layers, parent, rows, (long)T,
                       (long)t, row_bytes, seen_src, seen_dst, ld_words, next_tok, n, state_src, state_dst);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
