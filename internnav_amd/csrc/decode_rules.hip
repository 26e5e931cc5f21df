// transformers' logits-processor family for System-2 decoding (gfx950): sequence_bias, no_repeat_ngram_size, bad_words_ids, min_length /
// min_new_tokens, forced_eos_token_id, suppress_tokens, begin_suppress_tokens as DATA on the device, applied by ONE launch in front of the
// unchanged selection kernels (argmax_rows, argmax_penalty_rows, logprob_rows, sample_rows: all of them treat -inf as "mass 0, never chosen").
//   logit_rules_rows  one workgroup per row: append the token the previous step chose to the row's history, add the finite biases, store -inf
//                     over what the history and the step ban, and at the forced column fill the row
// The vocabulary is never walked but by the forced-EOS fill: the work is history length + rule count. Tables (internnav_amd/logit_rules.py):
//   grp_tok i32 [G], grp_base f32 [G], grp_ptr i32 [G + 1]   target groups: DISTINCT target tokens within [0, n_bias) and within [n_bias, G);
//                                                            groups [0, n_bias) add (grp_base + the biases of their matched sequences, in
//                                                            table order, fp32), groups [n_bias, G) ban on any match
//   seq_ptr i32 [Ns + 1], seq_ids i32, seq_bias f32 [Ns]     per multi-token sequence its tokens BUT THE LAST; a sequence of L tokens matches
//                                                            iff the history has at least L tokens and ends in its first L - 1
//   ban_tok / begin_tok / eos_tok / forced_tok i32           always banned / at col 0 / while col < eos_first[r] / 0.0 at col == forced_col
// Phases, a workgroup barrier between them: (1) append, (2) finite biases - one thread per group, one read-modify-write per target, (3) the
// history bans (n-gram scan strided over history positions, bad-word groups, EOS): stores of -inf, which commute, (4) at the forced column
// the dense fill and 0.0 at the forced ids, (5) ban_tok and begin_tok - behind (4), as transformers runs suppress_tokens behind
// forced_eos_token_id. No atomics; every thread uses prev_tok as loaded for the position thread 0 stores it to. History ids and prev_tok
// outside [0, n) only ever take part in integer comparisons; no index is used before it is range-checked.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxNgram = 16;
constexpr int kMaxSeqs = 1024;
constexpr int kMaxSeqLen = 32;

struct Hist {                       // the row's history as every thread sees it: position `last` is prev_tok (stored by thread 0, never re-read)
    const int32_t* h;
    int last, prev;
    __device__ __forceinline__ int operator()(int i) const { return i == last ? prev : h[i]; }
};

// does the history of H tokens end in the L - 1 tokens of sequence s (and hold at least L)?
__device__ __forceinline__ bool seq_match(const Hist& hv, int H, const int32_t* __restrict__ seq_ptr, const int32_t* __restrict__ seq_ids, int s, int n_ids) {
    const int p0 = seq_ptr[s], P = seq_ptr[s + 1] - p0;
    if (p0 < 0 || P < 1 || P >= kMaxSeqLen || p0 + P > n_ids || P + 1 > H) return false;
    for (int i = 0; i < P; ++i)
        if (hv(H - P + i) != seq_ids[p0 + i]) return false;
    return true;
}

__global__ __launch_bounds__(kThreads) void logit_rules_kernel(float* __restrict__ X, int ldx, int n, int col, int32_t* __restrict__ hist, int ld_hist,
                                                               int hist_cap, const int32_t* __restrict__ len0, const int32_t* __restrict__ prev_tok, int ngram,
                                                               const int32_t* __restrict__ grp_tok, const float* __restrict__ grp_base,
                                                               const int32_t* __restrict__ grp_ptr, int n_bias, int n_groups,
                                                               const int32_t* __restrict__ seq_ptr, const int32_t* __restrict__ seq_ids,
                                                               const float* __restrict__ seq_bias, int n_seqs, int n_ids,
                                                               const int32_t* __restrict__ ban_tok, int n_ban, const int32_t* __restrict__ begin_tok, int n_begin,
                                                               const int32_t* __restrict__ eos_tok, int n_eos, const int32_t* __restrict__ eos_first,
                                                               const int32_t* __restrict__ forced_tok, int n_forced, int forced_col) {
    __shared__ int32_t tail[kMaxNgram];
    const int r = blockIdx.x, tid = threadIdx.x;
    float* x = X + (size_t)r * ldx;
    int32_t* h = hist + (size_t)r * ld_hist;
    // ---- (1) append. A row whose prompt length is outside [0, hist_cap - col] has no history: nothing is stored, no history rule fires
    const int l0 = len0[r];
    const bool live = l0 >= 0 && l0 <= hist_cap - col;
    const int H = live ? l0 + col : 0;
    Hist hv{h, -1, 0};
    if (live && col > 0) {                                       // H - 1 = l0 + col - 1 is inside [0, hist_cap)
        hv.last = H - 1;
        hv.prev = prev_tok[r];
        if (tid == 0) h[H - 1] = hv.prev;
    }
    const int P = ngram - 1;                                     // the n-gram rule's prefix = the history's last P tokens
    const bool scan = ngram >= 1 && H >= ngram;
    if (scan && tid < P) tail[tid] = hv(H - P + tid);
    // ---- (2) finite biases: one thread per target, fp32 in table order, ONE read-modify-write
    for (int g = tid; g < n_bias; g += kThreads) {
        const int t = grp_tok[g];
        if ((unsigned)t >= (unsigned)n) continue;
        float b = grp_base[g];
        const int s1 = grp_ptr[g + 1];
        for (int s = grp_ptr[g]; s < s1; ++s)
            if ((unsigned)s < (unsigned)n_seqs && seq_match(hv, H, seq_ptr, seq_ids, s, n_ids)) b += seq_bias[s];
        x[t] += b;
    }
    __syncthreads();
    // ---- (3) bans that depend on the history or the step: stores of -inf only
    if (scan) {
        for (int i = tid; i + P < H; i += kThreads) {            // window [i, i + P] lies inside the history
            bool m = true;
            for (int k = 0; k < P && m; ++k) m = hv(i + k) == tail[k];
            if (m) {
                const int t = hv(i + P);
                if ((unsigned)t < (unsigned)n) x[t] = -INFINITY;
            }
        }
    }
    for (int g = n_bias + tid; g < n_groups; g += kThreads) {
        const int t = grp_tok[g];
        if ((unsigned)t >= (unsigned)n) continue;
        const int s1 = grp_ptr[g + 1];
        bool m = false;
        for (int s = grp_ptr[g]; s < s1 && !m; ++s) m = (unsigned)s < (unsigned)n_seqs && seq_match(hv, H, seq_ptr, seq_ids, s, n_ids);
        if (m) x[t] = -INFINITY;
    }
    if (n_eos > 0 && col < eos_first[r]) {
        for (int e = tid; e < n_eos; e += kThreads) {
            const int t = eos_tok[e];
            if ((unsigned)t < (unsigned)n) x[t] = -INFINITY;
        }
    }
    // ---- (4) forced EOS (col is the same in every thread: the barriers are uniform)
    if (n_forced > 0 && col == forced_col) {
        __syncthreads();
        const int a0 = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2);      // single entries up to the first 16-byte boundary
        const int v0 = a0 < n ? a0 : n, v1 = v0 + ((n - v0) & ~3);
        for (int j = tid; j < v0; j += kThreads) x[j] = -INFINITY;
        for (int j = v0 + 4 * tid; j < v1; j += 4 * kThreads) *reinterpret_cast<f32x4*>(x + j) = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int j = v1 + tid; j < n; j += kThreads) x[j] = -INFINITY;
        __syncthreads();
        for (int f = tid; f < n_forced; f += kThreads) {
            const int t = forced_tok[f];
            if ((unsigned)t < (unsigned)n) x[t] = 0.0f;
        }
        __syncthreads();
    }
    // ---- (5) the static lists
    for (int i = tid; i < n_ban; i += kThreads) {
        const int t = ban_tok[i];
        if ((unsigned)t < (unsigned)n) x[t] = -INFINITY;
    }
    if (col == 0) {
        for (int i = tid; i < n_begin; i += kThreads) {
            const int t = begin_tok[i];
            if ((unsigned)t < (unsigned)n) x[t] = -INFINITY;
        }
    }
}

}  // namespace

int ina_launch_logit_rules(float* X, int ldx, int rows, int n, int col, int32_t* hist, int ld_hist, int hist_cap, const int32_t* len0,
                           const int32_t* prev_tok, int ngram, const int32_t* grp_tok, const float* grp_base, const int32_t* grp_ptr, int n_bias, int n_groups,
                           const int32_t* seq_ptr, const int32_t* seq_ids, const float* seq_bias, int n_seqs, int n_ids, const int32_t* ban_tok, int n_ban,
                           const int32_t* begin_tok, int n_begin, const int32_t* eos_tok, int n_eos, const int32_t* eos_first, const int32_t* forced_tok,
                           int n_forced, int forced_col, hipStream_t stream) {
    INA_REQUIRE(X && hist && len0, "logit_rules_rows: X, hist and len0 required");
    INA_REQUIRE(rows >= 0 && rows <= 65535 && n >= 1 && ldx >= n, "logit_rules_rows: bad arguments rows=%d n=%d ldx=%d (0 <= rows <= 65535, n >= 1, ldx >= n)",
                rows, n, ldx);
    INA_REQUIRE(hist_cap >= 1 && ld_hist >= hist_cap && col >= 0 && col <= hist_cap,
                "logit_rules_rows: col=%d hist_cap=%d ld_hist=%d (hist_cap >= 1, ld_hist >= hist_cap, 0 <= col <= hist_cap)", col, hist_cap, ld_hist);
    INA_REQUIRE(col == 0 || prev_tok, "logit_rules_rows: prev_tok required behind column 0");
    INA_REQUIRE(ngram >= 0 && ngram <= kMaxNgram, "logit_rules_rows: n-gram size %d (0 = off .. %d)", ngram, kMaxNgram);
    INA_REQUIRE(n_bias >= 0 && n_groups >= n_bias && n_seqs >= 0 && n_seqs <= kMaxSeqs && n_ids >= 0,
                "logit_rules_rows: %d bias groups of %d groups, %d sequences (<= %d), %d sequence ids", n_bias, n_groups, n_seqs, kMaxSeqs, n_ids);
    INA_REQUIRE(n_groups == 0 || (grp_tok && grp_ptr && (n_bias == 0 || grp_base)), "logit_rules_rows: grp_tok, grp_ptr (and grp_base) required with groups");
    INA_REQUIRE(n_seqs == 0 || (seq_ptr && seq_bias && (n_ids == 0 || seq_ids)), "logit_rules_rows: seq_ptr, seq_ids and seq_bias required with sequences");
    INA_REQUIRE(n_ban >= 0 && n_begin >= 0 && n_eos >= 0 && n_forced >= 0, "logit_rules_rows: negative list length");
    INA_REQUIRE((n_ban == 0 || ban_tok) && (n_begin == 0 || begin_tok) && (n_eos == 0 || (eos_tok && eos_first)) && (n_forced == 0 || forced_tok),
                "logit_rules_rows: a list with a positive length needs its pointer (eos_tok also eos_first)");
    if (rows == 0) return 0;
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, (double)rows * 4.0 * hist_cap, stream);
    hipLaunchKernelGGL(logit_rules_kernel, dim3(rows), dim3(kThreads), 0, stream, X, ldx, n, col, hist, ld_hist, hist_cap, len0, prev_tok, ngram, grp_tok,
                       grp_base, grp_ptr, n_bias, n_groups, seq_ptr, seq_ids, seq_bias, n_seqs, n_ids, ban_tok, n_ban, begin_tok, n_begin, eos_tok, n_eos,
                       eos_first, forced_tok, n_forced, forced_col);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
