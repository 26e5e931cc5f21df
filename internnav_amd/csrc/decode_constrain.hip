// Constrained System-2 decoding (gfx950): a deterministic automaton over token CLASSES that lives on the device, consulted in front of the
// unchanged selection kernels (argmax_rows, argmax_penalty_rows, logprob_rows, sample_rows: all of them treat -inf as "mass 0, never chosen").
//   automaton_mask_rows  per row: advance the row's state by the token the previous step chose, then write -inf over every logit whose
//                        class the new state does not allow
// Tables: token_class u8 [vocab]; allow u32 [S, 8] (class c = bit c & 31 of word c >> 5); next u8 [S, 256].
// state_in and state_out are DISTINCT buffers (the engine ping-pongs two by step parity), so every workgroup of a row derives the new state
// itself from state_in / prev_tok and a row spreads over many workgroups with no reduction and no atomics; workgroup 0 of the row is the one
// writer of state_out[r]. The logits are never READ: a banned entry is stored, an allowed one is not touched (a NaN there stays that NaN).
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                           // class words (4 columns each) in flight per thread
constexpr int kCols = kThreads * kUnroll * 4;        // columns of a row per workgroup: 4096 (152064 columns = 38 workgroups per row)

__device__ __forceinline__ bool banned(const uint32_t* al, uint32_t c) { return !((al[c >> 5] >> (c & 31u)) & 1u); }

// the four columns 4j .. 4j + 3 of an aligned row; cw = their four classes (byte q = column 4j + q)
__device__ __forceinline__ void mask4(float* x, const uint32_t* al, uint32_t cw) {
    const bool b0 = banned(al, cw & 255u), b1 = banned(al, (cw >> 8) & 255u), b2 = banned(al, (cw >> 16) & 255u), b3 = banned(al, cw >> 24);
    if (b0 && b1 && b2 && b3) {
        *reinterpret_cast<f32x4*>(x) = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    } else {
        if (b0) x[0] = -INFINITY;
        if (b1) x[1] = -INFINITY;
        if (b2) x[2] = -INFINITY;
        if (b3) x[3] = -INFINITY;
    }
}

__global__ __launch_bounds__(kThreads) void automaton_mask_kernel(float* __restrict__ X, int ldx, int n, const uint8_t* __restrict__ cls,
                                                                  const uint32_t* __restrict__ allow, const uint8_t* __restrict__ next, int S,
                                                                  const int32_t* __restrict__ state_in, const int32_t* __restrict__ prev_tok,
                                                                  int32_t* __restrict__ state_out) {
    __shared__ uint32_t al[8];
    const int r = blockIdx.y;
    // advance: the same few loads at row-uniform addresses in every workgroup of the row; no index is used before it is range-checked
    int s = state_in[r];
    if (prev_tok) {
        const int t = prev_tok[r];
        int s1 = -1;
        if ((unsigned)s < (unsigned)S && (unsigned)t < (unsigned)n) {
            const uint32_t c = cls[t];
            if ((allow[s * 8 + (c >> 5)] >> (c & 31u)) & 1u) s1 = next[s * 256 + c];
        }
        s = s1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) state_out[r] = s;
    if ((unsigned)s >= (unsigned)S) return;                          // (whole workgroup: s is the same in every thread) the row stays as it is
    if (threadIdx.x < 8) al[threadIdx.x] = allow[s * 8 + threadIdx.x];
    __syncthreads();
    float* x = X + (size_t)r * ldx;
    const int c0 = blockIdx.x * kCols;                               // a multiple of 4
    const int c1 = c0 + kCols < n ? c0 + kCols : n;
    const int v1 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? (c1 & ~3) : c0;     // [c0, v1): 16-byte stores, [v1, c1): single ones
    int i = c0 + 4 * threadIdx.x;
    for (; i + (kUnroll - 1) * 4 * kThreads < v1; i += kUnroll * 4 * kThreads) {
        uint32_t cw[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) cw[u] = *reinterpret_cast<const uint32_t*>(cls + i + u * 4 * kThreads);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) mask4(x + i + u * 4 * kThreads, al, cw[u]);
    }
    for (; i < v1; i += 4 * kThreads) mask4(x + i, al, *reinterpret_cast<const uint32_t*>(cls + i));
    for (int j = v1 + threadIdx.x; j < c1; j += kThreads)
        if (banned(al, cls[j])) x[j] = -INFINITY;
}

}  // namespace

int ina_launch_automaton_mask(float* X, int ldx, int rows, int n, const uint8_t* token_class, int vocab, const uint32_t* allow, const uint8_t* next,
                              int n_states, const int32_t* state_in, const int32_t* prev_tok, int32_t* state_out, hipStream_t stream) {
    INA_REQUIRE(X && token_class && allow && next && state_in && state_out, "automaton_mask_rows: X, token_class, allow, next, state_in and state_out required");
    INA_REQUIRE(rows >= 0 && rows <= 65535 && n >= 1 && ldx >= n, "automaton_mask_rows: bad arguments rows=%d n=%d ldx=%d (0 <= rows <= 65535, n >= 1, ldx >= n)",
                rows, n, ldx);
    INA_REQUIRE(n <= vocab, "automaton_mask_rows: n=%d columns exceed the %d entries of token_class", n, vocab);
    INA_REQUIRE(n_states >= 1 && n_states <= 256, "automaton_mask_rows: %d states (1 .. 256)", n_states);
    INA_REQUIRE((reinterpret_cast<uintptr_t>(token_class) & 3) == 0, "automaton_mask_rows: token_class must be 4-byte aligned");
    INA_REQUIRE(state_out + rows <= state_in || state_in + rows <= state_out, "automaton_mask_rows: state_in and state_out must not overlap");
    if (rows == 0) return 0;
    InaProfScope prof(INA_PROF_ELEMENTWISE, 0.0, (double)rows * 5.0 * n, stream);
    hipLaunchKernelGGL(automaton_mask_kernel, dim3((n + kCols - 1) / kCols, rows), dim3(kThreads), 0, stream, X, ldx, n, token_class, allow, next, n_states,
                       state_in, prev_tok, state_out);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
