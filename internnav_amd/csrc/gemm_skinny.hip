// Skinny-M GEMM for gfx950 (M <= 64) on bf16 weights: C[M,N] = epilogue(A[M,K] . W[N,K]^T) as a WEIGHT-STREAMING kernel.
//
// The kernels, their design notes and the launch rules are gemm_skinny_core.h; this file is the bf16 weight format (its main loops) and the two entries
// behind ina_gemm_bf16 (kernel 32 = ina_launch_gemm_skinny_fused, kernel 30 = ina_launch_gemm_skinny_prenorm with the input RMSNorm).
// Algorithmic bytes per launch = 2*N*K (weights) + 2*M*K + out; roofline = HBM (measured 3.6 - 4.7 TB/s on the LLM shapes,
// profiles/r01i_skinny_gemm_streaming.log; the 25 - 33 MB projections are latency-bound at ~2 TB/s).
#include "gemm_skinny_core.h"

namespace {

// W[N, ldw] bf16, rows in natural k order: a ring slot holds the four MFMA fragments of a K step as they lie in memory. K % 8 == 0 is all
// ina_plan_gemm asks, so the last K step may be partial: fragments at k >= K are zeros
struct SkBf16 {
    static constexpr bool ROW_SCALE = false;
    using Q = void;   // the weights are p.W: a pointer behind the 192 bytes of p would be one more line of kernel arguments to fetch per launch
    using S = void;   // (measured on the o projection, M = 7: 11.2 -> 11.8 us)

    template <int MF, int NT16, int NW, int DEPTH>
    static __device__ __forceinline__ void main_fused(const GemmArgs& p, const void*, const void*, int n0, int w, int nmine, int r16, int g,
                                                      f32x4 (&acc)[NT16][MF]) {
        const bf16* __restrict__ A = reinterpret_cast<const bf16*>(p.A);
        const bf16* __restrict__ W = reinterpret_cast<const bf16*>(p.W);
        const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const bf16* wrow[NT16];
        bool wok[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            const int wn = n0 + t * 16 + r16;
            wok[t] = wn < p.N;
            wrow[t] = W + (size_t)(wok[t] ? wn : 0) * p.ldw;
        }
        const bf16* arow[MF];
        bool aok[MF];
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int m = i * 16 + r16;
            aok[i] = m < p.M;
            arow[i] = A + (size_t)(aok[i] ? m : 0) * p.lda;
        }
        bf16x8 wf[DEPTH][NT16][4], af[DEPTH][MF][4];
        auto load = [&](int j, int slot) {
            const int k0 = (w + j * NW) * SK_BK + g * 8;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = k0 + s * 32;   // load s: the 4 lane groups of a row cover 64 contiguous bytes
                const bool kok = j < nmine && k < p.K;
#pragma unroll
                for (int t = 0; t < NT16; ++t) wf[slot][t][s] = (kok && wok[t]) ? *reinterpret_cast<const bf16x8*>(wrow[t] + k) : zero8;
#pragma unroll
                for (int i = 0; i < MF; ++i) af[slot][i][s] = (kok && aok[i]) ? *reinterpret_cast<const bf16x8*>(arow[i] + k) : zero8;
            }
        };
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) load(d, d);
        for (int j0 = 0; j0 < nmine; j0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {      // static ring slots
#pragma unroll
                for (int t = 0; t < NT16; ++t)
#pragma unroll
                    for (int i = 0; i < MF; ++i)
#pragma unroll
                        for (int s = 0; s < 4; ++s) acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[d][t][s], af[d][i][s], acc[t][i], 0, 0, 0);
                load(j0 + d + DEPTH, d);
            }
        }
    }

    template <int NT16, int NW, int DEPTH, class Norm>
    static __device__ __forceinline__ void main_prenorm(const GemmArgs& p, const void*, const void*, const bf16* img, int lds_ld, int n0, int w,
                                                        int nmine, int r16, int g, f32x4 (&acc)[NT16][1], Norm norm) {
        const bf16* __restrict__ W = reinterpret_cast<const bf16*>(p.W);
        const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const bf16* wrow[NT16];
        bool wok[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            const int wn = n0 + t * 16 + r16;
            wok[t] = wn < p.N;
            wrow[t] = W + (size_t)(wok[t] ? wn : 0) * p.ldw;
        }
        bf16x8 wf[DEPTH][NT16][4];
        auto load_w = [&](int j, int slot) {
            const int k0 = (w + j * NW) * SK_BK + g * 8;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = k0 + s * 32;
                const bool kok = j < nmine && k < p.K;
#pragma unroll
                for (int t = 0; t < NT16; ++t) wf[slot][t][s] = (kok && wok[t]) ? *reinterpret_cast<const bf16x8*>(wrow[t] + k) : zero8;
            }
        };
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) load_w(d, d);
        norm();
        // rows of the MFMA fragment beyond M read a valid row: their outputs are never stored
        const bf16* arow = img + (size_t)(r16 < p.M ? r16 : p.M - 1) * lds_ld + g * 8;
        for (int j0 = 0; j0 < nmine; j0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                const int kb = (w + (j0 + d) * NW) * SK_BK;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = kb + s * 32;
                    const bf16x8 af = (j0 + d < nmine && k + g * 8 < p.K) ? *reinterpret_cast<const bf16x8*>(arow + k) : zero8;
#pragma unroll
                    for (int t = 0; t < NT16; ++t) acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[d][t][s], af, acc[t][0], 0, 0, 0);
                }
                load_w(j0 + d + DEPTH, d);
            }
        }
    }
};

}  // namespace

int ina_launch_gemm_skinny_fused(const GemmArgs& p, hipStream_t stream) {
    InaProfScope prof(INA_PROF_GEMM_SKINNY, 2.0 * p.M * p.N * p.K, sk_prof_bytes(p, 2.0 * p.N * p.K), stream);
    return sk_launch_fused<SkBf16>(p, nullptr, nullptr, stream);
}

int ina_launch_gemm_skinny_prenorm(const GemmArgs& p, hipStream_t stream) {
    InaProfScope prof(INA_PROF_GEMM_SKINNY, 2.0 * p.M * p.N * p.K, sk_prof_bytes(p, 2.0 * p.N * p.K), stream);
    return sk_launch_prenorm<SkBf16>(p, nullptr, nullptr, stream);
}
