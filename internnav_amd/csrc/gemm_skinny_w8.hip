// FP8-weight form of the weight-streaming skinny GEMMs (gemm_skinny_core.h) for gfx950: C[M,N] = epilogue(2^wexp[n] * (A[M,K] . Q[N,K]^T)).
//
// Q is OCP e4m3 (e4m3fn: gfx950's native fp8, not MI300X's fnuz), one byte per weight, with a power-of-two scale 2^wexp[n] per output row
// (ops.w8_quantize). Every dequantised weight q * 2^e is exactly a bf16 number, products of bf16 values are exact in fp32 and scaling an
// fp32 sum by a power of two is exact, so this format MUST give - and tests/test_w8_gemm_gpu.py asserts - the bits of the bf16 format
// (gemm_skinny.hip) run on the dequantised weights. The kernels, the decomposition, the reduction and the epilogue are gemm_skinny_core.h; the main loop below keeps the bf16 loop's K interleave and MFMA order. What this format decides:
//   * the weight ring holds raw fp8 - 2 VGPRs per MFMA fragment instead of 4 - and a fragment is converted to bf16 (one packed
//     fp8 -> bf16 conversion per two elements) just before its MFMA;
//   * packed layout (ops.w8_pack; K % 128 == 0): element k = step * 128 + s * 32 + g * 8 + j of a row (MFMA step s, lane group g, lane element j)
//     is byte step * 128 + g * 32 + s * 8 + j, so a lane fetches the 32 bytes of its four fragments of a K step as two 16-byte loads and the
//     four lane groups of a row cover 128 contiguous bytes (the contiguity lesson of gemm_skinny_core.h, at one byte per weight);
//   * the row scale multiplies the reduced fp32 sum in front of the epilogue, before the bias (GLU: gate and up rows by their own exponents
//     before the activation).
// Algorithmic bytes per launch = N*K + N (weights + exponents) + activations + out: half the bf16 kernels' weight stream.
#include "gemm_skinny_core.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 8 e4m3 bytes (two dwords, byte j = element j) -> one bf16 MFMA fragment; exact (every e4m3 value is a bf16 value)
__device__ __forceinline__ bf16x8 w8_frag(unsigned int lo, unsigned int hi) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// Q[N, ldw] packed e4m3 bytes (p.ldw = row pitch in bytes; K % 128 == 0: the entry refuses anything else) + wexp[N]. A ring slot holds a
// row's K step as two 16-byte halves: fragment s = dwords (s & 1) * 2, + 1 of half s >> 1
struct SkFp8 {
    static constexpr bool ROW_SCALE = true;
    using Q = uint8_t;
    using S = int8_t;   // wexp
    // 2^e for |e| <= 64 (the quantiser's clamp): a normal fp32
    static __device__ __forceinline__ float row_scale(const int8_t* __restrict__ wexp, int n) { return __int_as_float((127 + wexp[n]) << 23); }

    template <int MF, int NT16, int NW, int DEPTH>
    static __device__ __forceinline__ void main_fused(const GemmArgs& p, const uint8_t* __restrict__ W8, const int8_t*, int n0, int w, int nmine, int r16, int g,
                                                      f32x4 (&acc)[NT16][MF]) {
        const bf16* __restrict__ A = reinterpret_cast<const bf16*>(p.A);
        const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const u32x4 zero4 = {0u, 0u, 0u, 0u};
        const uint8_t* wrow[NT16];
        bool wok[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            const int wn = n0 + t * 16 + r16;
            wok[t] = wn < p.N;
            wrow[t] = W8 + (size_t)(wok[t] ? wn : 0) * p.ldw + g * 32;
        }
        const bf16* arow[MF];
        bool aok[MF];
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int m = i * 16 + r16;
            aok[i] = m < p.M;
            arow[i] = A + (size_t)(aok[i] ? m : 0) * p.lda;
        }
        u32x4 wf[DEPTH][NT16][2];
        bf16x8 af[DEPTH][MF][4];
        auto load = [&](int j, int slot) {
            const bool kok = j < nmine;
            const int kb = (w + j * NW) * SK_BK;
#pragma unroll
            for (int t = 0; t < NT16; ++t)
#pragma unroll
                for (int h = 0; h < 2; ++h) wf[slot][t][h] = (kok && wok[t]) ? *reinterpret_cast<const u32x4*>(wrow[t] + kb + h * 16) : zero4;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < MF; ++i) af[slot][i][s] = (kok && aok[i]) ? *reinterpret_cast<const bf16x8*>(arow[i] + kb + s * 32 + g * 8) : zero8;
        };
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) load(d, d);
        for (int j0 = 0; j0 < nmine; j0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {      // static ring slots
#pragma unroll
                for (int t = 0; t < NT16; ++t) {
                    bf16x8 wb[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) wb[s] = w8_frag(wf[d][t][s >> 1][(s & 1) * 2], wf[d][t][s >> 1][(s & 1) * 2 + 1]);
#pragma unroll
                    for (int i = 0; i < MF; ++i)
#pragma unroll
                        for (int s = 0; s < 4; ++s) acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[s], af[d][i][s], acc[t][i], 0, 0, 0);
                }
                load(j0 + d + DEPTH, d);
            }
        }
    }

    template <int NT16, int NW, int DEPTH, class Norm>
    static __device__ __forceinline__ void main_prenorm(const GemmArgs& p, const uint8_t* __restrict__ W8, const int8_t*, const bf16* img, int lds_ld, int n0,
                                                        int w, int nmine, int r16, int g, f32x4 (&acc)[NT16][1], Norm norm) {
        const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const u32x4 zero4 = {0u, 0u, 0u, 0u};
        const uint8_t* wrow[NT16];
        bool wok[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            const int wn = n0 + t * 16 + r16;
            wok[t] = wn < p.N;
            wrow[t] = W8 + (size_t)(wok[t] ? wn : 0) * p.ldw + g * 32;
        }
        u32x4 wf[DEPTH][NT16][2];
        auto load_w = [&](int j, int slot) {
            const bool kok = j < nmine;
            const int kb = (w + j * NW) * SK_BK;
#pragma unroll
            for (int t = 0; t < NT16; ++t)
#pragma unroll
                for (int h = 0; h < 2; ++h) wf[slot][t][h] = (kok && wok[t]) ? *reinterpret_cast<const u32x4*>(wrow[t] + kb + h * 16) : zero4;
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
                    const bf16x8 af = (j0 + d < nmine) ? *reinterpret_cast<const bf16x8*>(arow + kb + s * 32) : zero8;   // (LDS behind the image is anything)
#pragma unroll
                    for (int t = 0; t < NT16; ++t)
                        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w8_frag(wf[d][t][s >> 1][(s & 1) * 2], wf[d][t][s >> 1][(s & 1) * 2 + 1]), af, acc[t][0], 0, 0, 0);
                }
                load_w(j0 + d + DEPTH, d);
            }
        }
    }
};

}  // namespace

// Validation of one ina_gemm_w8 call: host arithmetic only, before any HIP call (testable without a GPU). `p` receives the defaults.
int ina_plan_gemm_w8(const GemmArgs& p_in, const void* W8, const int8_t* wexp, GemmArgs& p) {
    INA_REQUIRE(W8 != nullptr && wexp != nullptr, "gemm_w8: null weight / exponent pointer");
    return sk_plan_packed(p_in, p, "gemm_w8", "fp8", [&](const GemmArgs& q) {
        INA_REQUIRE(q.ldw >= q.K && q.ldw % 16 == 0 && ((uintptr_t)W8 % 16) == 0, "gemm_w8: packed rows must be 16-byte aligned with a pitch >= K bytes (ldw=%d K=%d)", q.ldw, q.K);
        return 0;
    });
}

// sub-tag of the fp8-weight launches inside the weight-streaming class of the profiler tally (ina_prof_read_sub(4, 48, ...))
constexpr int INA_PROF_SUB_W8 = 48;

int ina_launch_gemm_w8(const GemmArgs& p_in, const void* W8, const int8_t* wexp, hipStream_t stream) {
    GemmArgs p;
    if (int rc = ina_plan_gemm_w8(p_in, W8, wexp, p)) return rc;
    const uint8_t* q = reinterpret_cast<const uint8_t*>(W8);
    ina_prof_set_sub(INA_PROF_SUB_W8);
    InaProfScope prof(INA_PROF_GEMM_SKINNY, 2.0 * p.M * p.N * p.K, sk_prof_bytes(p, (double)p.N * p.K + p.N), stream);
    return p.norm_gamma ? sk_launch_prenorm<SkFp8>(p, q, wexp, stream) : sk_launch_fused<SkFp8>(p, q, wexp, stream);
}
