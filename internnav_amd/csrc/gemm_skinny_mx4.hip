// MXFP4-weight form of the weight-streaming skinny GEMMs (gemm_skinny_core.h) for gfx950: C[M,N] = epilogue(A[M,K] . (Q[N,K] * 2^E[N,K/32])^T).
//
// Q is OCP e2m1 (two elements per byte) with one OCP e8m0 scale byte per block of 32 consecutive k (ops.mx4_quantize). Every dequantised
// weight q * 2^e (|q| in {0, .5, 1, 1.5, 2, 3, 4, 6}, |e| <= 64) is exactly a bf16 number, and gfx950 converts two e2m1 elements to bf16 with
// the block scale folded in by one instruction, without rounding. So this format MUST give - and tests/test_mx4_gemm_gpu.py asserts - the
// bits of the bf16 format (gemm_skinny.hip) run on the dequantised weights. The kernels, the decomposition, the reduction and the epilogue are gemm_skinny_core.h; the main loop below keeps the bf16 loop's K interleave and MFMA order. What this format decides:
//   * the weight ring holds raw e2m1 - 1 VGPR per MFMA fragment instead of 4 - plus one dword of four scale bytes per K step, and a
//     fragment is converted to bf16 (four packed conversions, the block's scale inside them) just before its MFMA; there is no scale left
//     for the epilogue;
//   * packed layout (ops.mx4_pack; K % 128 == 0): element k = step * 128 + s * 32 + g * 8 + j of a row (MFMA step s, lane group g, lane
//     element j) is nibble j (bits 4j .. 4j + 3) of dword g * 4 + s of the row's 64-byte K step `step`, so a lane fetches its four fragments
//     of a K step as one 16-byte load and the four lane groups of a row cover 64 contiguous bytes;
//   * scales in natural order: byte step * 4 + s of the row's K / 32 scale bytes is block s of K step `step` (e8m0: 127 + e), a lane reads
//     the four of a K step as one dword and the fp32 scale operand of the conversion is byte << 23.
// Algorithmic bytes per launch = N*K/2 + N*K/32 (weights + scales) + activations + out: 0.27 of the bf16 kernels' weight stream.
#include "gemm_skinny_core.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 8 e2m1 nibbles (one dword, nibble j = element j) * 2^(byte - 127) -> one bf16 MFMA fragment; exact (see the header)
__device__ __forceinline__ bf16x8 mx4_frag(unsigned int q, unsigned int scale_byte) {
    const float sc = __uint_as_float(scale_byte << 23);
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 1);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 3);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
__device__ __forceinline__ unsigned int mx4_scale_byte(unsigned int four, int s) { return (four >> (8 * s)) & 0xffu; }

constexpr int MX_BKB = 64;    // packed bytes per K step

// Q[N, ldw] packed e2m1 nibbles (p.ldw = row pitch in bytes; K % 128 == 0: the entry refuses anything else) + scale[N, K / 32] e8m0 bytes.
// A ring slot holds a row's K step as one 16-byte load (fragment s = dword s) and one dword of its four scales (byte s).
// A slot of the ring whose K step lies behind the wave's last one is skipped (wave-uniform): the bf16 kernels multiply zeros there, which
// leaves every accumulator as it is, so skipping is the same bits - and the conversions of those slots are saved.
struct SkMx4 {
    static constexpr bool ROW_SCALE = false;
    using Q = uint8_t;
    using S = uint8_t;

    template <int MF, int NT16, int NW, int DEPTH>
    static __device__ __forceinline__ void main_fused(const GemmArgs& p, const uint8_t* __restrict__ W4, const uint8_t* __restrict__ wscale, int n0, int w, int nmine,
                                                      int r16, int g, f32x4 (&acc)[NT16][MF]) {
        const bf16* __restrict__ A = reinterpret_cast<const bf16*>(p.A);
        const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const u32x4 zero4 = {0u, 0u, 0u, 0u};
        const int spitch = p.K >> 5;
        const uint8_t* wrow[NT16];
        const uint8_t* srow[NT16];
        bool wok[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            const int wn = n0 + t * 16 + r16;
            wok[t] = wn < p.N;
            wrow[t] = W4 + (size_t)(wok[t] ? wn : 0) * p.ldw + g * 16;
            srow[t] = wscale + (size_t)(wok[t] ? wn : 0) * spitch;
        }
        const bf16* arow[MF];
        bool aok[MF];
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int m = i * 16 + r16;
            aok[i] = m < p.M;
            arow[i] = A + (size_t)(aok[i] ? m : 0) * p.lda;
        }
        u32x4 wf[DEPTH][NT16];
        unsigned int ws[DEPTH][NT16];
        bf16x8 af[DEPTH][MF][4];
        auto load = [&](int j, int slot) {
            const bool kok = j < nmine;
            const int ks = w + j * NW;
#pragma unroll
            for (int t = 0; t < NT16; ++t) {
                wf[slot][t] = (kok && wok[t]) ? *reinterpret_cast<const u32x4*>(wrow[t] + (size_t)ks * MX_BKB) : zero4;
                ws[slot][t] = (kok && wok[t]) ? *reinterpret_cast<const unsigned int*>(srow[t] + ks * 4) : 0u;
            }
            const int kb = ks * SK_BK;
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
                if (j0 + d >= nmine) break;        // wave-uniform: nothing but zeros behind the last K step
#pragma unroll
                for (int t = 0; t < NT16; ++t) {
                    bf16x8 wb[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) wb[s] = mx4_frag(wf[d][t][s], mx4_scale_byte(ws[d][t], s));
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
    static __device__ __forceinline__ void main_prenorm(const GemmArgs& p, const uint8_t* __restrict__ W4, const uint8_t* __restrict__ wscale, const bf16* img,
                                                        int lds_ld, int n0, int w, int nmine, int r16, int g, f32x4 (&acc)[NT16][1], Norm norm) {
        const u32x4 zero4 = {0u, 0u, 0u, 0u};
        const int spitch = p.K >> 5;
        const uint8_t* wrow[NT16];
        const uint8_t* srow[NT16];
        bool wok[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            const int wn = n0 + t * 16 + r16;
            wok[t] = wn < p.N;
            wrow[t] = W4 + (size_t)(wok[t] ? wn : 0) * p.ldw + g * 16;
            srow[t] = wscale + (size_t)(wok[t] ? wn : 0) * spitch;
        }
        u32x4 wf[DEPTH][NT16];
        unsigned int ws[DEPTH][NT16];
        auto load_w = [&](int j, int slot) {
            const bool kok = j < nmine;
            const int ks = w + j * NW;
#pragma unroll
            for (int t = 0; t < NT16; ++t) {
                wf[slot][t] = (kok && wok[t]) ? *reinterpret_cast<const u32x4*>(wrow[t] + (size_t)ks * MX_BKB) : zero4;
                ws[slot][t] = (kok && wok[t]) ? *reinterpret_cast<const unsigned int*>(srow[t] + ks * 4) : 0u;
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
                if (j0 + d >= nmine) break;        // wave-uniform: nothing but zeros behind the last K step
                const int kb = (w + (j0 + d) * NW) * SK_BK;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bf16x8 af = *reinterpret_cast<const bf16x8*>(arow + kb + s * 32);
#pragma unroll
                    for (int t = 0; t < NT16; ++t)
                        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mx4_frag(wf[d][t][s], mx4_scale_byte(ws[d][t], s)), af, acc[t][0], 0, 0, 0);
                }
                load_w(j0 + d + DEPTH, d);
            }
        }
    }
};

}  // namespace

// Validation of one ina_gemm_mx4 call: host arithmetic only, before any HIP call (testable without a GPU). `p` receives the defaults.
int ina_plan_gemm_mx4(const GemmArgs& p_in, const void* W4, const void* wscale, GemmArgs& p) {
    INA_REQUIRE(W4 != nullptr && wscale != nullptr, "gemm_mx4: null weight / scale pointer");
    return sk_plan_packed(p_in, p, "gemm_mx4", "MXFP4", [&](const GemmArgs& q) {
        INA_REQUIRE(q.ldw >= q.K / 2 && q.ldw % 16 == 0 && ((uintptr_t)W4 % 16) == 0,
                    "gemm_mx4: packed rows must be 16-byte aligned with a pitch >= K / 2 bytes (ldw=%d K=%d)", q.ldw, q.K);
        INA_REQUIRE(((uintptr_t)wscale % 4) == 0, "gemm_mx4: the scale bytes must be 4-byte aligned (rows of K / 32 contiguous bytes)");
        return 0;
    });
}

// sub-tag of the MXFP4-weight launches inside the weight-streaming class of the profiler tally (ina_prof_read_sub(4, 49, ...))
constexpr int INA_PROF_SUB_MX4 = 49;

int ina_launch_gemm_mx4(const GemmArgs& p_in, const void* W4, const void* wscale, hipStream_t stream) {
    GemmArgs p;
    if (int rc = ina_plan_gemm_mx4(p_in, W4, wscale, p)) return rc;
    const uint8_t *q = reinterpret_cast<const uint8_t*>(W4), *scale = reinterpret_cast<const uint8_t*>(wscale);
    ina_prof_set_sub(INA_PROF_SUB_MX4);
    InaProfScope prof(INA_PROF_GEMM_SKINNY, 2.0 * p.M * p.N * p.K, sk_prof_bytes(p, (double)p.N * p.K / 2 + (double)p.N * p.K / 32), stream);
    return p.norm_gamma ? sk_launch_prenorm<SkMx4>(p, q, scale, stream) : sk_launch_fused<SkMx4>(p, q, scale, stream);
}
