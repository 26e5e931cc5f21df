// MXFP4-weight forms of the weight-streaming skinny GEMMs (gemm_skinny.hip) for gfx950: C[M,N] = epilogue(A[M,K] . (Q[N,K] * 2^E[N,K/32])^T).
//
// Q is OCP e2m1 (two elements per byte) with one OCP e8m0 scale byte per block of 32 consecutive k (ops.mx4_quantize). Every dequantised
// weight q * 2^e (|q| in {0, .5, 1, 1.5, 2, 3, 4, 6}, |e| <= 64) is exactly a bf16 number, and gfx950 converts two e2m1 elements to bf16 with
// the block scale folded in by one instruction, without rounding. So these kernels MUST give - and tests/test_mx4_gemm_gpu.py asserts - the
// bits of gemm_skinny_fused_kernel / gemm_skinny_prenorm_kernel run on the dequantised bf16 weights. To that end the decomposition is
// theirs: 16-column tiles (32 interleaved gate | up rows for GLU), the group width of sk_group_waves / sk_group_waves_prenorm, 128-wide K
// steps interleaved over the group's waves, the four 16x16x32 bf16 MFMAs of a step in the same order, the LDS reduction in ascending slice
// order from 0.0f, the same epilogue. What differs:
//   * the weight ring holds raw e2m1 - 1 VGPR per MFMA fragment instead of 4 - plus one dword of four scale bytes per K step, and a
//     fragment is converted to bf16 (four packed conversions, the block's scale inside them) just before its MFMA; there is no scale left
//     for the epilogue;
//   * packed layout (ops.mx4_pack; K % 128 == 0): element k = step * 128 + s * 32 + g * 8 + j of a row (MFMA step s, lane group g, lane
//     element j) is nibble j (bits 4j .. 4j + 3) of dword g * 4 + s of the row's 64-byte K step `step`, so a lane fetches its four fragments
//     of a K step as one 16-byte load and the four lane groups of a row cover 64 contiguous bytes;
//   * scales in natural order: byte step * 4 + s of the row's K / 32 scale bytes is block s of K step `step` (e8m0: 127 + e), a lane reads
//     the four of a K step as one dword and the fp32 scale operand of the conversion is byte << 23.
// A slot of the ring whose K step lies behind the wave's last one is skipped (wave-uniform): the bf16 kernels multiply zeros there, which
// leaves every accumulator as it is, so skipping is the same bits - and the conversions of those slots are saved.
// Algorithmic bytes per launch = N*K/2 + N*K/32 (weights + scales) + activations + out: 0.27 of the bf16 kernels' weight stream.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SK_BK = 128;    // K elements per step
constexpr int MX_BKB = 64;    // packed bytes per step

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// the same two rules as gemm_skinny.hip (kept in step with it: the slice count decides the summation order)
inline int sk_group_waves(int tiles, int ksteps) {
    int nw = tiles >= 4096 ? 1 : tiles >= 2048 ? 2 : tiles >= 1024 ? 4 : 8;
    while (nw > 1 && nw > ksteps) nw >>= 1;
    return nw;
}
inline int sk_group_waves_prenorm(int tiles, int ksteps) {
    const int nw = sk_group_waves(tiles, ksteps);
    return nw < 4 ? 4 : nw;
}

// 8 e2m1 nibbles (one dword, nibble j = element j) * 2^(byte - 127) -> one bf16 MFMA fragment; exact (see the header)
__device__ __forceinline__ bf16x8 mx4_frag(unsigned int q, unsigned int scale_byte) {
    const float sc = __uint_as_float(scale_byte << 23);
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 1);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 3);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
__device__ __forceinline__ unsigned int mx4_scale_byte(unsigned int four, int s) { return (four >> (8 * s)) & 0xffu; }

// RMSNorm of the <= 16 activation rows into the LDS image: gemm_skinny.hip's sk_prenorm_rows, restated so that both files hand the MFMAs
// bit-identical operands (per lane fma in ascending chunk / element order, the xor butterfly of wave_sum, bf16(v * rstd * gamma))
template <int NWAVES>
__device__ __forceinline__ void mx4_prenorm_rows(const GemmArgs& p, bf16* img, int lds_ld, int wave, int lane) {
    const int nch = p.K >> 3;
    const float invK = 1.0f / (float)p.K;
    const bool a32 = p.a_dtype == INA_DT_F32;
    auto load8 = [&](int m, int c, float (&v)[8]) {
        if (a32) {
            const float* q = reinterpret_cast<const float*>(p.A) + (size_t)m * p.lda + c * 8;
            const f32x4 a = *reinterpret_cast<const f32x4*>(q), b = *reinterpret_cast<const f32x4*>(q + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
        } else {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16*>(p.A) + (size_t)m * p.lda + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
        }
    };
    for (int m = wave; m < p.M; m += NWAVES) {          // wave-uniform
        float sq = 0.f;
        for (int c = lane; c < nch; c += 64) {
            float v[8];
            load8(m, c, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) sq = fmaf(v[j], v[j], sq);
        }
        const float rstd = rsqrtf(fmaf(wave_sum(sq), invK, p.norm_eps));
        for (int c = lane; c < nch; c += 64) {
            float v[8];
            load8(m, c, v);
            const f32x4 ga = *reinterpret_cast<const f32x4*>(p.norm_gamma + c * 8), gb = *reinterpret_cast<const f32x4*>(p.norm_gamma + c * 8 + 4);
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = (bf16)(v[j] * rstd * ga[j]);
                o[4 + j] = (bf16)(v[4 + j] * rstd * gb[j]);
            }
            *reinterpret_cast<bf16x8*>(img + (size_t)m * lds_ld + c * 8) = o;
        }
    }
}

// epilogue of one lane's 4 output columns of row m (m < M, n < N checked by the caller): gemm_skinny.hip's order (the scales are spent)
template <int NT16>
__device__ __forceinline__ void mx4_epilogue(const GemmArgs& p, const f32x4 (&sum)[NT16], int m, int n, int n0, int g) {
    const float rs = p.rowscale ? p.rowscale[m / p.rowscale_div] : 1.0f;
    float v[4];
    int no = n;
    if constexpr (NT16 == 2) {
        // GLU: tile 0 = gate rows, tile 1 = up rows of the interleaved weight; output column block = pair index
        no = (n0 >> 1) + g * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float gg = sum[0][r], uu = sum[1][r];
            if (p.bias) { gg += p.bias[n + r]; uu += p.bias[n + 16 + r]; }
            v[r] = ina_act(gg, p.act) * uu * rs;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float x = sum[0][r];
            if (p.bias) x += p.bias[n + r];
            x = ina_act(x, p.act);
            if (p.colscale) x *= p.colscale[n + r];
            v[r] = x * rs;
        }
        if (p.R) {
            const size_t ro = (size_t)m * p.ldr + n;
            if (p.res_dtype == INA_DT_BF16) {
                const bf16x4 rr = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(p.R) + ro);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (float)rr[r];
            } else {
                const f32x4 rr = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.R) + ro);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += rr[r];
            }
        }
    }
    const size_t co = (size_t)m * p.ldc + no;
    if (p.out_dtype == INA_DT_BF16) *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(p.C) + co) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
    else *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + co) = f32x4{v[0], v[1], v[2], v[3]};
}

// ---- column owners (M <= 64): gemm_skinny_fused_kernel with an e2m1 weight ring. p.ldw = packed row pitch in bytes; scale rows K / 32 bytes.
template <int MF, int NT16, int NW, int NC, int DEPTH>
__global__ __launch_bounds__(NW * NC * 64) void gemm_skinny_mx4_fused_kernel(GemmArgs p, const uint8_t* __restrict__ W4, const uint8_t* __restrict__ wscale) {
    __shared__ __attribute__((aligned(16))) float red[NW > 1 ? NC : 1][NW > 1 ? NW : 1][NT16][MF][64 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = wave / NW, w = wave % NW;
    const int n0 = (blockIdx.x * NC + grp) * (16 * NT16);
    const int r16 = lane & 15, g = lane >> 4;
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
    f32x4 acc[NT16][MF];
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
        for (int i = 0; i < MF; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int ksteps = p.K / SK_BK;                                   // (K % 128 == 0: the entry refuses anything else)
    const int nmine = w < ksteps ? (ksteps - w + NW - 1) / NW : 0;   // K steps w, w + NW, ...
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
    // ---- cross-wave reduction (NW > 1) + epilogue: wave w of a group owns row fragments w, w + NW, ... of every column tile
    if constexpr (NW > 1) {
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int i = 0; i < MF; ++i) *reinterpret_cast<f32x4*>(&red[grp][w][t][i][lane * 4]) = acc[t][i];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        if (NW > 1 && (i % NW) != w) continue;
        const int m = i * 16 + r16;
        f32x4 sum[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            if constexpr (NW > 1) {
                sum[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ww = 0; ww < NW; ++ww) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(&red[grp][ww][t][i][lane * 4]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum[t][r] += v[r];
                }
            } else {
                sum[t] = acc[t][i];
            }
        }
        const int n = n0 + g * 4;
        if (m >= p.M || n >= p.N) continue;
        mx4_epilogue<NT16>(p, sum, m, n, n0, g);
    }
}

template <int MF, int NT16>
void launch_mx4_fused(const GemmArgs& p, const uint8_t* W4, const uint8_t* wscale, hipStream_t stream) {
    const int ksteps = p.K / SK_BK;
    const int tiles = (p.N + 16 * NT16 - 1) / (16 * NT16);
    // ring depth: the fp8 kernels'. Measured at M = 7 on the four layer shapes of the 7B geometry, these depths / twice them where the
    // registers allow / four times them in the prenorm form: q|k|v 12.2 / 12.2 / 12.0 us, o 9.8 / 10.6 / 9.8 (one process each; fp8 moved
    // alike), gate|up 30.9 / 31.2 / 39.2, down 20.3 / 20.4 / 20.5 - half the bytes per slot do not ask for more slots
    constexpr int DEEP = (MF <= 2 && NT16 == 1) ? 4 : 2;
    constexpr int D = 2;
    const int nw = sk_group_waves(tiles, ksteps);
#define INA_SKMX4(NW_, NC_, D_) hipLaunchKernelGGL((gemm_skinny_mx4_fused_kernel<MF, NT16, NW_, NC_, D_>), dim3((tiles + NC_ - 1) / NC_), dim3(NW_ * NC_ * 64), 0, stream, p, W4, wscale)
    if (nw == 1) INA_SKMX4(1, 4, D);
    else if (nw == 2) INA_SKMX4(2, 2, D);
    else if (nw == 4) INA_SKMX4(4, 1, D);
    else INA_SKMX4(8, 1, DEEP);
#undef INA_SKMX4
}

// ---- column owners with the input RMSNorm fused in front (M <= 16): gemm_skinny_prenorm_kernel with an e2m1 weight ring
template <int NT16, int NW, int NC, int DEPTH>
__global__ __launch_bounds__(NW * NC * 64) void gemm_skinny_mx4_prenorm_kernel(GemmArgs p, const uint8_t* __restrict__ W4, const uint8_t* __restrict__ wscale) {
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    constexpr int NWAVES = NW * NC;
    const int lds_ld = p.K + 8;
    bf16* img = reinterpret_cast<bf16*>(sk_smem);                                                     // [M][K + 8]
    float* red = reinterpret_cast<float*>(sk_smem + (((size_t)p.M * lds_ld * sizeof(bf16) + 15) & ~size_t(15)));   // [NC][NW][NT16][256]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wave / NW, w = wave % NW;
    const int n0 = (blockIdx.x * NC + grp) * (16 * NT16);
    const int r16 = lane & 15, g = lane >> 4;
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
    f32x4 acc[NT16];
#pragma unroll
    for (int t = 0; t < NT16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = p.K / SK_BK;
    const int nmine = w < ksteps ? (ksteps - w + NW - 1) / NW : 0;
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

    mx4_prenorm_rows<NWAVES>(p, img, lds_ld, wave, lane);   // (the weight ring is in flight meanwhile)
    __syncthreads();

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
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mx4_frag(wf[d][t][s], mx4_scale_byte(ws[d][t], s)), af, acc[t], 0, 0, 0);
            }
            load_w(j0 + d + DEPTH, d);
        }
    }
    if constexpr (NW > 1) {
#pragma unroll
        for (int t = 0; t < NT16; ++t) *reinterpret_cast<f32x4*>(&red[(((size_t)grp * NW + w) * NT16 + t) * 256 + lane * 4]) = acc[t];
        __syncthreads();
        if (w != 0) return;        // one 16-row fragment: wave 0 of the group reduces and stores
    }
    const int m = r16, n = n0 + g * 4;
    f32x4 sum[NT16];
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
        if constexpr (NW > 1) {
            sum[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&red[(((size_t)grp * NW + ww) * NT16 + t) * 256 + lane * 4]);
#pragma unroll
                for (int r = 0; r < 4; ++r) sum[t][r] += v[r];
            }
        } else {
            sum[t] = acc[t];
        }
    }
    if (m >= p.M || n >= p.N) return;
    mx4_epilogue<NT16>(p, sum, m, n, n0, g);
}

template <int NT16, int NW, int NC, int DEPTH>
int launch_mx4_prenorm(const GemmArgs& p, const uint8_t* W4, const uint8_t* wscale, hipStream_t stream, int tiles) {
    const size_t lds = (((size_t)p.M * (p.K + 8) * sizeof(bf16) + 15) & ~size_t(15)) + (NW > 1 ? size_t(NC) * NW * NT16 * 256 * sizeof(float) : 0);
    auto kern = gemm_skinny_mx4_prenorm_kernel<NT16, NW, NC, DEPTH>;
    static size_t attr = 0;
    if (lds > attr) {
        INA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = lds;
    }
    hipLaunchKernelGGL(kern, dim3((tiles + NC - 1) / NC), dim3(NW * NC * 64), lds, stream, p, W4, wscale);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

// Validation of one ina_gemm_mx4 call: host arithmetic only, before any HIP call (testable without a GPU). `p` receives the defaults.
int ina_plan_gemm_mx4(const GemmArgs& p_in, const void* W4, const void* wscale, GemmArgs& p) {
    p = p_in;
    if (p.rowscale_div <= 0) p.rowscale_div = 1;
    if (p.batch <= 0) p.batch = 1;
    INA_REQUIRE(W4 != nullptr && wscale != nullptr, "gemm_mx4: null weight / scale pointer");
    INA_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "gemm_mx4: empty problem M=%d N=%d K=%d", p.M, p.N, p.K);
    INA_REQUIRE(p.M <= 64, "gemm_mx4: the MXFP4-weight kernels are weight-streaming kernels for M <= 64 rows (M=%d)", p.M);
    INA_REQUIRE(p.K % 128 == 0, "gemm_mx4: the packed MXFP4 layout needs K %% 128 == 0 (K=%d)", p.K);
    INA_REQUIRE(p.batch == 1, "gemm_mx4: no batched form (batch=%d)", p.batch);
    INA_REQUIRE(!p.seg_stats, "gemm_mx4: seg_stats exist in the row-panel kernels only");
    INA_REQUIRE(!p.Wp, "gemm_mx4: Wp (fragment-ordered bf16 weights) has no meaning here");
    INA_REQUIRE(p.force_cfg == 0 || p.force_cfg == -1, "gemm_mx4: no tile configs to force (force_cfg %d)", p.force_cfg);
    INA_REQUIRE(p.ldw >= p.K / 2 && p.ldw % 16 == 0 && ((uintptr_t)W4 % 16) == 0,
                "gemm_mx4: packed rows must be 16-byte aligned with a pitch >= K / 2 bytes (ldw=%d K=%d)", p.ldw, p.K);
    INA_REQUIRE(((uintptr_t)wscale % 4) == 0, "gemm_mx4: the scale bytes must be 4-byte aligned (rows of K / 32 contiguous bytes)");
    INA_REQUIRE(p.lda % 8 == 0, "gemm_mx4: lda must be a multiple of 8 (lda=%d)", p.lda);
    INA_REQUIRE(p.N % 4 == 0 && p.ldc % 4 == 0, "gemm_mx4: N/ldc must be multiples of 4 (N=%d ldc=%d)", p.N, p.ldc);
    INA_REQUIRE(((uintptr_t)p.A % 16) == 0 && ((uintptr_t)p.C % 8) == 0, "gemm_mx4: misaligned pointer");
    INA_REQUIRE(!p.R || p.ldr % 4 == 0, "gemm_mx4: ldr must be a multiple of 4");
    INA_REQUIRE(!p.glu || (p.N % 32 == 0), "gemm_mx4: GLU mode needs N %% 32 == 0");
    INA_REQUIRE(p.act >= INA_ACT_NONE && p.act <= INA_ACT_TANH, "gemm_mx4: act=%d is not an activation code (0 .. %d)", p.act, (int)INA_ACT_TANH);
    INA_REQUIRE(!p.glu || !p.R, "gemm_mx4: glu cannot be combined with a residual (R)");
    INA_REQUIRE(!p.glu || !p.colscale, "gemm_mx4: glu cannot be combined with colscale");
    if (p.norm_gamma) {
        INA_REQUIRE(p.M <= 16 && p.K <= 4096 && p.N >= 256,
                    "gemm_mx4: the fused input RMSNorm is built for the decode passes (M <= 16 rows, K <= 4096): M=%d K=%d N=%d", p.M, p.K, p.N);
        INA_REQUIRE(p.a_dtype == INA_DT_BF16 || p.a_dtype == INA_DT_F32, "gemm_mx4: a_dtype must be bf16 or f32 with norm_gamma");
        INA_REQUIRE(((uintptr_t)p.norm_gamma % 16) == 0 && (p.lda % (p.a_dtype == INA_DT_F32 ? 4 : 8)) == 0, "gemm_mx4(prenorm): misaligned gamma / lda");
    }
    return 0;
}

// sub-tag of the MXFP4-weight launches inside the weight-streaming class of the profiler tally (ina_prof_read_sub(4, 49, ...))
constexpr int INA_PROF_SUB_MX4 = 49;

int ina_launch_gemm_mx4(const GemmArgs& p_in, const void* W4v, const void* wscalev, hipStream_t stream) {
    GemmArgs p;
    if (int rc = ina_plan_gemm_mx4(p_in, W4v, wscalev, p)) return rc;
    const uint8_t* W4 = reinterpret_cast<const uint8_t*>(W4v);
    const uint8_t* wscale = reinterpret_cast<const uint8_t*>(wscalev);
    const double osz = p.out_dtype == INA_DT_BF16 ? 2.0 : 4.0, asz = (p.norm_gamma && p.a_dtype == INA_DT_F32) ? 4.0 : 2.0;
    ina_prof_set_sub(INA_PROF_SUB_MX4);
    InaProfScope prof(INA_PROF_GEMM_SKINNY, 2.0 * p.M * p.N * p.K, asz * p.M * p.K + ((double)p.N * p.K / 2 + (double)p.N * p.K / 32) + osz * p.M * (p.glu ? p.N / 2 : p.N), stream);
    const int ksteps = p.K / SK_BK;
    if (p.norm_gamma) {
        if (p.glu) {
            const int tiles = (p.N + 31) / 32;
            if (sk_group_waves_prenorm(tiles, ksteps) == 4) return launch_mx4_prenorm<2, 4, 2, 2>(p, W4, wscale, stream, tiles);
            return launch_mx4_prenorm<2, 8, 1, 2>(p, W4, wscale, stream, tiles);
        }
        const int tiles = (p.N + 15) / 16;
        if (sk_group_waves_prenorm(tiles, ksteps) == 4) return launch_mx4_prenorm<1, 4, 2, 2>(p, W4, wscale, stream, tiles);
        return launch_mx4_prenorm<1, 8, 1, 4>(p, W4, wscale, stream, tiles);
    }
    const int mf = (p.M + 15) / 16;
    if (p.glu) {
        switch (mf) {
            case 1: launch_mx4_fused<1, 2>(p, W4, wscale, stream); break;
            case 2: launch_mx4_fused<2, 2>(p, W4, wscale, stream); break;
            case 3: launch_mx4_fused<3, 2>(p, W4, wscale, stream); break;
            default: launch_mx4_fused<4, 2>(p, W4, wscale, stream); break;
        }
    } else {
        switch (mf) {
            case 1: launch_mx4_fused<1, 1>(p, W4, wscale, stream); break;
            case 2: launch_mx4_fused<2, 1>(p, W4, wscale, stream); break;
            case 3: launch_mx4_fused<3, 1>(p, W4, wscale, stream); break;
            default: launch_mx4_fused<4, 1>(p, W4, wscale, stream); break;
        }
    }
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
