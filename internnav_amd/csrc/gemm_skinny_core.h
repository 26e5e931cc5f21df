// The kernel core of the weight-streaming skinny GEMMs (M <= 64) for gfx950: C[M,N] = epilogue(A[M,K] . W[N,K]^T), for the bf16
// weights of gemm_skinny.hip and the quantised weights of gemm_skinny_w8.hip (e4m3 + 2^e per row) and gemm_skinny_mx4.hip (MXFP4).
//
// Used by the decode steps of the System-2 LLM (M = number of sequences), the latent-query pass, lm_head on the last position
// and the adaLN modulation GEMMs. At M <= 64 the op is HBM-bound: every weight byte is read once and used for M <= 64 MACs, so
// the design goal is bytes/s, not MFMA utilisation. Common to both kernels:
//   * W is streamed straight from HBM into VGPRs (no LDS round trip: each weight element is used by exactly one wave). Every load
//     instruction of a wave covers a CONTIGUOUS run of each of its 16 rows: for bf16 4 x 16-byte loads per lane per 128-wide K step, load s
//     covering 64 bytes of a row (k = k0 + s*32 + g*8, the natural MFMA k order). The first version gave every lane 64 contiguous bytes
//     instead, i.e. 4 scattered 16-byte pieces per row per instruction: 3.3 -> 4.0 TB/s on the gate/up projection, 3.8 -> 4.9 TB/s on lm_head
//     from this change alone. The packed layouts of the quantised formats keep that property at one and at half a byte per weight;
//   * the activation rows (M x K bf16, <= 2.4 MB, L2 resident) are read directly as the second MFMA operand;
//   * one summation order per output element: K is cut into 128-wide steps, step j belongs to slice j % NS (NS = sk_group_waves(column
//     tiles, K steps): 1 / 2 / 4 / 8 waves of a group), a slice accumulates its steps in ascending order on the MFMA pipe, and the slices are
//     added in ascending order starting from 0.0f.
// gemm_skinny_fused_kernel / gemm_skinny_prenorm_kernel (column owners; the library's automatic choice at M <= 64): a group of NS waves of
//   one workgroup owns its output columns for all of K, reduces through LDS and applies the epilogue; the prenorm form (M <= 16) also
//   RMS-normalises its input rows itself.
// A split-K form of the single-token passes' GEMMs - the NS slices of a column tile as NS workgroups, write-through fp32 slabs, a ticket per
//   tile, the last arriver adding the slabs in slice order (bit-identical to these kernels), rope + KV append in the q|k|v reducer - was built
//   and measured in round 6 and is NOT here: 4.94-5.24 ms per pass against 4.02 alone, 288 against 295 policy steps/s inside the step
//   (profiles/NEGATIVE.md, r06c_*). The reducer's tail (ticket round trip + slab read-back, 3-12 us per GEMM) costs more than the launch it saves.
//
// THE BIT CONTRACT. Every dequantised weight of the quantised formats is exactly a bf16 number, so their kernels must give the bits of the
// bf16 kernels run on the dequantised weights (tests/test_w8_gemm_gpu.py, tests/test_mx4_gemm_gpu.py). The decomposition into column tiles
// and K slices, the slice count, the LDS reduction order, the input RMSNorm, the epilogue and the launch rules exist once, here. A weight
// format (`Fmt`, the first template argument of both kernels, readable in a trace name) supplies:
//   Fmt::Q, Fmt::S                   element types of the two device pointers of a packed weight, rows and scales, which reach both kernels as
//                                    __restrict__ arguments (bf16: void, null pointers - its weights are p.W)
//   Fmt::main_fused / main_prenorm   the main loop: the ring of weight (and activation) loads of the wave's K steps w, w + NW, ... and the four
//                                    16x16x32 bf16 MFMAs per step, tile and row fragment, fragments s = 0 .. 3 in ascending order into acc[t][i]
//   Fmt::ROW_SCALE, Fmt::row_scale() a factor per weight row on the reduced fp32 sum, in front of the epilogue (fp8 only; a power of two: exact)
// Why the main loop is the format's and not shared: one loop with format hooks for the slot, its load and the fragment conversion was built
// and measured first. It was bit-identical and kept every decode-pass kernel's occupancy, but its instruction schedule cost the decode pass
// time beyond the parent's run-to-run spread, first of all fused <1, 1, 8, 1, 4> on fp8 (down projection, M = 7: 22.4 -> 24.5 us), also
// prenorm <2, 4, 2, 2> on fp8 (gate|up 39.7 -> 41.0) and fused <1, 1, 1, 4, 2> on fp8 and MXFP4 (lm_head 134.2 -> 137.0, 127.0 -> 129.4).
// Register allocation of these loops turns on small things: bf16 needs weight load s beside activation load s with one shared offset and
// predicate (anything else: lm_head kernel 76 -> 84 VGPRs, a wave of occupancy), the packed formats want their weight loads in front; skipping
// ring slots behind the wave's last K step (MXFP4 does, and saves the conversions; zeros leave every accumulator as it is, so it is the same
// bits) costs bf16 and fp8 a wave of occupancy on the lm_head kernel. So a loop changes in its own file, and the tests that compare the
// formats bit for bit, with the order fixed above, say whether it still computes the same sum.
#pragma once
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SK_BK = 128;   // K elements per step

// waves of a group that share one column tile's K steps: enough to put a few thousand waves in
// flight, never more than there are K steps. `tiles` = 16-column tiles (GLU: 32 interleaved gate | up rows of W)
inline int sk_group_waves(int tiles, int ksteps) {
    int nw = tiles >= 4096 ? 1 : tiles >= 2048 ? 2 : tiles >= 1024 ? 4 : 8;   // (16 waves on the K = 18944 down projection: no gain)
    while (nw > 1 && nw > ksteps) nw >>= 1;
    return nw;
}
// ... of the kernels with the fused input norm (every workgroup repeats the normalisation: at least 4 slices per tile)
inline int sk_group_waves_prenorm(int tiles, int ksteps) {
    const int nw = sk_group_waves(tiles, ksteps);
    return nw < 4 ? 4 : nw;
}

// RMSNorm of the <= 16 activation rows into an LDS image of bf16 MFMA operand rows (row stride lds_ld = K + 8 elements: the 16 fragment rows
// of a ds_read_b128 land on 16 different bank quads): wave `wave` of NWAVES takes rows wave, wave + NWAVES, ...; lane l the 8-element chunks
// l, l + 64, ... of the row. Per lane the squares are accumulated by fma in ascending chunk / element order, the 64 lane sums by the xor
// butterfly of wave_sum.
template <int NWAVES>
__device__ __forceinline__ void sk_prenorm_rows(const GemmArgs& p, bf16* img, int lds_ld, int wave, int lane) {
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
        for (int c = lane; c < nch; c += 64) {           // second read of the row: L1 / L2 hits, keeps the register budget small
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

// cross-wave reduction through LDS, red = [group][slice][NT16][MF][64 lanes x 4] fp32: the slices are added in ascending order from 0.0f
// (I = index type: int over the fused kernel's static array, size_t over the prenorm kernel's dynamic one, as the parents of both formed it)
template <class I, int MF, int NT16, int NW>
__device__ __forceinline__ void sk_reduce_put(float* red, int grp, int w, int lane, const f32x4 (&acc)[NT16][MF]) {
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
        for (int i = 0; i < MF; ++i) *reinterpret_cast<f32x4*>(&red[((((I)grp * NW + w) * NT16 + t) * MF + i) * 256 + lane * 4]) = acc[t][i];
}
template <class I, int MF, int NT16, int NW>
__device__ __forceinline__ void sk_reduce_get(const float* red, int grp, int i, int lane, const f32x4 (&acc)[NT16][MF], f32x4 (&sum)[NT16]) {
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
        if constexpr (NW > 1) {
            sum[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ww = 0; ww < NW; ++ww) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&red[((((I)grp * NW + ww) * NT16 + t) * MF + i) * 256 + lane * 4]);
#pragma unroll
                for (int r = 0; r < 4; ++r) sum[t][r] += v[r];
            }
        } else {
            sum[t] = acc[t][i];
        }
    }
}

// epilogue of one lane's 4 output columns n .. n + 3 of row m (m < M, n < N checked by the caller; n0 = first column of the group's tile):
// +bias -> act -> *colscale -> *rowscale -> +residual -> store, or GLU: act(gate + bias) * (up + bias) * rowscale
template <int NT16>
__device__ __forceinline__ void sk_epilogue(const GemmArgs& p, const f32x4 (&sum)[NT16], int m, int n, int n0, int g) {
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

// the format's row scale (tile t of the group holds weight rows n + t * 16 + r) on the reduced sums, then the epilogue
template <class Fmt, int NT16>
__device__ __forceinline__ void sk_scale_store(const GemmArgs& p, const typename Fmt::S* __restrict__ ws, f32x4 (&sum)[NT16], int m, int n, int n0, int g) {
    if constexpr (Fmt::ROW_SCALE) {
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[t][r] *= Fmt::row_scale(ws, n + t * 16 + r);
    }
    sk_epilogue<NT16>(p, sum, m, n, n0, g);
}

// ---- column-owner kernel: a group of NW waves owns NT16 x 16 output columns for ALL of K (a workgroup holds NC such groups); the
// group's waves take interleaved 128-wide K steps, keep a DEPTH-deep register ring of loads in flight (the format's main loop), reduce their
// accumulators through LDS (NW > 1) and apply the epilogue in the same kernel: no partial workspace, no second launch (a decode pass of the
// 28-layer LLM is 4 such GEMMs per layer: the separate epilogue launches were ~0.8 ms of every pass). NW is chosen per shape so
// the launch has a few thousand waves: 1 for the 152064-row lm_head (long-lived independent waves), 8 for a 3584-row projection.
template <class Fmt, int MF, int NT16, int NW, int NC, int DEPTH>
__global__ __launch_bounds__(NW * NC * 64) void gemm_skinny_fused_kernel(GemmArgs p, const typename Fmt::Q* __restrict__ wq, const typename Fmt::S* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float red[(NW > 1 ? NC * NW : 1) * NT16 * MF * 64 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = wave / NW, w = wave % NW;
    const int n0 = (blockIdx.x * NC + grp) * (16 * NT16);
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc[NT16][MF];
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
        for (int i = 0; i < MF; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = (p.K + SK_BK - 1) / SK_BK;
    const int nmine = w < ksteps ? (ksteps - w + NW - 1) / NW : 0;   // K steps w, w + NW, ...
    Fmt::template main_fused<MF, NT16, NW, DEPTH>(p, wq, ws, n0, w, nmine, r16, g, acc);
    // ---- cross-wave reduction (NW > 1) + epilogue: wave w of a group owns row fragments w, w + NW, ... of every column tile
    if constexpr (NW > 1) {
        sk_reduce_put<int, MF, NT16, NW>(red, grp, w, lane, acc);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        if (NW > 1 && (i % NW) != w) continue;
        const int m = i * 16 + r16, n = n0 + g * 4;
        f32x4 sum[NT16];
        sk_reduce_get<int, MF, NT16, NW>(red, grp, i, lane, acc, sum);
        if (m >= p.M || n >= p.N) continue;
        sk_scale_store<Fmt, NT16>(p, ws, sum, m, n, n0, g);
    }
}

// ---- column-owner kernel with the INPUT RMSNorm fused in front (M <= 16: the single-token decode passes of the LLM, where a separate
// norm launch over 7 x 3584 values costs as much as a 30 MB projection). Every workgroup first requests its weight ring, then - while
// those loads are in flight - normalises the <= 16 activation rows itself: one wave per row reads the row (f32 residual stream or bf16
// embeddings, L2 hits: every workgroup reads the same <= 230 KB), reduces the sum of squares and writes bf16(x * rstd * gamma) into an
// LDS image whose rows sit 16 bytes past a multiple of 256 (the 16 fragment rows of a ds_read_b128 land on 16 different bank quads).
// The format's main loop is its fused one with the activation fragments read from that image instead of global memory; it calls `norm`
// once, between filling its ring and its first MFMA.
template <class Fmt, int NT16, int NW, int NC, int DEPTH>
__global__ __launch_bounds__(NW * NC * 64) void gemm_skinny_prenorm_kernel(GemmArgs p, const typename Fmt::Q* __restrict__ wq, const typename Fmt::S* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    constexpr int NWAVES = NW * NC;
    const int lds_ld = p.K + 8;
    bf16* img = reinterpret_cast<bf16*>(sk_smem);                                                     // [M][K + 8]
    float* red = reinterpret_cast<float*>(sk_smem + (((size_t)p.M * lds_ld * sizeof(bf16) + 15) & ~size_t(15)));   // [NC][NW][NT16][256]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wave / NW, w = wave % NW;
    const int n0 = (blockIdx.x * NC + grp) * (16 * NT16);
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc[NT16][1];
#pragma unroll
    for (int t = 0; t < NT16; ++t) acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = (p.K + SK_BK - 1) / SK_BK;
    const int nmine = w < ksteps ? (ksteps - w + NW - 1) / NW : 0;
    Fmt::template main_prenorm<NT16, NW, DEPTH>(p, wq, ws, img, lds_ld, n0, w, nmine, r16, g, acc, [&]() {
        sk_prenorm_rows<NWAVES>(p, img, lds_ld, wave, lane);   // (the weight ring is in flight meanwhile)
        __syncthreads();
    });
    if constexpr (NW > 1) {
        sk_reduce_put<size_t, 1, NT16, NW>(red, grp, w, lane, acc);
        __syncthreads();
        if (w != 0) return;        // one 16-row fragment: wave 0 of the group reduces and stores
    }
    const int m = r16, n = n0 + g * 4;
    f32x4 sum[NT16];
    sk_reduce_get<size_t, 1, NT16, NW>(red, grp, 0, lane, acc, sum);
    if (m >= p.M || n >= p.N) return;
    sk_scale_store<Fmt, NT16>(p, ws, sum, m, n, n0, g);
}

// ---- launch ladders (host). The <NW, NC, DEPTH> table is one table for every format: the group width decides the summation order.
template <class Fmt, int MF, int NT16>
void sk_launch_fused_tile(const GemmArgs& p, const typename Fmt::Q* wq, const typename Fmt::S* ws, hipStream_t stream) {
    const int ksteps = (p.K + SK_BK - 1) / SK_BK;
    const int tiles = (p.N + 16 * NT16 - 1) / (16 * NT16);
    // waves per column group: enough to put >= ~4096 waves in flight (16 per CU), never more than there are K steps
    const int nw = sk_group_waves(tiles, ksteps);
    // ring depth. Round 3 measured and dropped: twice the register ring for the single-fragment shapes, and 4-wave column groups everywhere -
    // neutral alone, -10 % inside the step where the chain shares the CUs with System-1 (profiles/r03e / r03g_bench_*_experiments.log).
    // The quantised formats keep the bf16 depths. Measured for MXFP4 at M = 7 on the four layer shapes of the 7B geometry, these depths /
    // twice them where the registers allow / four times them in the prenorm form: q|k|v 12.2 / 12.2 / 12.0 us, o 9.8 / 10.6 / 9.8 (one
    // process each; fp8 moved alike), gate|up 30.9 / 31.2 / 39.2, down 20.3 / 20.4 / 20.5 - fewer bytes per slot do not ask for more slots
    constexpr int DEEP = (MF <= 2 && NT16 == 1) ? 4 : 2;
#define INA_SKF(NW_, NC_, D_) \
    hipLaunchKernelGGL((gemm_skinny_fused_kernel<Fmt, MF, NT16, NW_, NC_, D_>), dim3((tiles + NC_ - 1) / NC_), dim3(NW_ * NC_ * 64), 0, stream, p, wq, ws)
    if (nw == 1) INA_SKF(1, 4, 2);
    else if (nw == 2) INA_SKF(2, 2, 2);
    else if (nw == 4) INA_SKF(4, 1, 2);
    else INA_SKF(8, 1, DEEP);
#undef INA_SKF
}

template <class Fmt, int NT16>
int sk_launch_fused_glu(const GemmArgs& p, const typename Fmt::Q* wq, const typename Fmt::S* ws, hipStream_t stream) {
    switch ((p.M + 15) / 16) {
        case 1: sk_launch_fused_tile<Fmt, 1, NT16>(p, wq, ws, stream); break;
        case 2: sk_launch_fused_tile<Fmt, 2, NT16>(p, wq, ws, stream); break;
        case 3: sk_launch_fused_tile<Fmt, 3, NT16>(p, wq, ws, stream); break;
        default: sk_launch_fused_tile<Fmt, 4, NT16>(p, wq, ws, stream); break;
    }
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
template <class Fmt>
int sk_launch_fused(const GemmArgs& p, const typename Fmt::Q* wq, const typename Fmt::S* ws, hipStream_t stream) {
    return p.glu ? sk_launch_fused_glu<Fmt, 2>(p, wq, ws, stream) : sk_launch_fused_glu<Fmt, 1>(p, wq, ws, stream);
}

template <class Fmt, int NT16, int NW, int NC, int DEPTH>
int sk_launch_prenorm_cfg(const GemmArgs& p, const typename Fmt::Q* wq, const typename Fmt::S* ws, hipStream_t stream, int tiles) {
    const size_t lds = (((size_t)p.M * (p.K + 8) * sizeof(bf16) + 15) & ~size_t(15)) + (NW > 1 ? size_t(NC) * NW * NT16 * 256 * sizeof(float) : 0);
    auto kern = gemm_skinny_prenorm_kernel<Fmt, NT16, NW, NC, DEPTH>;
    static size_t attr = 0;   // (per instantiation) the largest dynamic LDS size this kernel has been allowed so far
    if (lds > attr) {
        INA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = lds;
    }
    hipLaunchKernelGGL(kern, dim3((tiles + NC - 1) / NC), dim3(NW * NC * 64), lds, stream, p, wq, ws);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
// every workgroup repeats the (cheap, L2-served) normalisation, so the column groups are packed NC per workgroup where one group
// alone would be a 4-wave workgroup; the group width follows the fused kernel's rule (a few thousand waves per launch)
template <class Fmt>
int sk_launch_prenorm(const GemmArgs& p, const typename Fmt::Q* wq, const typename Fmt::S* ws, hipStream_t stream) {
    const int ksteps = (p.K + SK_BK - 1) / SK_BK;
    if (p.glu) {
        const int tiles = (p.N + 31) / 32;
        if (sk_group_waves_prenorm(tiles, ksteps) == 4) return sk_launch_prenorm_cfg<Fmt, 2, 4, 2, 2>(p, wq, ws, stream, tiles);
        return sk_launch_prenorm_cfg<Fmt, 2, 8, 1, 2>(p, wq, ws, stream, tiles);
    }
    const int tiles = (p.N + 15) / 16;
    if (sk_group_waves_prenorm(tiles, ksteps) == 4) return sk_launch_prenorm_cfg<Fmt, 1, 4, 2, 2>(p, wq, ws, stream, tiles);
    return sk_launch_prenorm_cfg<Fmt, 1, 8, 1, 4>(p, wq, ws, stream, tiles);
}

// algorithmic bytes of one launch for the profiler: activations (f32 rows only in front of the fused norm) + the format's weight bytes + out
inline double sk_prof_bytes(const GemmArgs& p, double weight_bytes) {
    const double osz = p.out_dtype == INA_DT_BF16 ? 2.0 : 4.0, asz = (p.norm_gamma && p.a_dtype == INA_DT_F32) ? 4.0 : 2.0;
    return asz * p.M * p.K + weight_bytes + osz * p.M * (p.glu ? p.N / 2 : p.N);
}

// Validation shared by the entries of the packed formats (ina_gemm_w8, ina_gemm_mx4): host arithmetic only, before any HIP call (testable
// without a GPU). `p` receives the defaults. `tag` prefixes every refusal ("gemm_w8"), `what` names the format in two of them ("fp8");
// `layout(p)` holds the format's own checks on the packed rows (pitch, scale alignment) and runs where they have always run.
template <class LayoutChecks>
int sk_plan_packed(const GemmArgs& p_in, GemmArgs& p, const char* tag, const char* what, LayoutChecks layout) {
    p = p_in;
    if (p.rowscale_div <= 0) p.rowscale_div = 1;
    if (p.batch <= 0) p.batch = 1;
    INA_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "%s: empty problem M=%d N=%d K=%d", tag, p.M, p.N, p.K);
    INA_REQUIRE(p.M <= 64, "%s: the %s-weight kernels are weight-streaming kernels for M <= 64 rows (M=%d)", tag, what, p.M);
    INA_REQUIRE(p.K % 128 == 0, "%s: the packed %s layout needs K %% 128 == 0 (K=%d)", tag, what, p.K);
    INA_REQUIRE(p.batch == 1, "%s: no batched form (batch=%d)", tag, p.batch);
    INA_REQUIRE(!p.seg_stats, "%s: seg_stats exist in the row-panel kernels only", tag);
    INA_REQUIRE(!p.Wp, "%s: Wp (fragment-ordered bf16 weights) has no meaning here", tag);
    INA_REQUIRE(p.force_cfg == 0 || p.force_cfg == -1, "%s: no tile configs to force (force_cfg %d)", tag, p.force_cfg);
    if (int rc = layout(p)) return rc;
    INA_REQUIRE(p.lda % 8 == 0, "%s: lda must be a multiple of 8 (lda=%d)", tag, p.lda);
    INA_REQUIRE(p.N % 4 == 0 && p.ldc % 4 == 0, "%s: N/ldc must be multiples of 4 (N=%d ldc=%d)", tag, p.N, p.ldc);
    INA_REQUIRE(((uintptr_t)p.A % 16) == 0 && ((uintptr_t)p.C % 8) == 0, "%s: misaligned pointer", tag);
    INA_REQUIRE(!p.R || p.ldr % 4 == 0, "%s: ldr must be a multiple of 4", tag);
    INA_REQUIRE(!p.glu || (p.N % 32 == 0), "%s: GLU mode needs N %% 32 == 0", tag);
    INA_REQUIRE(p.act >= INA_ACT_NONE && p.act <= INA_ACT_TANH, "%s: act=%d is not an activation code (0 .. %d)", tag, p.act, (int)INA_ACT_TANH);
    INA_REQUIRE(!p.glu || !p.R, "%s: glu cannot be combined with a residual (R)", tag);
    INA_REQUIRE(!p.glu || !p.colscale, "%s: glu cannot be combined with colscale", tag);
    if (p.norm_gamma) {
        INA_REQUIRE(p.M <= 16 && p.K <= 4096 && p.N >= 256,
                    "%s: the fused input RMSNorm is built for the decode passes (M <= 16 rows, K <= 4096): M=%d K=%d N=%d", tag, p.M, p.K, p.N);
        INA_REQUIRE(p.a_dtype == INA_DT_BF16 || p.a_dtype == INA_DT_F32, "%s: a_dtype must be bf16 or f32 with norm_gamma", tag);
        INA_REQUIRE(((uintptr_t)p.norm_gamma % 16) == 0 && (p.lda % (p.a_dtype == INA_DT_F32 ? 4 : 8)) == 0, "%s(prenorm): misaligned gamma / lda", tag);
    }
    return 0;
}

}  // namespace
