// The 64-key chunk step of the single-token attention family for gfx950, defined once: attn_decode_split_kernel, attn_decode_fused_kernel and
// attn_decode_fused8_kernel (attention.hip), attn_prefix_kernel and its twin with a tail segment, attn_prefix_tail_kernel (one body,
// attention_prefix.hip), and attn_shared_kernel (attention_shared.hip).
//
// All of them put 16 packed query rows in one MFMA tile and cut their key axis into chunks of AC_KVB = 64 keys. Both MFMAs are issued in the
// "swapped" form of attention.hip: lane l owns query row lq = l & 15, lane group g = l >> 4 owns the keys t * 16 + g * 4 + r of a chunk:
//   S^T[kv][q] = K . Q^T    -> lane holds S[q][kv0 + t * 16 + g * 4 + r] in s[t][r]
//   O^T[d][q]  = V^T . P^T  -> lane holds O[q][nt * 16 + g * 4 + r] in acc_o[nt][r]
// so the probabilities a lane computed are its own P V operand once V^T lies in LDS in the key order vt_pos. A wave keeps a running
// (max m_run, sum l_run, un-normalised O) over the chunks it walks, in the exp2 domain; the waves' partials meet in LDS and are added in wave
// order. What is NOT here is each kernel's own: which chunks a wave walks and where their K / V come from, when the next chunk is requested,
// the prologue, and the write of the output rows. The pieces are plain inlined functions on the caller's register arrays: nothing is kept
// between calls.
#pragma once
#include "common.h"

namespace {

constexpr int AC_KVB = 64;              // keys per chunk
constexpr int AC_VT_LD = AC_KVB + 8;    // row pitch of a V^T image (bf16)
constexpr int AC_NST = AC_KVB / 16;     // 16-key score tiles per chunk
constexpr int AC_NSB = AC_KVB / 32;     // 32-key sub-blocks per chunk: one P fragment each

// V^T LDS image: row d holds the block's keys in the slot order vt_pos(key), with its 8-slot groups ROTATED by d >> 3 (mod KVB/8).
// The transposing 2-byte stores of one wave instruction go to rows d = c*8 + i for 8-16 different chunks c: without the rotation
// all of them fall on the same bank (row stride x 8 = 0 mod 32 dwords), a 16-way conflict on every store.
__device__ __forceinline__ int vt_pos(int kv_local) {
    // key permutation inside each 32-key sub-block: MFMA k index g*8 + j  <->  key (j<4 ? g*4+j : 16+g*4+(j-4))
    int sub = kv_local >> 5, w = kv_local & 31;
    int t = w >> 4, x = w & 15;
    return (sub << 5) + ((x >> 2) << 3) + (x & 3) + (t << 2);
}

// a wave's LDS accesses so far have completed (its LDS queue is in order) before it overwrites or reads an image of its own
__device__ __forceinline__ void ac_wave_lds_fence() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// ---- fetches: keys kv0 .. kv0 + 63 of a source of `len` keys at `base` (row stride rs elements), one wave
// row-major pieces of a W-wide block (W = DP for a K image, DV for V): piece q = lane + u * 64 is 16 bytes of row q / (W / 8); zeros behind
// len and, for K, behind the head dim D
template <int W, bool GUARD_D>
__device__ __forceinline__ void ac_fetch_rows(const bf16* __restrict__ base, long rs, int kv0, int len, int D, int lane, bf16x8 (&reg)[AC_KVB * (W / 8) / 64]) {
    constexpr int CPR = W / 8;
    static_assert((AC_KVB * CPR) % 64 == 0, "chunk pieces must divide evenly over the wave");
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < AC_KVB * CPR / 64; ++u) {
        const int q = lane + u * 64, row = q / CPR, c = q % CPR, kv = kv0 + row;
        reg[u] = (kv < len && (!GUARD_D || c * 8 < D)) ? *reinterpret_cast<const bf16x8*>(base + (size_t)kv * rs + c * 8) : zero8;
    }
}
template <int DV>
__device__ __forceinline__ void ac_fetch_v(const bf16* __restrict__ V, long rs, int kv0, int len, int lane, bf16x8 (&vreg)[AC_KVB * (DV / 8) / 64]) {
    ac_fetch_rows<DV, false>(V, rs, kv0, len, 0, lane, vreg);
}
// K straight into MFMA operand layout: lane -> key row t * 16 + lq, 16 bytes of its 32-wide k slice (64 contiguous bytes per row and instruction).
// Keys beyond len read row len - 1: a valid row, their scores are masked. GUARD_D: zeros behind the head dim D (d = 128 sources need none)
template <int NKK, bool GUARD_D>
__device__ __forceinline__ void ac_fetch_kf(const bf16* __restrict__ K, long rs, int kv0, int len, int D, int lq, int g, bf16x8 (&kf)[AC_NST][NKK]) {
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < AC_NST; ++t) {
        const int kv = kv0 + t * 16 + lq;
        const bf16* kr = K + (size_t)(kv < len ? kv : len - 1) * rs + g * 8;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) kf[t][kk] = (!GUARD_D || kk * 32 + g * 8 < D) ? *reinterpret_cast<const bf16x8*>(kr + kk * 32) : zero8;
    }
}

// ---- LDS images of a chunk
// row-major K image (pitch DP + 8) from the pieces of ac_fetch_rows<DP>
template <int DP>
__device__ __forceinline__ void ac_store_k_image(bf16* Ks, int lane, const bf16x8 (&kreg)[AC_KVB * (DP / 8) / 64]) {
    constexpr int CPR = DP / 8;
#pragma unroll
    for (int u = 0; u < AC_KVB * CPR / 64; ++u) {
        const int q = lane + u * 64, row = q / CPR, c = q % CPR;
        *reinterpret_cast<bf16x8*>(&Ks[row * (DP + 8) + c * 8]) = kreg[u];
    }
}
// transposed, permuted and rotated V^T image (see vt_pos) from the pieces of ac_fetch_v<DV>. (attn_decode_fused8_kernel writes two half images
// with a store loop of its own: through this function, with the first head dim of the image as an argument, it spills 60 - 116 VGPRs.)
template <int DV>
__device__ __forceinline__ void ac_store_vt_image(bf16* Vt, int lane, const bf16x8 (&vreg)[AC_KVB * (DV / 8) / 64]) {
    constexpr int CPR = DV / 8;
#pragma unroll
    for (int u = 0; u < AC_KVB * CPR / 64; ++u) {
        const int q = lane + u * 64, row = q / CPR, c = q % CPR;
        const int pos = vt_pos(row);
#pragma unroll
        for (int i = 0; i < 8; ++i) Vt[(c * 8 + i) * AC_VT_LD + ((pos + 8 * c) & (AC_KVB - 1))] = vreg[u][i];
    }
}

// ---- S^T = K Q^T, K from the register fragments of ac_fetch_kf or from a K image
template <int NKK>
__device__ __forceinline__ void ac_scores(const bf16x8 (&kf)[AC_NST][NKK], const bf16x8 (&qf)[NKK], f32x4 (&s)[AC_NST]) {
#pragma unroll
    for (int t = 0; t < AC_NST; ++t) {
        s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][kk], qf[kk], s[t], 0, 0, 0);
    }
}
template <int NKK>
__device__ __forceinline__ void ac_scores_image(const bf16* Ks, int lq, int g, const bf16x8 (&qf)[NKK], f32x4 (&s)[AC_NST]) {
    constexpr int KS_LD = NKK * 32 + 8;
#pragma unroll
    for (int t = 0; t < AC_NST; ++t) {
        s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(t * 16 + lq) * KS_LD + kk * 32 + g * 8]);
            s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s[t], 0, 0, 0);
        }
    }
}

// ---- mask + online softmax of one chunk: the lane's scores s[t][r] of keys kv = kv0 + t * 16 + g * 4 + r become exp2(s * sc - max) where
// ok(kv), else 0; (m_run, l_run) move on. Returns alpha, the factor the running O takes (ac_scale_o) before this chunk's P V is added.
// A first chunk scales by 0: exp2 never sees -inf - -inf. UNIT_ALPHA: an unchanged maximum scales by exactly 1, so that a chunk that is masked
// for a row leaves the row's (m_run, l_run, O) bit for bit as they were even when it is the row's first - the promise of attn_shared_kernel.
template <bool UNIT_ALPHA = false, class Mask>
__device__ __forceinline__ float ac_softmax_update(f32x4 (&s)[AC_NST], int kv0, int g, float sc, Mask ok, float& m_run, float& l_run) {
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < AC_NST; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kv = kv0 + t * 16 + g * 4 + r;
            const float v = ok(kv) ? s[t][r] * sc : -INFINITY;
            s[t][r] = v;
            mx = fmaxf(mx, v);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = (UNIT_ALPHA && m_new == m_run) ? 1.f : (m_run == -INFINITY) ? 0.f : exp2f(m_run - m_use);
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < AC_NST; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = exp2f(s[t][r] - m_use);
            s[t][r] = e;
            rs += e;
        }
    rs += __shfl_xor(rs, 16);
    rs += __shfl_xor(rs, 32);
    l_run = l_run * alpha + rs;
    m_run = m_new;
    return alpha;
}
template <int NDT>
__device__ __forceinline__ void ac_scale_o(f32x4 (&acc_o)[NDT], float alpha) {
#pragma unroll
    for (int nt = 0; nt < NDT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc_o[nt][r] *= alpha;
}
// the lane's 8 probabilities of 32-key sub-block sb are its P V operand (key order vt_pos)
__device__ __forceinline__ void ac_pack_p(const f32x4 (&s)[AC_NST], bf16x8 (&pf)[AC_NSB]) {
#pragma unroll
    for (int sb = 0; sb < AC_NSB; ++sb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pf[sb][r] = (bf16)s[2 * sb][r];
            pf[sb][4 + r] = (bf16)s[2 * sb + 1][r];
        }
}
// ---- O^T += V^T P^T for the N 16-dim tiles nt0 .. nt0 + N - 1 of acc_o, against an image whose row 0 is head dim nt0 * 16
template <int N, int NDT>
__device__ __forceinline__ void ac_pv(const bf16* Vt, int lq, int g, const bf16x8 (&pf)[AC_NSB], f32x4 (&acc_o)[NDT], int nt0 = 0) {
#pragma unroll
    for (int sb = 0; sb < AC_NSB; ++sb)
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const int dl = n * 16 + lq, d = nt0 * 16 + dl;               // row of the image / head dim
            const bf16x8 vf = *reinterpret_cast<const bf16x8*>(&Vt[dl * AC_VT_LD + ((sb * 32 + g * 8 + 8 * (d >> 3)) & (AC_KVB - 1))]);
            acc_o[nt0 + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[sb], acc_o[nt0 + n], 0, 0, 0);
        }
}

// ---- a wave's partial, pitch PLD floats: row lq -> [DV] un-normalised O (exp2 domain), then m, l
template <int PLD, int NDT>
__device__ __forceinline__ void ac_store_partial(float* part, int lq, int g, const f32x4 (&acc_o)[NDT], float m_run, float l_run) {
    float* orow = part + (size_t)lq * PLD;
#pragma unroll
    for (int nt = 0; nt < NDT; ++nt) *reinterpret_cast<f32x4*>(orow + nt * 16 + g * 4) = acc_o[nt];
    if (g == 0) { orow[NDT * 16] = m_run; orow[NDT * 16 + 1] = l_run; }
}
// the NW partials of row `row` (wave w's at smem + w * PER_WAVE bf16 elements), added in wave order: o = the normalised columns c0 .. c0 + DV / 16 - 1
// (a row without an allowed key: l = 0 -> zeros)
template <int NW, int PER_WAVE, int PLD, int DV>
__device__ __forceinline__ void ac_combine(const char* smem, int row, int c0, float (&o)[DV / 16]) {
    constexpr int CPT = DV / 16;
    const float* pw[NW];
    float ms[NW], m = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        pw[w] = reinterpret_cast<const float*>(reinterpret_cast<const bf16*>(smem) + w * PER_WAVE) + row * PLD;
        ms[w] = pw[w][DV];
        m = fmaxf(m, ms[w]);
    }
    const float m_use = (m == -INFINITY) ? 0.f : m;
    float l = 0.f;
#pragma unroll
    for (int c = 0; c < CPT; ++c) o[c] = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const float wl = (ms[w] == -INFINITY) ? 0.f : exp2f(ms[w] - m_use);
        l += pw[w][DV + 1] * wl;
#pragma unroll
        for (int c = 0; c < CPT; ++c) o[c] += pw[w][c0 + c] * wl;
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int c = 0; c < CPT; ++c) o[c] *= inv;
}

// ---- launch of a kernel whose dynamic LDS exceeds the default limit: the limit is raised once per kernel
template <auto KERN, class... Args>
int ac_launch_big_lds(dim3 grid, int threads, size_t lds, hipStream_t stream, Args... args) {
    static bool attr_done = false;
    if (!attr_done) {
        INA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done = true;
    }
    hipLaunchKernelGGL(KERN, grid, dim3(threads), lds, stream, args...);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace
