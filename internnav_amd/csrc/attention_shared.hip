// Shared-prompt decode attention for gfx950 (bf16 in/out, fp32 softmax + accumulation, d = 128): single-token attention for R rows, one returned
// sequence per row (generate(do_sample=True, num_return_sequences=K, share_prefix=True): the prompt is prefilled once into its cache slot and the
// K sampled answers of a prompt keep their own K/V in a small per-layer TAIL buffer - no cache slot per returned sequence, no copy of the prompt).
//
//   row r sees  keys 0 .. pfx_len - 1 of cache slot `slot` of its tile   (its prompt, read in place and shared with the other rows of that prompt)
//          and  the first tail_len[r] rows of ITS OWN tail               (the K/V of its own answer tokens, the current one included)
//
// nothing of another row's tail, no cache row at or behind pfx_len. Nothing is written to the cache.
//
// Structure: attn_prefix_kernel (attention_prefix.hip) with the rows of a 16-row MFMA tile taken from cpt = 16 / G candidates of the SAME prompt
// (G = H / Hkv query heads per KV head): packed row R -> (place R / G of the tile, head kh * G + R % G); the host names the row of every place in
// an int32 [n_tiles, cpt] table (-1 = empty place). One four-wave workgroup per (tile, KV head), so the prompt's 64-key prefix chunks are read
// once per tile and KV head, not once per candidate (an expectation: no counter was read). The key axis: prefix chunks 0 .. nc - 1, then per
// place j the 64-key chunks of that candidate's tail; a tail chunk of place j is masked for the rows of the other places.
// Bits do not depend on neighbours: the wave that owns a chunk is a function of the row's OWN chunk index (prefix chunk c -> wave c mod 4, tail
// chunk t of any place -> wave (nc + t) mod 4), a wave walks its chunks in (prefix, place 0, place 1, ...) order, and a chunk that is masked
// for a row leaves that row's running (max, sum, O) exactly as it was (alpha = 1 by construction - never exp2(-inf - -inf) -, e = 0, O += 0).
// So every wave sees, per row, the row's own chunks in the row's own order whatever else shares the tile. The four partials meet in LDS in wave
// order and the workgroup writes the normalised rows itself: no atomics, no workspace, the same bits on every launch.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int SHR_WAVES = 4, SHR_CHUNK = 64, SHR_D = 128;

// key permutation of the V^T image (attention.hip, vt_pos)
__device__ __forceinline__ int shr_vt_pos(int kv_local) {
    int sub = kv_local >> 5, w = kv_local & 31;
    int t = w >> 4, x = w & 15;
    return (sub << 5) + ((x >> 2) << 3) + (x & 3) + (t << 2);
}

struct SharedArgs {
    const bf16* Q; bf16* O;
    const bf16 *Kc, *Vc, *Kt, *Vt;
    const int32_t *tile_rows, *tile_slot, *tile_pfx, *tail_len;
    long q_rs, q_hs, o_rs, o_hs, c_ss, c_rs, c_hs, t_ps, t_rs, t_hs;
    int n_tiles, n_rows, T, H, Hkv, G, cpt, n_slots, max_pfx;
    float scale;
};

__global__ __launch_bounds__(SHR_WAVES * 64) void attn_shared_kernel(SharedArgs a) {
    constexpr int D = SHR_D, KVB = SHR_CHUNK, VT_LD = KVB + 8, VCPR = D / 8, NKK = D / 32, NST = KVB / 16, NSB = KVB / 32, NDT = D / 16;
    constexpr int PER_WAVE = D * VT_LD;                       // bf16 elements of one wave's V^T image
    constexpr int PLD = D + 4;                                // partial row: D x O, m, l (f32), padded to a 16-byte pitch
    constexpr int CPT = D / 16;                               // output columns per thread in the combine
    static_assert(16 * PLD * 4 <= PER_WAVE * 2, "the partial of a wave fits its V^T image");
    extern __shared__ __attribute__((aligned(16))) char shr_smem[];
    __shared__ int s_row[16], s_tl[16];                       // per place of the tile: its row (-1: empty) and its clipped tail length
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, lq = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    bf16* Vt = reinterpret_cast<bf16*>(shr_smem) + wave * PER_WAVE;
    const int tile = blockIdx.x, kh = blockIdx.y;
    const int G = a.G, cpt = a.cpt;
    const int sl = a.tile_slot[tile];
    const int pfx = min(max(a.tile_pfx[tile], 0), a.max_pfx);
    const bool bad_slot = sl < 0 || sl >= a.n_slots;
    if (tid < 16) {
        int r = -1, tl = 0;
        if (tid < cpt) {
            r = a.tile_rows[(size_t)tile * cpt + tid];
            if (r < 0 || r >= a.n_rows) r = -1;               // an empty place (or a row outside the buffers: never an access)
            else tl = min(max(a.tail_len[r], 0), a.T);
        }
        s_row[tid] = r;
        s_tl[tid] = tl;
    }
    __syncthreads();

    if (bad_slot) {
        // a slot outside the cache: NaN in the tile's live rows (the library's convention), zeros in its rows without a tail, never an access
        const int row = tid >> 4, c0 = (tid & 15) * CPT;
        const int pl = row / G;
        if (pl < cpt && s_row[pl] >= 0) {
            const bf16 fill = (bf16)(s_tl[pl] > 0 ? NAN : 0.f);
            const bf16x4 f4 = {fill, fill, fill, fill};
            bf16* op = a.O + (size_t)s_row[pl] * a.o_rs + (size_t)(kh * G + row % G) * a.o_hs + c0;
            *reinterpret_cast<bf16x4*>(op) = f4;
            *reinterpret_cast<bf16x4*>(op + 4) = f4;
        }
        return;
    }

    const int place = lq / G;                                  // packed row lq of this lane: place of the tile, head of the KV group
    const int my_row = place < cpt ? s_row[place] : -1;
    const bool active = my_row >= 0 && s_tl[place < cpt ? place : 0] > 0;      // rows without a tail attend nothing: zeros
    const int head = kh * G + lq % G;
    const bf16* __restrict__ Q = a.Q + (size_t)(active ? my_row : 0) * a.q_rs + (size_t)head * a.q_hs;
    const bf16* __restrict__ Kc = a.Kc + (size_t)sl * a.c_ss + (size_t)kh * a.c_hs;
    const bf16* __restrict__ Vc = a.Vc + (size_t)sl * a.c_ss + (size_t)kh * a.c_hs;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc_o[NDT];
#pragma unroll
    for (int i = 0; i < NDT; ++i) acc_o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 qf[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = active ? *reinterpret_cast<const bf16x8*>(Q + kk * 32 + g * 8) : zero8;

    const int nc = (pfx + KVB - 1) / KVB;                      // prefix chunks
    const int t0 = (wave - nc % SHR_WAVES + SHR_WAVES) % SHR_WAVES;            // first tail chunk of this wave: (nc + t) mod 4 == wave
    // this wave's chunks in order: (j, c) = prefix chunk c (j = -1), then tail chunk c of place j = 0 .. cpt - 1; j == cpt: done. Wave uniform.
    auto advance = [&](int& j, int& c) {
        c += SHR_WAVES;
        while (j < cpt) {
            const int n = j < 0 ? nc : (s_tl[j] + KVB - 1) / KVB;
            if (c < n) return;
            ++j;
            c = t0;
        }
    };
    constexpr int NVI = KVB * VCPR / 64;
    static_assert((KVB * VCPR) % 64 == 0, "chunk pieces must divide evenly over the wave");
    bf16x8 kf[NST][NKK], vreg[NVI];
    auto fetch = [&](int j, int c) {
        const bool tail = j >= 0;
        const size_t toff = tail ? (size_t)s_row[j] * a.t_ps + (size_t)kh * a.t_hs : 0;
        const bf16* Kb = tail ? a.Kt + toff : Kc;
        const bf16* Vb = tail ? a.Vt + toff : Vc;
        const long rs = tail ? a.t_rs : a.c_rs;
        const int kv0 = c * KVB, len = tail ? s_tl[j] : pfx;
#pragma unroll
        for (int t = 0; t < NST; ++t) {
            const int kv = kv0 + t * 16 + lq;
            const bf16* kr = Kb + (size_t)(kv < len ? kv : len - 1) * rs + g * 8;      // (keys beyond len: a valid row, their scores are masked)
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) kf[t][kk] = *reinterpret_cast<const bf16x8*>(kr + kk * 32);
        }
#pragma unroll
        for (int u = 0; u < NVI; ++u) {
            const int q = lane + u * 64, row = q / VCPR, cc = q % VCPR, kv = kv0 + row;
            vreg[u] = (kv < len) ? *reinterpret_cast<const bf16x8*>(Vb + (size_t)kv * rs + cc * 8) : zero8;
        }
    };
    const float sc = a.scale * 1.4426950408889634f;            // exp2 domain
    int j = -1, c = wave - SHR_WAVES;
    advance(j, c);
    if (j < cpt) fetch(j, c);
    while (j < cpt) {
        const int kv0 = c * KVB, len = j < 0 ? pfx : s_tl[j];
        const bool mine = active && (j < 0 || j == place);     // a tail chunk of another place: masked for this row
        // ---- S^T = K Q^T from the register fragments
        f32x4 s[NST];
#pragma unroll
        for (int t = 0; t < NST; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][kk], qf[kk], s[t], 0, 0, 0);
        }
        // ---- V registers -> this wave's transposed image
#pragma unroll
        for (int u = 0; u < NVI; ++u) {
            const int q = lane + u * 64, row = q / VCPR, cc = q % VCPR;
            const int pos = shr_vt_pos(row);
#pragma unroll
            for (int i = 0; i < 8; ++i) Vt[(cc * 8 + i) * VT_LD + ((pos + 8 * cc) & (KVB - 1))] = vreg[u][i];   // rotated rows: see vt_pos
        }
        int jn = j, cn = c;
        advance(jn, cn);
        if (jn < cpt) fetch(jn, cn);                           // next chunk in flight under this one's math
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // ---- mask + online softmax (lane owns packed row lq, keys kv0 + t*16 + g*4 + r)
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NST; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kv = kv0 + t * 16 + g * 4 + r;
                const float v = (mine && kv < len) ? s[t][r] * sc : -INFINITY;
                s[t][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
        // an unchanged maximum (every masked chunk) scales by exactly 1, a first chunk by 0: exp2 never sees -inf - -inf
        const float alpha = (m_new == m_run) ? 1.f : (m_run == -INFINITY) ? 0.f : exp2f(m_run - m_use);
        float rs = 0.f;
#pragma unroll
        for (int t = 0; t < NST; ++t)
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
#pragma unroll
        for (int nt = 0; nt < NDT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc_o[nt][r] *= alpha;
        // ---- O^T += V^T P^T
#pragma unroll
        for (int sb = 0; sb < NSB; ++sb) {
            bf16x8 pf;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pf[r] = (bf16)s[2 * sb][r];
                pf[4 + r] = (bf16)s[2 * sb + 1][r];
            }
#pragma unroll
            for (int nt = 0; nt < NDT; ++nt) {
                const bf16x8 vf = *reinterpret_cast<const bf16x8*>(&Vt[(nt * 16 + lq) * VT_LD + ((sb * 32 + g * 8 + 8 * ((nt * 16 + lq) >> 3)) & (KVB - 1))]);
                acc_o[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc_o[nt], 0, 0, 0);
            }
        }
        j = jn;
        c = cn;
    }
    // ---- the four partials meet in LDS (each in its wave's image): row lq -> [D] un-normalised O (exp2 domain), m, l
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    float* part = reinterpret_cast<float*>(Vt);
#pragma unroll
    for (int nt = 0; nt < NDT; ++nt) *reinterpret_cast<f32x4*>(part + lq * PLD + nt * 16 + g * 4) = acc_o[nt];
    if (g == 0) { part[lq * PLD + D] = m_run; part[lq * PLD + D + 1] = l_run; }
    __syncthreads();
    {   // 256 threads: packed row tid / 16, D / 16 consecutive columns each; the waves' partials are summed in wave order
        const int row = tid >> 4, c0 = (tid & 15) * CPT;
        const int pl = row / G;
        if (pl < cpt && s_row[pl] >= 0) {
            const float* pw[SHR_WAVES];
            float ms[SHR_WAVES], mm = -INFINITY;
#pragma unroll
            for (int w = 0; w < SHR_WAVES; ++w) {
                pw[w] = reinterpret_cast<const float*>(reinterpret_cast<const bf16*>(shr_smem) + w * PER_WAVE) + row * PLD;
                ms[w] = pw[w][D];
                mm = fmaxf(mm, ms[w]);
            }
            const float m_use = (mm == -INFINITY) ? 0.f : mm;
            float l = 0.f, o[CPT];
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc) o[cc] = 0.f;
#pragma unroll
            for (int w = 0; w < SHR_WAVES; ++w) {
                const float wl = (ms[w] == -INFINITY) ? 0.f : exp2f(ms[w] - m_use);
                l += pw[w][D + 1] * wl;
#pragma unroll
                for (int cc = 0; cc < CPT; ++cc) o[cc] += pw[w][c0 + cc] * wl;
            }
            const float inv = l > 0.f ? 1.0f / l : 0.f;        // (rows without a tail: l = 0 -> zeros)
            bf16* op = a.O + (size_t)s_row[pl] * a.o_rs + (size_t)(kh * G + row % G) * a.o_hs + c0;
            const bf16x4 lo = {(bf16)(o[0] * inv), (bf16)(o[1] * inv), (bf16)(o[2] * inv), (bf16)(o[3] * inv)};
            const bf16x4 hi = {(bf16)(o[4] * inv), (bf16)(o[5] * inv), (bf16)(o[6] * inv), (bf16)(o[7] * inv)};
            *reinterpret_cast<bf16x4*>(op) = lo;
            *reinterpret_cast<bf16x4*>(op + 4) = hi;
        }
    }
}

}  // namespace

int ina_launch_attention_shared(const void* Q, long q_rs, long q_hs, void* O, long o_rs, long o_hs, const void* Kc, const void* Vc, long c_ss,
                                long c_rs, long c_hs, int n_slots, const void* Kt, const void* Vt, long t_ps, long t_rs, long t_hs, int T,
                                const int32_t* tile_rows, const int32_t* tile_slot, const int32_t* tile_pfx, const int32_t* tail_len, int n_tiles,
                                int n_rows, int H, int Hkv, int D, int max_pfx, float scale, hipStream_t stream) {
    INA_REQUIRE(D == SHR_D, "attention_shared: head dim %d (128 only)", D);
    INA_REQUIRE(H > 0 && Hkv > 0 && H % Hkv == 0, "attention_shared: bad H/Hkv (%d,%d)", H, Hkv);
    INA_REQUIRE(H / Hkv <= 16, "attention_shared: %d query heads per KV head (at most 16: the heads of one candidate fill a 16-row tile)", H / Hkv);
    INA_REQUIRE(n_tiles > 0 && n_rows > 0 && T > 0, "attention_shared: n_tiles=%d, n_rows=%d, T=%d must be positive", n_tiles, n_rows, T);
    INA_REQUIRE(max_pfx >= 0 && n_slots >= 1, "attention_shared: max_pfx=%d (>= 0), n_slots=%d (>= 1)", max_pfx, n_slots);
    INA_REQUIRE(std::isfinite(scale), "attention_shared: scale %g is not finite", (double)scale);
    INA_REQUIRE(Q && O && Kc && Vc && Kt && Vt && tile_rows && tile_slot && tile_pfx && tail_len,
                "attention_shared: null pointer (q, out, caches, tails and the four tables are required)");
    INA_REQUIRE(q_rs % 8 == 0 && q_hs % 8 == 0 && c_ss % 8 == 0 && c_rs % 8 == 0 && c_hs % 8 == 0 && t_ps % 8 == 0 && t_rs % 8 == 0 && t_hs % 8 == 0 &&
                    o_rs % 4 == 0 && o_hs % 4 == 0,
                "attention_shared: strides must keep 16-byte row alignment");
    INA_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)Kc % 16) == 0 && ((uintptr_t)Vc % 16) == 0 && ((uintptr_t)Kt % 16) == 0 &&
                    ((uintptr_t)Vt % 16) == 0 && ((uintptr_t)O % 8) == 0,
                "attention_shared: misaligned pointer");
    INA_REQUIRE(Hkv <= 65535, "attention_shared: grid of %d tiles x %d KV heads", n_tiles, Hkv);
    SharedArgs a;
    a.Q = reinterpret_cast<const bf16*>(Q); a.O = reinterpret_cast<bf16*>(O);
    a.Kc = reinterpret_cast<const bf16*>(Kc); a.Vc = reinterpret_cast<const bf16*>(Vc);
    a.Kt = reinterpret_cast<const bf16*>(Kt); a.Vt = reinterpret_cast<const bf16*>(Vt);
    a.tile_rows = tile_rows; a.tile_slot = tile_slot; a.tile_pfx = tile_pfx; a.tail_len = tail_len;
    a.q_rs = q_rs; a.q_hs = q_hs; a.o_rs = o_rs; a.o_hs = o_hs; a.c_ss = c_ss; a.c_rs = c_rs; a.c_hs = c_hs; a.t_ps = t_ps; a.t_rs = t_rs; a.t_hs = t_hs;
    a.n_tiles = n_tiles; a.n_rows = n_rows; a.T = T; a.H = H; a.Hkv = Hkv; a.G = H / Hkv; a.cpt = 16 / a.G; a.n_slots = n_slots; a.max_pfx = max_pfx;
    a.scale = scale;
    // algorithmic bound: every row against max_pfx prefix keys + T tail keys; the prefix K / V once per (tile, KV head), the tails once per row
    InaProfScope prof(INA_PROF_ATTN, 4.0 * n_rows * H * ((double)max_pfx + T) * D,
                      2.0 * D * ((double)n_rows * H * 2.0 + 2.0 * Hkv * ((double)n_tiles * max_pfx + (double)n_rows * T)), stream);
    constexpr size_t LDS = (size_t)SHR_WAVES * SHR_D * (SHR_CHUNK + 8) * sizeof(bf16);
    static bool attr_done = false;
    if (!attr_done) {
        INA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_shared_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
        attr_done = true;
    }
    hipLaunchKernelGGL(attn_shared_kernel, dim3((unsigned)n_tiles, Hkv), dim3(SHR_WAVES * 64), LDS, stream, a);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
