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
// for a row leaves that row's running (max, sum, O) exactly as it was (alpha = 1 by construction - never exp2(-inf - -inf) -, e = 0, O += 0:
// the UNIT_ALPHA form of ac_softmax_update, attention_chunk.h, which holds the chunk step of this kernel).
// So every wave sees, per row, the row's own chunks in the row's own order whatever else shares the tile. The four partials meet in LDS in wave
// order and the workgroup writes the normalised rows itself: no atomics, no workspace, the same bits on every launch.
#include <cmath>

#include "attention_chunk.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SHR_WAVES = 4, SHR_CHUNK = AC_KVB, SHR_D = 128;

struct SharedArgs {
    const bf16* Q; bf16* O;
    const bf16 *Kc, *Vc, *Kt, *Vt;
    const int32_t *tile_rows, *tile_slot, *tile_pfx, *tail_len;
    long q_rs, q_hs, o_rs, o_hs, c_ss, c_rs, c_hs, t_ps, t_rs, t_hs;
    int n_tiles, n_rows, T, H, Hkv, G, cpt, n_slots, max_pfx;
    float scale;
};

__global__ __launch_bounds__(SHR_WAVES * 64) void attn_shared_kernel(SharedArgs a) {
    constexpr int D = SHR_D, KVB = SHR_CHUNK, NKK = D / 32, NDT = D / 16;
    constexpr int PER_WAVE = D * AC_VT_LD;                       // bf16 elements of one wave's V^T image
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
    bf16x8 kf[AC_NST][NKK], vreg[KVB * (D / 8) / 64];
    auto fetch = [&](int j, int c) {
        const bool tail = j >= 0;
        const size_t toff = tail ? (size_t)s_row[j] * a.t_ps + (size_t)kh * a.t_hs : 0;
        const bf16* Kb = tail ? a.Kt + toff : Kc;
        const bf16* Vb = tail ? a.Vt + toff : Vc;
        const long rs = tail ? a.t_rs : a.c_rs;
        const int kv0 = c * KVB, len = tail ? s_tl[j] : pfx;
        ac_fetch_kf<NKK, false>(Kb, rs, kv0, len, D, lq, g, kf);
        ac_fetch_v<D>(Vb, rs, kv0, len, lane, vreg);
    };
    const float sc = a.scale * 1.4426950408889634f;            // exp2 domain
    int j = -1, c = wave - SHR_WAVES;
    advance(j, c);
    if (j < cpt) fetch(j, c);
    while (j < cpt) {
        const int kv0 = c * KVB, len = j < 0 ? pfx : s_tl[j];
        const bool mine = active && (j < 0 || j == place);     // a tail chunk of another place: masked for this row
        f32x4 s[AC_NST];
        ac_scores(kf, qf, s);
        ac_store_vt_image<D>(Vt, lane, vreg);
        int jn = j, cn = c;
        advance(jn, cn);
        if (jn < cpt) fetch(jn, cn);                           // next chunk in flight under this one's math
        ac_wave_lds_fence();
        ac_scale_o(acc_o, ac_softmax_update<true>(s, kv0, g, sc, [&](int kv) { return mine && kv < len; }, m_run, l_run));
        bf16x8 pf[AC_NSB];
        ac_pack_p(s, pf);
        ac_pv<NDT>(Vt, lq, g, pf, acc_o);
        j = jn;
        c = cn;
    }
    // ---- the four partials meet in LDS (each in its wave's image)
    ac_wave_lds_fence();
    ac_store_partial<PLD>(reinterpret_cast<float*>(Vt), lq, g, acc_o, m_run, l_run);
    __syncthreads();
    {   // 256 threads: packed row tid / 16, D / 16 consecutive columns each
        const int row = tid >> 4, c0 = (tid & 15) * CPT;
        const int pl = row / G;
        if (pl < cpt && s_row[pl] >= 0) {
            float o[CPT];
            ac_combine<SHR_WAVES, PER_WAVE, PLD, D>(shr_smem, row, c0, o);       // (rows without a tail: l = 0 -> zeros)
            bf16* op = a.O + (size_t)s_row[pl] * a.o_rs + (size_t)(kh * G + row % G) * a.o_hs + c0;
            const bf16x4 lo = {(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
            const bf16x4 hi = {(bf16)o[4], (bf16)o[5], (bf16)o[6], (bf16)o[7]};
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
    return ac_launch_big_lds<attn_shared_kernel>(dim3((unsigned)n_tiles, Hkv), SHR_WAVES * 64, LDS, stream, a);
}
