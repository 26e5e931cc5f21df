// Shared-prefix attention for gfx950 (bf16 in/out, fp32 softmax + accumulation, d = 128): P (prompt, candidate) pairs, each a short causal
// SUFFIX of m rows that also sees a PREFIX kept once per prompt in the System-2 KV cache (score_answers(share_prefix=True): the prompt is
// prefilled once into its cache slot, only the candidates' own tokens run through the stack).
//
//   query row i of pair p (i < suf_len[p]) sees  keys 0 .. pfx_len[p] - 1 of cache slot slot[p]   (the prefix, read in place)
//                                          and   suffix keys j <= i of pair p                     (read from the q|k|v projection buffer)
//
// nothing of another pair, no cache row at or behind pfx_len[p]. Nothing is written to the cache.
//
// Structure: the one-launch decode kernels of attention.hip. The G = H / Hkv query heads of a KV head and their m positions are the ROWS of
// 16-row MFMA tiles (row R -> head kh * G + R / m, position R % m); one four-wave workgroup per (pair, KV head, row tile). The key axis is cut in
// 64-key chunks: chunks 0 .. nc - 1 are the prefix, chunk nc is the (single, causal) suffix chunk; wave w walks chunks w, w + 4, ... with a running
// (max, sum, O) in registers. The chunk step is attention_chunk.h's: K fragments straight from global memory in MFMA operand layout, V through a
// wave-private transposed LDS image, the next chunk requested before the current one is multiplied. The four partials meet in LDS in wave
// order and the workgroup writes the normalised rows itself: no atomics, no workspace, the same bits on every launch.
// Workgroups of the pairs that share a slot are neighbours in the grid (pair index runs faster than the KV head), so that the first of them brings
// the prompt's K/V of that head in from HBM and the others can find it in L2 / Infinity Cache (an expectation: no counter was read).
// Resources: 256 VGPRs + 136 AGPRs (two chunks' K fragments and V pieces live across the prefetch), no scratch -> one workgroup per CU.
//
// attn_prefix_tail_kernel (ina_attention_prefix_tail) is the same body with one more read-only key segment between prefix and suffix: the first
// tail_len[p] rows of tail tail_row[p] of a [n_tail_rows, T, Hkv, 128] buffer in the cache's row format (the latent queries of a SAMPLED answer
// continue what generate left: the prompt in its slot, the answer's K/V in its row of the shared-prefix tails). Chunks of a pair in order:
// prefix chunks 0 .. nc - 1, tail chunks nc .. nc + nt - 1 (64 tail keys each, counted from the tail's row 0), the suffix chunk nc + nt; chunk c
// belongs to wave c mod 4 - a function of the pair alone. With pfx_len % 64 = 0 the chunks and their owners are those attn_prefix_kernel walks
// on a slot that holds [prefix | tail], so the bits are equal; with tail_len = 0 they are attn_prefix_kernel's on the same slot. A chunk that is
// masked for a row (a row at or behind suf_len) leaves the row's state as it was: m = -inf, l = 0, O = 0 stay, alpha = 0 scales zeros.
// A tail_row outside the buffer with tail_len > 0 is treated as a bad slot is: NaN live rows, never an access; tail_len <= 0 never looks at it.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): 256 VGPRs + 40 AGPRs, 74 SGPRs, 73728 bytes of dynamic LDS, no scratch -> one
// workgroup per CU, as attn_prefix_kernel.
#include <cmath>

#include "attention_chunk.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PFX_WAVES = 4, PFX_CHUNK = AC_KVB, PFX_D = 128;

struct PrefixArgs {
    const bf16* Q; bf16* O;
    const bf16 *Kc, *Vc, *Ks, *Vs;
    const int32_t *slot, *pfx_len, *suf_len;
    long q_ps, q_rs, q_hs, o_ps, o_rs, o_hs, c_ss, c_rs, c_hs, s_ps, s_rs, s_hs;
    int P, m, H, Hkv, n_slots, max_pfx, rtiles;
    float scale;
    // the tail segment (attn_prefix_tail_kernel only; attn_prefix_kernel never reads these)
    const bf16 *Kt, *Vt;
    const int32_t *tail_row, *tail_len;
    long t_ps, t_rs, t_hs;
    int n_tail_rows, max_tail;
};

// a key source of a pair (K base, V base, row stride, keys it holds) and a 64-key chunk of one: wave uniform
struct PfxSrc { const bf16 *K, *V; long rs; int len; };
struct PfxChunk { PfxSrc src; int kv0; };
// chunk c of a pair: prefix chunks 0 .. nc - 1, tail chunks nc .. ns - 1 (TAIL only), the suffix chunk ns. (Free functions inlined by force, and
// sources passed by value: written as a by-reference lambda called at two places, with the tail's three-way choice inside it, the compiler kept
// kf, vreg and what the lambda captures in memory - 784 to 1008 bytes of scratch per lane at 96 - 110 VGPRs.)
template <bool TAIL>
__device__ __forceinline__ PfxChunk pfx_chunk(int c, int nc, int ns, PfxSrc pfx, PfxSrc tail, PfxSrc suf) {
    if (c == ns) return {suf, 0};
    if (TAIL && c >= nc) return {tail, (c - nc) * PFX_CHUNK};
    return {pfx, c * PFX_CHUNK};
}
template <int NKK, int D>
__device__ __forceinline__ void pfx_fetch(PfxChunk ch, int lane, bf16x8 (&kf)[AC_NST][NKK], bf16x8 (&vreg)[AC_KVB * (D / 8) / 64]) {
    ac_fetch_kf<NKK, false>(ch.src.K, ch.src.rs, ch.kv0, ch.src.len, D, lane & 15, lane >> 4, kf);
    ac_fetch_v<D>(ch.src.V, ch.src.rs, ch.kv0, ch.src.len, lane, vreg);
}

// the body of both kernels. TAIL = false is attn_prefix_kernel as it always was: every tail term below is a compile-time zero there.
template <bool TAIL>
__device__ __forceinline__ void attn_prefix_body(const PrefixArgs& a) {
    constexpr int D = PFX_D, KVB = PFX_CHUNK, NKK = D / 32, NDT = D / 16;
    constexpr int PER_WAVE = D * AC_VT_LD;                       // bf16 elements of one wave's V^T image
    constexpr int PLD = D + 4;                                // partial row: D x O, m, l (f32), padded to a 16-byte pitch (f32x4 stores)
    constexpr int CPT = D / 16;                               // output columns per thread in the combine
    static_assert(16 * PLD * 4 <= PER_WAVE * 2, "the partial of a wave fits its V^T image");
    extern __shared__ __attribute__((aligned(16))) char pfx_smem[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, lq = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    bf16* Vt = reinterpret_cast<bf16*>(pfx_smem) + wave * PER_WAVE;
    const int rt = blockIdx.x % a.rtiles, p = blockIdx.x / a.rtiles, kh = blockIdx.y;
    const int G = a.H / a.Hkv;
    const int sl = a.slot[p];
    const int pfx = min(max(a.pfx_len[p], 0), a.max_pfx);
    const int suf = min(max(a.suf_len[p], 0), a.m);
    const int tl = TAIL ? min(max(a.tail_len[p], 0), a.max_tail) : 0;           // tail rows this pair sees; 0: tail_row is not looked at
    const int tr = (TAIL && tl > 0) ? a.tail_row[p] : 0;
    const bool bad_slot = sl < 0 || sl >= a.n_slots || (TAIL && (tr < 0 || tr >= a.n_tail_rows));
    bf16* __restrict__ O = a.O + (size_t)p * a.o_ps;

    if (bad_slot || suf == 0) {
        // nothing to attend (zeros), or a slot / tail row outside its buffer: NaN in the pair's live rows (the library's convention), never an access
        const int row = tid >> 4, c0 = (tid & 15) * CPT;
        const int Rr = rt * 16 + row;
        if (Rr < G * a.m) {
            const int hd = kh * G + Rr / a.m, qp = Rr % a.m;
            const bf16 fill = (bf16)((bad_slot && qp < suf) ? NAN : 0.f);
            const bf16x4 f4 = {fill, fill, fill, fill};
            bf16* op = O + (size_t)qp * a.o_rs + (size_t)hd * a.o_hs + c0;
            *reinterpret_cast<bf16x4*>(op) = f4;
            *reinterpret_cast<bf16x4*>(op + 4) = f4;
        }
        return;
    }

    const int R = rt * 16 + lq;                                // packed row of this lane
    const bool live = R < G * a.m;
    const int head = kh * G + (live ? R / a.m : 0), qpos = live ? R % a.m : 0;
    const bool active = live && qpos < suf;                    // rows at or behind suf_len attend nothing: zeros
    const bf16* __restrict__ Q = a.Q + (size_t)p * a.q_ps + (size_t)qpos * a.q_rs + (size_t)head * a.q_hs;
    const bf16* __restrict__ Kc = a.Kc + (size_t)sl * a.c_ss + (size_t)kh * a.c_hs;
    const bf16* __restrict__ Vc = a.Vc + (size_t)sl * a.c_ss + (size_t)kh * a.c_hs;
    const bf16* __restrict__ Ks = a.Ks + (size_t)p * a.s_ps + (size_t)kh * a.s_hs;
    const bf16* __restrict__ Vs = a.Vs + (size_t)p * a.s_ps + (size_t)kh * a.s_hs;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    float m_run = -INFINITY, l_run = 0.f;
    f32x4 acc_o[NDT];
#pragma unroll
    for (int i = 0; i < NDT; ++i) acc_o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 qf[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = active ? *reinterpret_cast<const bf16x8*>(Q + kk * 32 + g * 8) : zero8;

    const int nc = (pfx + KVB - 1) / KVB;                      // prefix chunks 0 .. nc - 1
    const int nt = TAIL ? (tl + KVB - 1) / KVB : 0;            // tail chunks nc .. nc + nt - 1
    const int ns = nc + nt;                                    // chunk ns is the suffix
    const bf16* __restrict__ Kt = TAIL ? a.Kt + (size_t)tr * a.t_ps + (size_t)kh * a.t_hs : nullptr;
    const bf16* __restrict__ Vtl = TAIL ? a.Vt + (size_t)tr * a.t_ps + (size_t)kh * a.t_hs : nullptr;
    bf16x8 kf[AC_NST][NKK], vreg[KVB * (D / 8) / 64];
    const PfxSrc src_pfx = {Kc, Vc, a.c_rs, pfx}, src_suf = {Ks, Vs, a.s_rs, suf};
    const PfxSrc src_tail = {Kt, Vtl, TAIL ? a.t_rs : 0, tl};
    const float sc = a.scale * 1.4426950408889634f;            // exp2 domain
    int c = wave;
    if (c <= ns) pfx_fetch<NKK, D>(pfx_chunk<TAIL>(c, nc, ns, src_pfx, src_tail, src_suf), lane, kf, vreg);
    for (; c <= ns; c += PFX_WAVES) {
        const bool sfx = c == ns;
        const PfxChunk ch = pfx_chunk<TAIL>(c, nc, ns, src_pfx, src_tail, src_suf);
        const int kv0 = ch.kv0, len = ch.src.len;
        f32x4 s[AC_NST];
        ac_scores(kf, qf, s);
        // V registers -> this wave's transposed image (the reads of the previous chunk were consumed by its MFMAs: the LDS queue of a wave is in order)
        ac_store_vt_image<D>(Vt, lane, vreg);
        if (c + PFX_WAVES <= ns)                                // next chunk in flight under this one's math
            pfx_fetch<NKK, D>(pfx_chunk<TAIL>(c + PFX_WAVES, nc, ns, src_pfx, src_tail, src_suf), lane, kf, vreg);
        ac_wave_lds_fence();
        ac_scale_o(acc_o, ac_softmax_update(s, kv0, g, sc, [&](int kv) { return active && kv < len && (!sfx || kv <= qpos); }, m_run, l_run));
        bf16x8 pf[AC_NSB];
        ac_pack_p(s, pf);
        ac_pv<NDT>(Vt, lq, g, pf, acc_o);
    }
    // ---- the four partials meet in LDS (each in its wave's image)
    ac_wave_lds_fence();
    ac_store_partial<PLD>(reinterpret_cast<float*>(Vt), lq, g, acc_o, m_run, l_run);
    __syncthreads();
    {   // 256 threads: row tid / 16, D / 16 consecutive columns each
        const int row = tid >> 4, c0 = (tid & 15) * CPT;
        const int Rr = rt * 16 + row;
        if (Rr < G * a.m) {
            float o[CPT];
            ac_combine<PFX_WAVES, PER_WAVE, PLD, D>(pfx_smem, row, c0, o);       // (rows at or behind suf_len: l = 0 -> zeros)
            const int hd = kh * G + Rr / a.m, qp = Rr % a.m;
            bf16* op = O + (size_t)qp * a.o_rs + (size_t)hd * a.o_hs + c0;
            const bf16x4 lo = {(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
            const bf16x4 hi = {(bf16)o[4], (bf16)o[5], (bf16)o[6], (bf16)o[7]};
            *reinterpret_cast<bf16x4*>(op) = lo;
            *reinterpret_cast<bf16x4*>(op + 4) = hi;
        }
    }
}

__global__ __launch_bounds__(PFX_WAVES * 64) void attn_prefix_kernel(PrefixArgs a) { attn_prefix_body<false>(a); }
__global__ __launch_bounds__(PFX_WAVES * 64) void attn_prefix_tail_kernel(PrefixArgs a) { attn_prefix_body<true>(a); }

// the checks and the launch of both entries; `who` names the entry in every refusal. tail: the four tail arguments are present
int launch_prefix(const char* who, bool tail, const void* Q, long q_ps, long q_rs, long q_hs, void* O, long o_ps, long o_rs, long o_hs, const void* Kc,
                  const void* Vc, long c_ss, long c_rs, long c_hs, int n_slots, const void* Kt, const void* Vt, long t_ps, long t_rs, long t_hs,
                  int n_tail_rows, const void* Ks, const void* Vs, long s_ps, long s_rs, long s_hs, const int32_t* slot, const int32_t* pfx_len,
                  const int32_t* tail_row, const int32_t* tail_len, const int32_t* suf_len, int P, int m, int H, int Hkv, int D, int max_pfx,
                  int max_tail, float scale, hipStream_t stream) {
    INA_REQUIRE(D == PFX_D, "%s: head dim %d (128 only)", who, D);
    INA_REQUIRE(P >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0, "%s: bad P/H/Hkv (%d,%d,%d)", who, P, H, Hkv);
    INA_REQUIRE(m >= 1 && m <= PFX_CHUNK, "%s: m=%d suffix rows (1 .. %d: the suffix is one key chunk)", who, m, PFX_CHUNK);
    INA_REQUIRE(max_pfx >= 0 && n_slots >= 1, "%s: max_pfx=%d (>= 0), n_slots=%d (>= 1)", who, max_pfx, n_slots);
    INA_REQUIRE(std::isfinite(scale), "%s: scale %g is not finite", who, (double)scale);
    INA_REQUIRE(Q && O && Kc && Vc && Ks && Vs && slot && pfx_len && suf_len,
                "%s: null pointer (q, out, caches, suffix k / v and the three tables are required)", who);
    INA_REQUIRE(q_ps % 8 == 0 && q_rs % 8 == 0 && q_hs % 8 == 0 && c_ss % 8 == 0 && c_rs % 8 == 0 && c_hs % 8 == 0 && s_ps % 8 == 0 && s_rs % 8 == 0 &&
                    s_hs % 8 == 0 && o_ps % 4 == 0 && o_rs % 4 == 0 && o_hs % 4 == 0,
                "%s: strides must keep 16-byte row alignment", who);
    INA_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)Kc % 16) == 0 && ((uintptr_t)Vc % 16) == 0 && ((uintptr_t)Ks % 16) == 0 &&
                    ((uintptr_t)Vs % 16) == 0 && ((uintptr_t)O % 8) == 0,
                "%s: misaligned pointer", who);
    if (tail) {
        INA_REQUIRE(n_tail_rows >= 1 && max_tail >= 0, "%s: n_tail_rows=%d (>= 1), max_tail=%d (>= 0)", who, n_tail_rows, max_tail);
        INA_REQUIRE(t_ps % 8 == 0 && t_rs % 8 == 0 && t_hs % 8 == 0 && ((uintptr_t)Kt % 16) == 0 && ((uintptr_t)Vt % 16) == 0,
                    "%s: tail strides and pointers must keep 16-byte row alignment", who);
    }
    if (P == 0) return 0;
    const int G = H / Hkv, rtiles = (G * m + 15) / 16;
    INA_REQUIRE((long)P * rtiles <= 0x7fffffffL && Hkv <= 65535, "%s: grid of %d pairs x %d row tiles x %d KV heads", who, P, rtiles, Hkv);
    PrefixArgs a;
    a.Q = reinterpret_cast<const bf16*>(Q); a.O = reinterpret_cast<bf16*>(O);
    a.Kc = reinterpret_cast<const bf16*>(Kc); a.Vc = reinterpret_cast<const bf16*>(Vc);
    a.Ks = reinterpret_cast<const bf16*>(Ks); a.Vs = reinterpret_cast<const bf16*>(Vs);
    a.slot = slot; a.pfx_len = pfx_len; a.suf_len = suf_len;
    a.q_ps = q_ps; a.q_rs = q_rs; a.q_hs = q_hs; a.o_ps = o_ps; a.o_rs = o_rs; a.o_hs = o_hs;
    a.c_ss = c_ss; a.c_rs = c_rs; a.c_hs = c_hs; a.s_ps = s_ps; a.s_rs = s_rs; a.s_hs = s_hs;
    a.P = P; a.m = m; a.H = H; a.Hkv = Hkv; a.n_slots = n_slots; a.max_pfx = max_pfx; a.rtiles = rtiles; a.scale = scale;
    a.Kt = reinterpret_cast<const bf16*>(Kt); a.Vt = reinterpret_cast<const bf16*>(Vt);
    a.tail_row = tail_row; a.tail_len = tail_len;
    a.t_ps = tail ? t_ps : 0; a.t_rs = tail ? t_rs : 0; a.t_hs = tail ? t_hs : 0;
    a.n_tail_rows = tail ? n_tail_rows : 0; a.max_tail = tail ? max_tail : 0;
    // algorithmic bound: every row against max_pfx prefix (+ max_tail tail) keys + half the suffix; their K / V once per (pair, KV head) at most
    const double before = (double)max_pfx + a.max_tail, keys = before + 0.5 * (m + 1.0);
    InaProfScope prof(INA_PROF_ATTN, 4.0 * P * H * (double)m * keys * D, 2.0 * D * ((double)P * H * m * 2.0 + 2.0 * (double)P * Hkv * (before + m)), stream);
    constexpr size_t LDS = (size_t)PFX_WAVES * PFX_D * (PFX_CHUNK + 8) * sizeof(bf16);
    const dim3 grid((unsigned)(P * rtiles), Hkv);
    // without a tail the entry runs attn_prefix_kernel itself: the bits of ina_attention_prefix by construction
    return tail ? ac_launch_big_lds<attn_prefix_tail_kernel>(grid, PFX_WAVES * 64, LDS, stream, a)
                : ac_launch_big_lds<attn_prefix_kernel>(grid, PFX_WAVES * 64, LDS, stream, a);
}

}  // namespace

int ina_launch_attention_prefix(const void* Q, long q_ps, long q_rs, long q_hs, void* O, long o_ps, long o_rs, long o_hs, const void* Kc,
                                const void* Vc, long c_ss, long c_rs, long c_hs, int n_slots, const void* Ks, const void* Vs, long s_ps, long s_rs,
                                long s_hs, const int32_t* slot, const int32_t* pfx_len, const int32_t* suf_len, int P, int m, int H, int Hkv, int D,
                                int max_pfx, float scale, hipStream_t stream) {
    return launch_prefix("attention_prefix", false, Q, q_ps, q_rs, q_hs, O, o_ps, o_rs, o_hs, Kc, Vc, c_ss, c_rs, c_hs, n_slots, nullptr, nullptr, 0, 0, 0,
                         0, Ks, Vs, s_ps, s_rs, s_hs, slot, pfx_len, nullptr, nullptr, suf_len, P, m, H, Hkv, D, max_pfx, 0, scale, stream);
}

int ina_launch_attention_prefix_tail(const void* Q, long q_ps, long q_rs, long q_hs, void* O, long o_ps, long o_rs, long o_hs, const void* Kc,
                                     const void* Vc, long c_ss, long c_rs, long c_hs, int n_slots, const void* Kt, const void* Vt, long t_ps,
                                     long t_rs, long t_hs, int n_tail_rows, const void* Ks, const void* Vs, long s_ps, long s_rs, long s_hs,
                                     const int32_t* slot, const int32_t* pfx_len, const int32_t* tail_row, const int32_t* tail_len,
                                     const int32_t* suf_len, int P, int m, int H, int Hkv, int D, int max_pfx, int max_tail, float scale,
                                     hipStream_t stream) {
    const int n_tail_args = (Kt != nullptr) + (Vt != nullptr) + (tail_row != nullptr) + (tail_len != nullptr);
    INA_REQUIRE(n_tail_args == 0 || n_tail_args == 4,
                "attention_prefix_tail: k_tail, v_tail, tail_row and tail_len come together (all four, or all null = no tail)");
    return launch_prefix("attention_prefix_tail", n_tail_args == 4, Q, q_ps, q_rs, q_hs, O, o_ps, o_rs, o_hs, Kc, Vc, c_ss, c_rs, c_hs, n_slots, Kt, Vt,
                         t_ps, t_rs, t_hs, n_tail_rows, Ks, Vs, s_ps, s_rs, s_hs, slot, pfx_len, tail_row, tail_len, suf_len, P, m, H, Hkv, D, max_pfx,
                         max_tail, scale, stream);
}
