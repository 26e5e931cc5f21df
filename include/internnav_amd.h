/* internnav_amd - C ABI of the MI355X (gfx950) InternVLA-N1 / NavDP policy engine.
 *
 * The reference (InternRobotics/InternNav) is 100 % Python: its hot path reaches the GPU only through
 * torch / transformers / diffusers / flash-attn, so there is no reference FFI to mirror.
 * This header is the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md): plain pointers,
 * sizes and a hipStream_t; the caller (PyTorch-ROCm) owns every tensor, the library owns only its workspace.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on error; ina_last_error() gives the message (thread-local).
 *  - all device pointers are HBM addresses on the current HIP device; `stream` is a hipStream_t passed as void*.
 *  - bf16 = bfloat16 (uint16 storage); "f32" params (bias, norm weights, gates) are float32.
 *  - functions are stream-ordered and never synchronise the device.
 */
#ifndef INTERNNAV_AMD_H
#define INTERNNAV_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INA_ABI_VERSION 8

/* activation codes (GEMM epilogue) */
#define INA_ACT_NONE_C 0
#define INA_ACT_GELU_ERF_C 1
#define INA_ACT_GELU_TANH_C 2
#define INA_ACT_RELU_C 3
#define INA_ACT_SILU_C 4
#define INA_ACT_MISH_C 5
/* dtype codes */
#define INA_BF16 0
#define INA_F32 1

int ina_abi_version(void);
const char* ina_last_error(void);
/* Fails (non-zero) unless a gfx950 device is current; fills name[0..n) with the arch string. */
int ina_device_check(char* name, int n);
/* sizeof() of the k-th argument struct below (0 gemm, 1 attn, 2 norm, 3 patchify, 4 embed3, 5 head3, 6 seqpool, 7 select, 8 pool_act, 9 gather, 10 rope, 11 mrope_table, 12 argmax, 13 dit_attn, 14 resize_u8, 15 qwen_patchify, 16 u8_lut, 17 resize_f32, 18 gn_mish, 19 pad_rows, 20 ddim_step, 21 ew, 22 colsum, 23 norm_bwd, 24 transpose, 25 sparse_rows, 26 small_linear, 27 mse, 28 adamw, 29 gemm_nn, 30 attn_bwd, 31 dit_rowchain, 32 gemm_dw):
 * lets a binding verify its struct mirrors against the compiled layout. */
int ina_struct_size(int k);
/* Per-launch timing for the benchmark's roofline line: while enabled every launch is bracketed by a hipEvent pair on its
 * stream and its algorithmic FLOPs / bytes are tallied per kernel class (0 tiled MFMA gemm, 1 attention, 2 norm, 3 elementwise,
 * 4 weight-streaming skinny gemm (M <= 64, HBM-bound)).
 * ina_prof_enable(0|1) also clears the tally; ina_prof_read synchronises on the recorded events. Eager launches only. */
/* Library-owned scratch (split-K partials of the skinny GEMM, flash-decoding partials) lives in numbered slots [0, 8). Launches
 * use the slot current at issue time (default 0) and a captured graph keeps it: graphs that may replay concurrently on different
 * streams must be captured under different slots.
 * The current slot is per host thread. A buffer that a captured graph has seen is never freed: if a later launch under the same
 * slot needs more, a new buffer serves new launches and the old one is retired but stays allocated (ina_workspace_retired() counts
 * them), so graphs captured earlier keep replaying into valid memory. */
int ina_set_workspace_slot(int slot);
int ina_workspace_retired(void);
int ina_prof_enable(int on);
int ina_prof_read(int kind, double* ms_total, int64_t* launches, double* flops, double* bytes);
/* the same tally restricted to one kernel of the class: sub = GEMM tile config id (18 = gemm_bf16_pp_kernel<256,256,4>, 21 = <192,256,4>,
 * 22 = gemm_bf16_glds_kernel<128,128,2,2,1>, 33 = gemm_bf16_glds_kernel<256,256,4,4,2>, 11 / 14 / 26 / 27 other LDS-DMA tiles, 1-5 gemm_bf16_nt_kernel tiles, 34 / 35 = gemm_bf16_rowpanel_kernel<8|4 waves>, 39 = gemm_bf16_w4_kernel<256> (four-wave 256x256 tile), 40 = gemm_bf16_w4p_kernel<256> (the same tile on fragment-ordered weights), 42 = dit_rowchain_kernel, 43 = gemm_dw_kernel; in class 4: 48 = the fp8-weight kernels of ina_gemm_w8, 49 = the MXFP4-weight kernels of ina_gemm_mx4) */
int ina_prof_read_sub(int kind, int sub, double* ms_total, int64_t* launches, double* flops, double* bytes);

/* ---- C[M,N] = epilogue(A[M,K] . W[N,K]^T): replaces every nn.Linear / patch-embed conv on the path
 *      (reference: torch.nn.Linear call sites, e.g. dinov2_layers/attention.py:46-48, mlp.py:27-29,
 *       navdp.py:94-100, internvla_n1_arch.py:129-134; transformers Qwen2.5-VL q/k/v/o/mlp projections).
 *      Epilogue order, the same in every kernel: +bias[n] -> act -> *colscale[n] -> *rowscale[m / rowscale_div] -> +R[m,n] -> store;
 *      glu: act(gate + bias_g) * (up + bias_u) * rowscale. Refused (non-zero return): act outside INA_ACT_NONE_C .. INA_ACT_TANH_C, and
 *      glu together with R or colscale - no kernel computes those. */
typedef struct ina_gemm_args {
    const void* A;          /* bf16 [M,K], row stride lda (elements) */
    const void* W;          /* bf16 [N,K], row stride ldw */
    void* C;                /* bf16|f32 [M,N] (N/2 columns in glu mode), row stride ldc */
    const float* bias;      /* f32 [N] or NULL */
    const float* colscale;  /* f32 [N] or NULL (LayerScale gamma) */
    const float* rowscale;  /* f32 [M / rowscale_div] or NULL */
    const void* R;          /* residual [M,N] or NULL, dtype res_dtype, row stride ldr */
    int32_t M, N, K;
    int32_t lda, ldw, ldc, ldr;
    int32_t act;            /* INA_ACT_*_C (0 .. 6, INA_ACT_TANH_C included); any other value is refused */
    int32_t out_dtype;      /* INA_BF16 | INA_F32 */
    int32_t res_dtype;
    int32_t glu;            /* 1: W rows interleaved [gate16|up16], C = act(gate) * up */
    int32_t rowscale_div;   /* 0 means 1 */
    int32_t batch;          /* 0 means 1; grid.y batches with the element strides below */
    int64_t strideA, strideW, strideC, strideR;
    int32_t force_cfg;      /* 0 = auto tile selection; -1 = auto for a launch that shares the device with another stream's GEMMs (tile quantisation not charged); > 0 = that tile config */
    int32_t group_m;        /* tile order of the LDS-DMA kernels: 0 = auto, 1 = row-major, n > 1 = groups of n row-tiles (L2 locality) */
    /* fused input RMSNorm (M <= 16, the single-token decode passes of the LLM: transformers Qwen2RMSNorm in front of q/k/v and gate/up):
     * C = epilogue(bf16(A * rsqrt(mean(A^2) + norm_eps) * norm_gamma) . W^T) with A of dtype a_dtype - the separate norm launch and its
     * bf16 round trip disappear (every workgroup normalises the <= 16 rows into LDS while its first weight tiles are in flight) */
    const float* norm_gamma; /* f32 [K] or NULL (no fused norm; A is bf16) */
    float norm_eps;
    int32_t a_dtype;        /* dtype of A when norm_gamma is set: INA_BF16 | INA_F32 */
    /* LayerNorm statistics of the produced rows (row-panel kernels only: K = 384, plain epilogue, N a multiple of 384, M >= 16384 rows): seg_stats
     * f32 [M, N / 384, 2] receives (mean, 1 / sqrt(var + seg_eps)) of every 384-wide segment of C's fp32 row - what ina_dit_attention(stats=)
     * consumes (the fused q1|k1|v1|q2 projection of a NextDiT block). Refused, not ignored, where another kernel would run. */
    float* seg_stats;
    float seg_eps;
    int32_t _pad_seg;
    const void* Wp;         /* NULL, or the same W in MFMA fragment order (ina_gemm_preshuffle; N % 16 == 0, K % 32 == 0): tile config 40 takes its
                             * B fragments from it straight into registers (selected where cfg 39 would run; bit-equal results) */
} ina_gemm_args;
int ina_gemm_bf16(const ina_gemm_args* args, void* stream);
/* The weight-streaming kernels (M <= 64; with norm_gamma: M <= 16, the fused input RMSNorm) on FP8 weights: W8 holds OCP e4m3 (e4m3fn) bytes,
 * one per weight, and wexp[n] a power-of-two exponent per output row; the weight is q[n,k] * 2^wexp[n] (|wexp| <= 64), which is exactly a bf16
 * number. The result is, bit for bit, ina_gemm_bf16's weight-streaming result (kernel 32 / 30) on those dequantised bf16 weights: same K
 * decomposition and summation order, the row scale applied to the reduced fp32 sum before the bias. Half the weight bytes per launch.
 * Packed row layout (K % 128 == 0): element k = step * 128 + s * 32 + g * 8 + j (s < 4, g < 4, j < 8) is byte step * 128 + g * 32 + s * 8 + j of
 * its row; rows are ldw BYTES apart (ldw >= K, a multiple of 16). args->W is ignored; every other field means what it means for ina_gemm_bf16.
 * Refused (non-zero, ina_last_error; checked before any HIP call): M > 64, K % 128 != 0, batch > 1, seg_stats, Wp, force_cfg > 0, norm_gamma
 * with M > 16 / K > 4096 / N < 256, and the glu / R / colscale / act combinations ina_gemm_bf16 refuses.
 * Profiler tally: class 4 (weight streaming), sub 48, with N * K + N weight bytes. */
int ina_gemm_w8(const ina_gemm_args* args, const void* W8, const int8_t* wexp, void* stream);
/* The same weight-streaming kernels on MXFP4 weights (OCP microscaling): W4 holds e2m1 elements, two per byte, and wscale one e8m0 byte
 * (127 + e, |e| <= 64, never 0xFF) per block of 32 consecutive k; the weight is q[n,k] * 2^e[n,k/32] with |q| in {0, .5, 1, 1.5, 2, 3, 4, 6},
 * exactly a bf16 number. The result is, bit for bit, ina_gemm_bf16's weight-streaming result (kernel 32 / 30) on those dequantised bf16
 * weights: same K decomposition and summation order; the block scale is applied inside the (exact) e2m1 -> bf16 conversion, so nothing is
 * left for the epilogue. 0.53 bytes per weight.
 * Packed row layout (K % 128 == 0): element k = step * 128 + s * 32 + g * 8 + j (s < 4, g < 4, j < 8) is nibble j (bits 4j .. 4j + 3) of the
 * little-endian dword g * 4 + s of the 64-byte K step `step` of its row; rows are ldw BYTES apart (ldw >= K / 2, a multiple of 16). Scales
 * in natural order: row n, block b at wscale[n * (K / 32) + b], contiguous, 4-byte aligned. args->W is ignored; every other field means
 * what it means for ina_gemm_bf16.
 * Refused (non-zero, ina_last_error; checked before any HIP call): null pointers, M > 64, K % 128 != 0, ldw < K / 2 or not a multiple of
 * 16, batch > 1, seg_stats, Wp, force_cfg > 0, norm_gamma with M > 16 / K > 4096 / N < 256, and the glu / R / colscale / act combinations
 * ina_gemm_bf16 refuses.
 * Profiler tally: class 4 (weight streaming), sub 49, with N * K / 2 + N * K / 32 weight bytes. */
int ina_gemm_mx4(const ina_gemm_args* args, const void* W4, const void* wscale, void* stream);
/* W bf16 [N,K] (row stride ldw) -> Wp bf16 [N*K]: fragment (n / 16, k / 32) is one contiguous KiB, element (n, k) at
 * ((n / 16) * (K / 32) + k / 32) * 512 + ((k % 32) / 8 * 16 + n % 16) * 8 + k % 8. Done once per weight at load time. */
int ina_gemm_preshuffle(const void* W, void* Wp, int32_t N, int32_t K, int64_t ldw, void* stream);
/* Which kernel ina_gemm_bf16 would run for these arguments - validation and tile selection only, nothing is launched and no GPU is needed
 * (the selection is host arithmetic on M / N / K, the epilogue and force_cfg): *kernel = 1-5 register-staged tiles, 11-27 / 33 LDS-DMA tiles
 * (18 = 256x256 ping-pong, 21 = 192x256 ping-pong, 22 / 26 / 27 single-buffer tiles of the d = 384 heads, 33 = 256x256 with 16 waves),
 * 34 / 35 row-panel kernels (K = 384), 39 / 40 the 256x256 tile on four waves of 128x128 (39 is selected for wide no-residual K = 2048 .. 4096 GEMMs, 40 instead of it when Wp is given),
 * 30 = weight streaming with the fused input RMSNorm, 32 = weight streaming (M <= 64). Returns non-zero (and sets ina_last_error)
 * exactly when ina_gemm_bf16 would reject the arguments. */
int ina_gemm_select(const ina_gemm_args* args, int* kernel);

/* ---- flash-style attention forward (bf16, fp32 softmax): replaces flash_attn / SDPA / nn.MultiheadAttention
 *      (reference call sites: dinov2_layers/attention.py:49-62, navdp.py:57-66,192, navdp_backbone.py:77,148,
 *       nextdit_traj.py:147-165; transformers Qwen2.5-VL vision/text attention). Strides in elements. */
typedef struct ina_attn_args {
    const void* Q;
    const void* K;
    const void* V;
    void* O;
    int64_t q_bs, q_rs, q_hs;
    int64_t k_bs, k_rs, k_hs;
    int64_t v_bs, v_rs, v_hs;
    int64_t o_bs, o_rs, o_hs;
    int32_t B, H, Hkv;
    int32_t Lq, Lk;
    int32_t D;              /* 48 | 64 | 80 | 128 */
    int32_t causal;
    int32_t kv_start;       /* keys < kv_start masked */
    int32_t kv_bdiv;        /* K/V batch = b / kv_bdiv (0 means 1) */
    float scale;
    const int32_t* cu_q;    /* int32 [B+1] varlen offsets or NULL */
    const int32_t* cu_k;
    const float* head_gate; /* f32 [H] or NULL: O *= tanh(gate[h]) */
    const int32_t* k_len;   /* int32 [B / kv_bdiv] or NULL: valid keys per K/V batch (dense mode; Lk is then the maximum) */
    int32_t accumulate;     /* 1: O += result */
    /* training only - attention-probability dropout of nn.MultiheadAttention(dropout=p) in train mode (dense layouts, no decode path):
     * P[b,h,q,k] is kept iff ina_hash(drop_seed, ((b*H + h)*Lq + q)*Lk + k) >= drop_thresh and scaled by drop_scale = 1 / (1 - p);
     * drop_thresh = p * 2^32, 0 = off. The backward kernel regenerates the same mask from the same numbers. */
    uint32_t drop_seed;
    uint32_t drop_thresh;
    float drop_scale;
    int32_t kernel;         /* (decode shapes - few query rows against a long dense KV - have their own kernels: 0 = one launch (d = 128: eight waves,
                             * K fragments straight from global memory; otherwise four waves), 1 = the split + combine pair, 3 = the four-wave one-launch kernel.)
                             * 0 = automatic (long dense shapes run the 32-rows-per-wave kernel of attention_wide.hip, everything else the
                             * 16-rows-per-wave kernel), 1 = the 16-rows-per-wave kernel, 2 = the 32-rows-per-wave kernel (an error outside its
                             * contract: d 64 / 80 / 128, Lq and Lk >= 128 - or packed d-80 sequences of <= 64 tokens, the Qwen ViT windows - no head gate /
                             * accumulate / dropout). Same result up to the bf16
                             * rounding of P and O; parity tests pin both and compare them. */
    int32_t _pad0;
    const uint32_t* drop_salt; /* training, optional: one device word ADDED to drop_seed when the kernel starts - a launch sequence captured in a
                                * hipGraph draws fresh masks on every replay (the host bumps the word between replays); NULL = drop_seed alone */
    /* single-token decoder passes (d = 128, causal, 256 <= Lk <= 1024, Lq <= 8: the one-launch decode kernel): the rotary embedding of the NEW tokens
     * and their KV-cache append inside the attention launch - what ina_rope_bf16 with KV set does in a launch of its own. Q holds the UN-rotated
     * query heads; k_new / v_new the un-rotated key / raw value heads of the Lq new tokens (element strides kn_bs per sequence, kn_rs per token,
     * kn_hs per kv head - the q|k|v projection buffer); the kernel rotates q in registers, writes rotate(k_new) and v_new into rows
     * len_k - Lq .. len_k - 1 of K / V (the cache) and then attends. Same arithmetic and rounding as the separate launch. NULL: Q / K / V as given.
     * PRECONDITION (the caller's: k_len lives on the device, the host-side checks cannot see it): every k_len[b] >= Lq (and Lk >= Lq without
     * k_len) - len_k counts the new tokens; a smaller k_len[b] would put the append rows BEFORE row 0 of the cache, and the kernel does not guard
     * that write. Without rope_cos any k_len[b] >= 0 is fine (rows without a key come out as zeros). */
    const float* rope_cos;     /* f32 [B * Lq, 128] or NULL */
    const float* rope_sin;
    const void* k_new;
    const void* v_new;
    int64_t kn_bs, kn_rs, kn_hs;
} ina_attn_args;
int ina_attention_bf16(const ina_attn_args* args, void* stream);

/* One-level row map: logical row r -> physical row (r / seg_len) * seg_stride + off + r % seg_len (seg_len 0 = identity).
 * Lets norm / embed kernels drop the ViT cls token, concatenate token groups and scatter into [env, slot] buffers
 * (reference: torch.cat call sites navdp_backbone.py:187,281; navdp_policy.py:162-164; navdp.py:182-185). */
typedef struct ina_rowmap {
    int32_t seg_len, seg_stride, off, _pad;
} ina_rowmap;

/* ---- LayerNorm / RMSNorm (+ NextDiT modulation / tanh gate / base add / positional table); reference: nn.LayerNorm call
 *      sites (dinov2_layers/block.py:83-87, navdp.py:78,193), diffusers RMSNorm / LuminaRMSNormZero (nextdit_traj.py:109-119,146,172-176).
 *      t = norm(X[in_map(r)]) * gamma + beta ; t *= 1 + mod_scale[r/mod_div] ; t *= tanh(gate[r/mod_div]) ; t += G[r] ; t += P[r % p_mod]
 *      -> Y[out_map(r)] (bf16) and/or Y32[out_map(r)] (f32).
 *      Chained pre-norm (Y2 != NULL): Y2[out_map(r)] = norm(t) * gamma2 * (1 + mod_scale2[r/mod_div]) (bf16; same rms / eps) - the
 *      next sub-block's modulated norm of the residual row this call just produced (LuminaNextDiTBlock: norm2 -> ffn_norm1,
 *      ffn_norm2 -> next block's norm1). */
typedef struct ina_norm_args {
    const void* X;          /* bf16|f32 (x_dtype) rows of C, row stride ldx */
    void* Y;                /* bf16 out or NULL */
    void* Y32;              /* f32 out or NULL */
    const float* gamma;     /* f32 [C] or NULL */
    const float* beta;      /* f32 [C] or NULL */
    const float* mod_scale; /* f32 [rows/mod_div, mod_ld] or NULL */
    const float* gate;      /* f32 [rows/mod_div, mod_ld] or NULL */
    const void* G;          /* bf16|f32 (g_dtype) [rows, ldg] base added after gating, or NULL */
    const float* P;         /* f32 [p_mod, C] table or NULL */
    ina_rowmap in_map, out_map;
    int32_t rows, C;
    int32_t ldx, ldy, ldy32, ldg;
    int32_t x_dtype, g_dtype;
    int32_t mod_div, mod_ld;
    int32_t p_mod, rms;
    float eps;
    int32_t ldy2;
    void* Y2;               /* bf16 chained output or NULL */
    const float* gamma2;    /* f32 [C] or NULL */
    const float* mod_scale2;/* f32 [rows/mod_div, mod_ld] or NULL */
} ina_norm_args;
int ina_norm_bf16(const ina_norm_args* args, void* stream);

/* ---- patchify: NHWC frames -> im2col rows of the ViT patch-embed conv, fused with the input normalisation.
 *      out[(i*gh + py)*gw + px, c*ps*ps + y*ps + x] = (img[i, py*ps+y, px*ps+x, c] - mean[c]) * inv_std[c]   (bf16),
 *      columns >= 3*ps*ps are zero padding. C == 1 replicates the channel 3x (depth frames).
 *      C == 4, 6, 7 (NavDPNet goal-image / goal-pixel encoders, navdp_backbone.py:316-412): identity normalisation only (mean 0,
 *      inv_std 1), out[.., c*ps*ps + y*ps + x] = bf16(img[.., c]) for c < C, columns >= C*ps*ps are zero padding.
 *      reference: navdp_backbone.py:155-181,258-279 + dinov2_layers/patch_embed.py:151-164 (Conv2d 14x14 stride 14). */
typedef struct ina_patchify_args {
    const void* img;        /* f32|bf16 (in_dtype) [n, H, W, C], C in {1, 3, 4, 6, 7} */
    void* out;              /* bf16 [n * gh * gw, ldo] */
    float mean[3];
    float inv_std[3];
    int32_t n, H, W, C;
    int32_t ps, ldo, in_dtype, _pad;
} ina_patchify_args;
int ina_patchify(const ina_patchify_args* args, void* stream);

/* ---- embed3: Y[out_map(r)] = W[:, 0:3] . X[r, 0:3] + b + P[r % p_mod]   (nn.Linear(3, C) + positional table; X NULL = table fill)
 *      reference: input_embed / point_encoder / action_encoder (navdp_policy.py:160,165; navdp.py:178,190; internvla_n1.py:402-410). */
typedef struct ina_embed3_args {
    const float* X;         /* f32 [rows, 3] or NULL */
    const float* W;         /* f32 [C, 3] */
    const float* b;         /* f32 [C] or NULL */
    const float* P;         /* f32 [p_mod, C] or NULL */
    void* Y;                /* bf16|f32 (out_dtype) */
    ina_rowmap out_map;
    int32_t rows, C, ldy, p_mod;
    int32_t out_dtype, x_div;   /* x row = r / x_div (0 means 1): broadcast one vector to x_div consecutive rows */
} ina_embed3_args;
int ina_embed3(const ina_embed3_args* args, void* stream);

/* ---- goal_slots: the goal rows of the NavDPNet condition for B envs with goals of mixed kinds, one launch
 *      reference: NavDPNet.predict_noise writes one goal embedding into condition slots 1..3 (navdp_policy.py:159-170); the embedding is
 *      point_encoder(goal) or ImageGoalBackbone / PixelGoalBackbone.forward (navdp_backbone.py:340-346, 391-397).
 *  env b, kind[b]:  0 none   e = 0
 *                   1 point  e = point_w [D,3] . point[row[b]] + point_b
 *                   2 image  e = image_w [D,E] . mean_{t < ntok} image_tok[row[b]*ntok + t] + image_b   (fp32 mean of the tower's f32 tokens)
 *                   3 pixel  the same with the pixel_* operands
 *  Y[b*L + slot0 + j] = e + P[slot0 + j] for j < nslots (Y bf16|f32 per y_dtype, row stride ldy; P f32 [>= slot0 + nslots, D] or NULL);
 *  embed (f32 [B, D] or NULL) receives e. row[b] indexes the compact input of its kind (n_point / n_image / n_pixel rows); the caller
 *  validates the plan - an entry outside it yields NaN rows, never an out-of-bounds read. Plain arguments: no struct, no ABI bump. */
int ina_goal_slots(void* Y, int32_t ldy, int32_t y_dtype, int32_t L, int32_t slot0, int32_t nslots, const float* P, int32_t B, int32_t D,
                   const int32_t* kind, const int32_t* row, float* embed, const float* point, int32_t n_point, const float* point_w,
                   const float* point_b, const float* image_tok, int32_t n_image, const float* image_w, const float* image_b,
                   const float* pixel_tok, int32_t n_pixel, const float* pixel_w, const float* pixel_b, int32_t ntok, int32_t E, void* stream);

/* ---- kv_copy: row ranges of the System-2 KV cache between the engine's cache slots and caller-owned tensors, all layers and sequences
 *      of a call in ONE launch (a 16-byte vector bit copy, graph capturable).
 *  layer_base: device int64 [n_layers], address of layer l's cache (rows of row_bytes bytes, engine_rows of them);
 *  seq: device int64 [n_seq, 4] = { caller address of the sequence's layer-0 first row, caller layer stride in bytes,
 *       first engine row (slot * S_max + first cached position), n_rows }; the caller side holds n_rows contiguous rows per layer.
 *  to_engine 0: engine -> caller (export), 1: caller -> engine (import). max_rows >= every n_rows (sizes the grid);
 *  row_bytes a multiple of 16, every address 16-byte aligned. An entry outside [0, engine_rows) copies nothing.
 *  Plain arguments: no struct, no ABI bump. */
int ina_kv_copy(int32_t to_engine, const int64_t* layer_base, int32_t n_layers, const int64_t* seq, int32_t n_seq, int64_t engine_rows,
                int64_t row_bytes, int64_t max_rows, void* stream);

/* ---- attention_prefix: causal self-attention of P short suffixes that also see a prefix kept ONCE in the System-2 KV cache, one launch
 *      (teacher-forced scoring of several candidate answers behind one prefilled prompt: score_answers(share_prefix=True)).
 *  bf16 in / out, fp32 softmax and accumulation, strides in elements, D = 128.
 *  Q, O       P pairs x m rows x H heads x D: element (p, i, h, d) at p * ?_ps + i * ?_rs + h * ?_hs + d;
 *  k_cache, v_cache   the engine's cache layout: key / value row r of slot s, KV head kh at s * c_ss + r * c_rs + kh * c_hs (one set of
 *             strides for both pointers), n_slots slots, at least max_pfx rows in each;
 *  k_suf, v_suf       the pairs' own keys / values (the k and v columns of the q|k|v projection after the in-place rotary embedding):
 *             row j of pair p, KV head kh at p * s_ps + j * s_rs + kh * s_hs (one set of strides for both pointers);
 *  slot, pfx_len, suf_len   device int32 [P].
 *  Query row i of pair p, i < suf_len[p], sees keys 0 .. min(pfx_len[p], max_pfx) - 1 of cache slot slot[p] and suffix keys j <= i of
 *  pair p: nothing of another pair, no cache row at or behind pfx_len[p]. pfx_len 0 = plain causal self-attention over the suffix.
 *  Output rows i >= suf_len[p] are written as zeros. A slot[p] outside [0, n_slots) yields NaN in the rows i < suf_len[p] of that pair
 *  and never an out-of-bounds access. Nothing is written to the cache. No atomics, no workspace: two launches give the same bits;
 *  device tables only: graph capturable.
 *  Contract: D = 128, H % Hkv = 0, 1 <= m <= 64 (the suffix is one 64-key chunk), suf_len <= m (clipped), max_pfx >= 0, n_slots >= 1,
 *  16-byte aligned Q / K / V rows (strides multiples of 8, pointers of 16 bytes), 8-byte aligned O rows; anything else is refused before
 *  any HIP call. P = 0 returns 0 and launches nothing. Plain arguments: no struct, no ABI bump. */
int ina_attention_prefix(const void* Q, int64_t q_ps, int64_t q_rs, int64_t q_hs, void* O, int64_t o_ps, int64_t o_rs, int64_t o_hs,
                         const void* k_cache, const void* v_cache, int64_t c_ss, int64_t c_rs, int64_t c_hs, int32_t n_slots, const void* k_suf,
                         const void* v_suf, int64_t s_ps, int64_t s_rs, int64_t s_hs, const int32_t* slot, const int32_t* pfx_len,
                         const int32_t* suf_len, int32_t P, int32_t m, int32_t H, int32_t Hkv, int32_t D, int32_t max_pfx, float scale, void* stream);

/* ---- attention_prefix_tail: attention_prefix with one more read-only key segment between prefix and suffix, one launch (the latent queries
 *      of a SAMPLED answer continue the state generate left behind: the prompt in its cache slot, the answer's own K/V either behind it in a
 *      slot of its own or in its row of the shared-prefix tail buffer - no second prefill).
 *  bf16 in / out, fp32 softmax and accumulation, strides in elements, D = 128. Q, O, k_cache, v_cache, k_suf, v_suf, slot, pfx_len, suf_len
 *  and their strides: as for ina_attention_prefix.
 *  k_tail, v_tail     n_tail_rows tails in the cache's row format (a layer of the engine's shared-prefix tails): key / value row t of tail r,
 *             KV head kh at r * t_ps + t * t_rs + kh * t_hs (one set of strides for both pointers), at least max_tail rows in each;
 *  tail_row, tail_len   device int32 [P]: the tail of pair p and how many of its rows the pair sees.
 *  Query row i of pair p, i < suf_len[p], sees keys 0 .. min(pfx_len[p], max_pfx) - 1 of cache slot slot[p], then rows 0 ..
 *  min(tail_len[p], max_tail) - 1 of tail tail_row[p], then suffix keys j <= i of pair p: nothing of another pair, no cache row at or behind
 *  pfx_len[p], no tail row at or behind tail_len[p]. Two pairs may name the same slot and the same tail. tail_len[p] <= 0: tail_row[p] is
 *  not looked at (-1 is legal) and the pair is computed as by ina_attention_prefix, bit for bit. k_tail, v_tail, tail_row and tail_len all
 *  NULL: no tail at all, the launch IS ina_attention_prefix's (n_tail_rows, max_tail and the tail strides are ignored); some of them NULL
 *  is refused.
 *  Output rows i >= suf_len[p] are written as zeros. A slot[p] outside [0, n_slots), or a tail_row[p] outside [0, n_tail_rows) with
 *  tail_len[p] > 0, yields NaN in the rows i < suf_len[p] of that pair and never an out-of-bounds access. Nothing is written to the cache or
 *  the tails. The key axis is cut in 64-key chunks per segment (prefix, tail, suffix); their order and owners depend on the pair alone, so
 *  the bits of a pair do not depend on its neighbours, and a pair with pfx_len % 64 = 0 has the bits ina_attention_prefix gives on a slot
 *  that holds [prefix | tail]. No atomics, no workspace: two launches give the same bits; device tables only: graph capturable.
 *  Contract: that of ina_attention_prefix, and with a tail n_tail_rows >= 1, max_tail >= 0, tail strides multiples of 8, tail pointers
 *  16-byte aligned; anything else is refused before any HIP call. P = 0 returns 0 and launches nothing.
 *  Plain arguments: no struct, no ABI bump. */
int ina_attention_prefix_tail(const void* Q, int64_t q_ps, int64_t q_rs, int64_t q_hs, void* O, int64_t o_ps, int64_t o_rs, int64_t o_hs,
                              const void* k_cache, const void* v_cache, int64_t c_ss, int64_t c_rs, int64_t c_hs, int32_t n_slots, const void* k_tail,
                              const void* v_tail, int64_t t_ps, int64_t t_rs, int64_t t_hs, int32_t n_tail_rows, const void* k_suf, const void* v_suf,
                              int64_t s_ps, int64_t s_rs, int64_t s_hs, const int32_t* slot, const int32_t* pfx_len, const int32_t* tail_row,
                              const int32_t* tail_len, const int32_t* suf_len, int32_t P, int32_t m, int32_t H, int32_t Hkv, int32_t D,
                              int32_t max_pfx, int32_t max_tail, float scale, void* stream);

/* ---- attention_shared: single-token attention of n_rows rows (one returned sequence each) whose prompts stay ONCE in the System-2 KV cache,
 *      one launch (generate(do_sample=True, num_return_sequences=K, share_prefix=True): K sampled answers per prompt, no cache slot per answer).
 *  bf16 in / out, fp32 softmax and accumulation, strides in elements, D = 128, G = H / Hkv <= 16.
 *  Q, O       n_rows rows x H heads x D: element (r, h, d) at r * ?_rs + h * ?_hs + d;
 *  k_cache, v_cache   the engine's cache layout: key / value row i of slot s, KV head kh at s * c_ss + i * c_rs + kh * c_hs (one set of
 *             strides for both pointers), n_slots slots, at least max_pfx rows in each;
 *  k_tail, v_tail     the rows' own keys / values (their answer tokens, the current one included), in the cache's row format: tail row t of
 *             row r, KV head kh at r * t_ps + t * t_rs + kh * t_hs (one set of strides for both pointers), T tail rows per row;
 *  tile_rows  device int32 [n_tiles, cpt], cpt = 16 / G: the rows that share one 16-row MFMA tile - rows of the SAME prompt -, -1 = an empty
 *             place (skipped; so is an index outside [0, n_rows)); a row named twice is computed twice;
 *  tile_slot, tile_pfx   device int32 [n_tiles]: the cache slot of the tile's prompt and its cached length; tail_len device int32 [n_rows].
 *  Row r of tile t sees keys 0 .. min(tile_pfx[t], max_pfx) - 1 of cache slot tile_slot[t] and the first min(tail_len[r], T) rows of its own
 *  tail: nothing of another row's tail, no cache row at or behind tile_pfx[t]. tail_len[r] <= 0: the row comes out as zeros. A tile_slot[t]
 *  outside [0, n_slots) yields NaN in the rows of that tile that have a tail (zeros in the others) and never an out-of-bounds access. Rows no
 *  tile names are not written. Nothing is written to the cache. The bits of a row do not depend on which rows share its tile nor on their
 *  tail lengths; no atomics, no workspace: two launches give the same bits; device tables only: graph capturable.
 *  Contract: D = 128, H % Hkv = 0, H / Hkv <= 16, n_tiles / n_rows / T >= 1, max_pfx >= 0, n_slots >= 1, 16-byte aligned Q / K / V rows (strides
 *  multiples of 8, pointers of 16 bytes), 8-byte aligned O rows; anything else is refused before any HIP call.
 *  Plain arguments: no struct, no ABI bump. */
int ina_attention_shared(const void* Q, int64_t q_rs, int64_t q_hs, void* O, int64_t o_rs, int64_t o_hs, const void* k_cache, const void* v_cache,
                         int64_t c_ss, int64_t c_rs, int64_t c_hs, int32_t n_slots, const void* k_tail, const void* v_tail, int64_t t_ps, int64_t t_rs,
                         int64_t t_hs, int32_t T, const int32_t* tile_rows, const int32_t* tile_slot, const int32_t* tile_pfx, const int32_t* tail_len,
                         int32_t n_tiles, int32_t n_rows, int32_t H, int32_t Hkv, int32_t D, int32_t max_pfx, float scale, void* stream);

/* ---- memory_gather: the visual-memory rows of the NavDPNet former's token buffer for n stepped envs of a rollout, from a per-env ring of
 *      cached frame tokens, in ONE launch (graph capturable; reference memory semantics: navdp_lerobot_dataset.py:215-222).
 *  ring  f32 [max_envs, depth, ntok, C]: final-LayerNorm tokens of each env's last depth = (M - 1) * stride + 1 frames, without positions;
 *  fresh f32 [n, ntok, C]: the tokens of this step's new frame of launch row i; blank f32 [ntok, C]: the tokens of an all-zero frame;
 *  pe    f32 [M * ntok, C]: the former's positional table; env / head / count: device int32 [n] = the env of launch row i, the ring slot its
 *  new frame goes to, and its pushes since the last reset (this one included).
 *  ring[env[i], head[i]] = fresh[i];  out[i * out_env_stride + (j * ntok + p) * C ...] (bf16, contiguous rows) = bf16(src + pe[j * ntok + p]) with
 *  src = fresh[i] for j = M - 1, ring[env[i], (head[i] - (M-1-j) * stride) mod depth] when (M-1-j) * stride < count[i], else blank.
 *  The env ids of one launch are distinct (caller's contract); an entry outside the ring yields NaN rows, never an out-of-bounds access.
 *  16-byte aligned tensors, C a multiple of 8. Plain arguments: no struct, no ABI bump. */
int ina_memory_gather(void* out, int64_t out_env_stride, float* ring, const float* fresh, const float* blank, const float* pe, const int32_t* env,
                      const int32_t* head, const int32_t* count, int32_t n, int32_t max_envs, int32_t M, int32_t ntok, int32_t C, int32_t depth,
                      int32_t stride, void* stream);

/* ---- traj_actions: the step's action table from the sampled System-1 trajectories of B envs, in ONE launch (graph capturable, no host
 *      synchronisation) - what vln_utils.traj_to_actions computes on the host per env (vln_utils.py:63-136), rounding for rounding.
 *  traj  f32|bf16 (traj_dtype: INA_F32 | INA_BF16) [B, S, T, 3], the S samples of an env contiguous (generate_traj's [S * B, T, 3]); x, y are
 *        x4-scaled increments. Per env: x, y * 0.25; sequential fp32 running sum over t per sample; fp64 mean over the S samples in sample order
 *        with a leading zero row -> the mean trajectory [T + 1, 2]; greedy pure pursuit in fp64 (0.25 m steps, 15 degree turns, look-ahead 4, stop
 *        radius 0.2 m): 1 forward, 2 left, 3 right.
 *  actions int32 [B, max_actions] = the first max_actions entries of the host's list, zero-padded; count int32 [B] = min(len(list), max_actions).
 *        1 <= max_actions <= 256; the loop ends once max_actions entries exist (the policy path uses 4).
 *  traj_out f64 [B, T + 1, 2] or NULL: receives the mean trajectory (bit-equal to the host's numpy result).
 *  scale_in_place != 0: x * 0.25, y * 0.25 are written back into traj, the reference's in-place un-normalisation (vln_utils.py:129).
 *  S >= 1, 1 <= T <= 1023. atan2 / cos / sin differ from the host libm by a few ulp: a decision whose margin is below that may fall the other
 *  way (margins of real trajectories are >= 1e-5; tests/traj_actions_ref.py). Plain arguments: no struct, no ABI bump. */
int ina_traj_actions(void* traj, int32_t traj_dtype, int32_t B, int32_t S, int32_t T, int32_t* actions, int32_t max_actions, int32_t* count,
                     double* traj_out, int32_t scale_in_place, void* stream);

/* ---- head3: final norm + Linear(C, 3) + sampler update, one wave per row.
 *      e = W . (norm(X[r]) * gamma + beta) * (1 + mod_scale[r / mod_div]) ... + b
 *      mode 0: eps_out[r] = e ; mode 1 (DDPM, diffusers DDPMScheduler.step): x0 = clamp((s - c1 e) c0, +-clip),
 *      s <- c2 x0 + c3 s + c4 noise[r] ; mode 2 (FlowMatch Euler): s <- s + c0 e.
 *      reference: navdp_policy.py:167-169,312-315; navdp.py:193-195,247-250; internvla_n1.py:418-431. */
typedef struct ina_head3_args {
    const void* X;          /* bf16|f32 (x_dtype) [rows, ldx] */
    const float* gamma;     /* f32 [C] or NULL */
    const float* beta;      /* f32 [C] or NULL */
    const float* mod_scale; /* f32 [rows/mod_div, mod_ld] or NULL */
    const float* W;         /* f32 [3, C] */
    const float* b;         /* f32 [3] */
    float* sample;          /* f32 [rows, 3], updated in place (modes 1, 2) */
    const float* noise;     /* f32 [rows, 3] or NULL */
    float* eps_out;         /* f32 [rows, 3] or NULL */
    float coef[5];
    float clip;
    float eps;
    int32_t rows, C, ldx, x_dtype;
    int32_t mode, mod_div, mod_ld;
} ina_head3_args;
int ina_head3(const ina_head3_args* args, void* stream);

/* ---- seqpool_head: out[s] = w . mean_t( norm(X[s*T + t]) * gamma + beta ) + b   (critic head, navdp_policy.py:183-184) */
typedef struct ina_seqpool_args {
    const void* X;
    const float* gamma;
    const float* beta;
    const float* w;         /* f32 [C] */
    const float* b;         /* f32 [1] */
    float* out;             /* f32 [nseq] */
    float eps;
    int32_t nseq, T, C, ldx, x_dtype, _pad;
} ina_seqpool_args;
int ina_seqpool_head(const ina_seqpool_args* args, void* stream);

/* ---- pool_act: Y[s, :] = act( mean_{t < T} X[s*T + t, :] + P[s % p_mod, :] )   (T = 1: bias + activation)
 *      reference: masked mean of the caption features + SiLU(temb) (diffusers LuminaCombinedTimestepCaptionEmbedding,
 *      LuminaRMSNormZero as used by nextdit_traj.py:109-119, 355). */
typedef struct ina_pool_act_args {
    const void* X;          /* bf16|f32 (x_dtype) [nseq*T, ldx] */
    const float* P;         /* f32 [p_mod, C] or NULL */
    void* Y;                /* bf16|f32 (out_dtype) [nseq, ldy] */
    int32_t nseq, T, C, ldx, ldy, p_mod;
    int32_t x_dtype, out_dtype, act, _pad;
} ina_pool_act_args;
int ina_pool_act(const ina_pool_act_args* args, void* stream);

/* ---- gather_rows: Y[dst ? dst[r] : r, :] = X[src ? src[r] : r, :]   (bit copy of `row_bytes` per row)
 *      reference: embed_tokens lookup, masked_scatter of image embeds, latent_queries rows (internvla_n1.py:129-172),
 *      the ViT window permutation and its inverse (transformers modeling_qwen2_5_vl.py:434-466). */
typedef struct ina_gather_args {
    const void* X;
    void* Y;
    const int32_t* src;     /* int32 [rows] or NULL */
    const int32_t* dst;     /* int32 [rows] or NULL */
    int64_t ldx_bytes, ldy_bytes;
    int32_t rows, row_bytes; /* row_bytes multiple of 16 */
} ina_gather_args;
int ina_gather_rows(const ina_gather_args* args, void* stream);

/* ---- rope: in-place rotary embedding of `heads` heads of width D starting at column `col0` of each row:
 *      x' = x * cos + rotate_half(x) * sin with per-row tables cos/sin f32 [*, D] (row tab ? tab[r] : r).
 *      reference: apply_rotary_pos_emb_vision / apply_multimodal_rotary_pos_emb (transformers modeling_qwen2_5_vl.py:160-171,557-599). */
typedef struct ina_rope_args {
    void* X;                /* bf16 rows, row stride ldx (elements) */
    const float* cos;
    const float* sin;
    const int32_t* tab;     /* int32 [rows] table row per logical row, or NULL */
    ina_rowmap map;         /* logical row -> physical row of X */
    int32_t rows, heads, D, ldx, col0, _pad;
    /* optional fused KV-cache append (decoder layers: q|k|v rows -> rotate q in place, write rotated k and the raw v of each row into
     * the cache row kv_dst[r]): heads [kv_head0, heads) are the key heads, v_heads value heads follow them in X; the cache row holds
     * [k heads | v heads] contiguously. KV == NULL: plain in-place rope on all heads. */
    void* KV;               /* bf16 cache rows, row stride ldkv, or NULL */
    const int32_t* kv_dst;  /* int32 [rows] cache row per logical row */
    int32_t kv_head0, v_heads, ldkv, _pad2;
} ina_rope_args;
int ina_rope_bf16(const ina_rope_args* args, void* stream);

/* ---- mrope_table: cos/sin [n, D] from the 3-D (t, h, w) position ids of Qwen2.5-VL: frequency f = j % (D/2) uses axis
 *      axis_of[f] (mrope_section [16, 24, 24] -> 0 x16, 1 x24, 2 x24); angle = pos[axis][i] * inv_freq[f].
 *      reference: Qwen2_5_VLRotaryEmbedding.forward + mrope interleave (modeling_qwen2_5_vl.py:525-538,582-590); position ids
 *      from internnav/dataset/rope2d.py:6 (get_rope_index_25). */
typedef struct ina_mrope_table_args {
    const int32_t* pos;     /* int32 [3, n] */
    const float* inv_freq;  /* f32 [D/2] */
    const int32_t* axis_of; /* int32 [D/2] */
    float* cos;             /* f32 [n, D] */
    float* sin;
    int32_t n, D;
} ina_mrope_table_args;
int ina_mrope_table(const ina_mrope_table_args* args, void* stream);

/* ---- argmax_rows: out[r] = argmax_j X[r, j] (first maximum), greedy decoding (HF generate do_sample=False).
 *      NaN entries are never selected; a row with no entry above -inf (all -inf or all NaN) returns 0. The result is always in [0, n). */
typedef struct ina_argmax_args {
    const float* X;         /* f32 [rows, ldx] */
    int32_t* out;           /* int32 [rows] */
    int32_t rows, n, ldx, _pad;
} ina_argmax_args;
int ina_argmax_rows(const ina_argmax_args* args, void* stream);

/* ---- token_seen_set / argmax_penalty_rows: the repetition penalty of greedy decoding, what HF generate() applies on every greedy step when
 *      the checkpoint's generation_config.json sets repetition_penalty (RepetitionPenaltyLogitsProcessor over prompt + answer so far).
 *  A row's seen set is a bitmap: token t is bit t & 31 of word t >> 5 of seen[r] (uint32 [rows, ld_words], ld_words * 32 >= n).
 *
 *  token_seen_set: seen[r] becomes exactly the bitmap of { ids[r, i] : i < lens[r], 0 <= ids[r, i] < n } (ids int32 [rows, ld_ids], lens int32
 *  [rows], at most ld_ids ids of a row are read). Bits left by an earlier call are cleared in the same launch; the bits of the last word
 *  beyond n, the words at or beyond ceil(n / 32) and rows >= rows are left untouched. Ids outside [0, n) are ignored, never an out-of-bounds
 *  access. One workgroup per row builds the bitmap in LDS (no global atomics): n <= 262144 (a 32 KiB LDS bitmap), a larger vocabulary is
 *  refused.
 *
 *  argmax_penalty_rows: out[r] = argmax_j y[r, j] by the selection rule of argmax_rows (first maximum, NaN never selected, a row without an entry
 *  above -inf gives 0, the result always in [0, n)), with y = x where the token's bit is clear and y = x < 0 ? x * penalty : x / penalty (fp32,
 *  IEEE division: bit-equal to torch on the host) where it is set. X (f32 [rows, ldx]) is NOT modified. mark != 0: the chosen token's bit is
 *  then set in seen[r] (the row's workgroup is its only writer), so decode steps chain without host work. penalty must be finite and > 0.
 *  Refusals (null pointers, rows <= 0, n <= 0, ld_words * 32 < n, bad penalty) return non-zero before any HIP call.
 *  Plain arguments: no struct, no ABI bump. */
int ina_token_seen_set(uint32_t* seen, int32_t ld_words, const int32_t* ids, int32_t ld_ids, const int32_t* lens, int32_t rows, int32_t n, void* stream);
int ina_argmax_penalty_rows(const float* X, int32_t ldx, int32_t rows, int32_t n, uint32_t* seen, int32_t ld_words, float penalty, int32_t mark,
                            int32_t* out, void* stream);

/* ---- logprob_rows: log-softmax of a vocabulary row at ONE index, fused with the greedy selection - HF's generate(output_scores=True) +
 *      compute_transition_scores(normalize_logits=True) without a [rows, vocab] tensor leaving the device; with `target`, the per-token
 *      log-likelihood of caller-supplied tokens (teacher forcing).
 *  y[r] is row r of X (f32 [rows, ldx], NOT modified): x itself with seen == NULL, else the repetition-penalised row of argmax_penalty_rows
 *  (y = x < 0 ? x * penalty : x / penalty where the token's bit is set in seen[r], uint32 [rows, ld_words], ld_words * 32 >= n).
 *  tok[r]:     target == NULL: the selection of argmax_rows / argmax_penalty_rows over y (first maximum, NaN never selected, a row without an
 *              entry above -inf gives 0) - bit-equal to those kernels on the same input; mark != 0 (needs seen) then sets the chosen token's
 *              bit in seen[r] in the same launch. target != NULL (int32 [rows]): tok[r] = target[r]; mark is refused. A target outside [0, n)
 *              is an ignored label (HF's -100): logprob[r] = 0, margin[r] = 0, the row is not read.
 *  logprob[r]: y[tok] - max(y) - log sum_j exp(y[j] - max(y)) in fp32 with expf / logf (= torch.log_softmax(y, -1)[tok]). A NaN anywhere in
 *              the row gives NaN; -inf entries contribute 0; an all -inf row gives NaN.
 *  margin[r]:  (may be NULL) y[tok] - the largest y at any OTHER index (NaN entries skipped; n == 1: +inf). >= 0 when tok was selected:
 *              the top-2 margin of the decision.
 *  One workgroup per row (any rows >= 0; rows == 0 launches nothing). Refusals (X / tok / logprob NULL, rows < 0, n < 1, ldx < n,
 *  ld_words * 32 < n or a penalty that is not finite and > 0 when seen is set, mark without seen or with target) return non-zero before any
 *  HIP call. Plain arguments: no struct, no ABI bump. */
int ina_logprob_rows(const float* X, int32_t ldx, int32_t rows, int32_t n, uint32_t* seen, int32_t ld_words, float penalty, int32_t mark,
                     const int32_t* target, int32_t* tok, float* logprob, float* margin, void* stream);

/* ---- sample_rows: one sampling step of HF generate(do_sample=True) - repetition penalty, temperature, top-k, top-p (HF's processor order) and
 *      the draw - in ONE launch in place of the argmax / logprob launch. No random number is generated on the device: u holds one uniform
 *      in [0, 1) per output row, drawn by the caller.
 *  Output row r reads logits row s = src ? src[r] : r of X (f32 [x_rows, ldx], NOT modified); seen (uint32 [rows, ld_words], may be NULL), u
 *  and every output are indexed by r, so K draws of one prompt can come from one logits row. A src entry outside [0, x_rows) is never
 *  accessed: tok 0, logprob NaN, n_kept 0, thr NaN.
 *   1. y = x, or the repetition-penalised row of argmax_penalty_rows over seen[r]; z = y / temperature, one IEEE fp32 division (bit-equal
 *      to torch's scores / temperature). -0 counts as +0. NaN entries are never kept.
 *   2. top_k > 0: with k = min(top_k, entries that are not NaN) and v_k the k-th largest z, keep z >= v_k (ties at v_k all stay, as
 *      TopKLogitsWarper keeps them). 0 = off.
 *   3. top_p < 1, over what top-k kept, with softmax masses p_i: a VALUE v stays iff the mass of the kept entries with z <= v is
 *      > 1 - top_p. Entries that share a value stay or go together (tie-free rows: TopPLogitsWarper(min_tokens_to_keep=1); with ties the
 *      superset of what HF keeps under any sort order); the maximum always stays. 1 = off (entries of mass 0 stay in the kept set).
 *      thr[r] = the smallest kept value, n_kept[r] = the number of entries with z >= thr[r] (both may be NULL).
 *   4. q_i = p_i / (kept mass); tok[r] = the first kept index, in ascending token id, whose inclusive cumulative q exceeds u[r].
 *   5. logprob[r] = log q_tok: the log-softmax of HF's processed scores at the draw (compute_transition_scores(normalize_logits=True)),
 *      with expf / logf.
 *  -inf entries have mass 0 and are never drawn; a row with nothing above -inf gives tok 0, logprob NaN, n_kept 0, thr NaN. The result is
 *  always in [0, n). mark != 0 (needs seen) sets the drawn token's bit in seen[r] in the same launch. Masses are summed as 44-bit fixed-point
 *  integers: two launches on the same inputs give the same bits in every output. n <= 262144.
 *  Refusals (X / tok / logprob / u NULL, rows < 0, x_rows < 1, n < 1, n > 262144, ldx < n, rows > x_rows without src, a temperature that is
 *  not finite and > 0, top_k < 0, top_p outside (0, 1], ld_words * 32 < n or a penalty that is not finite and > 0 when seen is set, mark
 *  without seen) return non-zero before any HIP call. Plain arguments: no struct, no ABI bump. */
int ina_sample_rows(const float* X, int32_t ldx, int32_t x_rows, int32_t rows, int32_t n, uint32_t* seen, int32_t ld_words, float penalty, int32_t mark,
                    float temperature, int32_t top_k, float top_p, const float* u, const int32_t* src, int32_t* tok, float* logprob, int32_t* n_kept,
                    float* thr, void* stream);

/* ---- automaton_mask_rows: constrained decoding - a deterministic automaton over token classes, consulted in front of the selection
 *      kernels above (which all treat -inf as "mass 0, never chosen"); what HF's prefix_allowed_tokens_fn does, without a host round trip.
 *  Tables: token_class u8 [vocab] (4-byte aligned), allow u32 [n_states, 8] (class c allowed in state s = bit c & 31 of word c >> 5 of
 *  allow[s]), next u8 [n_states, 256]; 1 <= n_states <= 256. X f32 [rows, ldx] with n <= vocab live columns, modified IN PLACE.
 *  Per row r:
 *   advance  prev_tok == NULL: s = state_in[r]. Else s0 = state_in[r], t = prev_tok[r]: s = next[s0][class(t)] if s0 is in [0, n_states),
 *            t in [0, n) and class(t) in allow[s0]; otherwise s = -1, and no table is read through the bad index. state_out[r] = s.
 *   mask     s in [0, n_states): X[r][i] = -inf for every i < n whose class is not in allow[s]; allowed entries are not written (a NaN
 *            there stays that NaN; X is never read). s outside that range: the row is left exactly as it is. Columns >= n are never touched.
 *  state_in and state_out (int32 [rows]) must not overlap: a row is spread over many workgroups, each of which derives s from state_in. No
 *  atomics: two launches on the same inputs give the same bits. The tables are read-only. rows == 0 launches nothing.
 *  Refusals (a NULL pointer other than prev_tok, rows outside [0, 65535], n < 1, ldx < n, n > vocab, n_states outside [1, 256], a misaligned
 *  token_class, overlapping state buffers) return non-zero before any HIP call. Plain arguments: no struct, no ABI bump. */
int ina_automaton_mask_rows(float* X, int32_t ldx, int32_t rows, int32_t n, const uint8_t* token_class, int32_t vocab, const uint32_t* allow,
                            const uint8_t* next, int32_t n_states, const int32_t* state_in, const int32_t* prev_tok, int32_t* state_out, void* stream);

/* ---- beam search of System-2 decoding (decode_beam.hip): transformers' GenerationMixin._beam_search as three launches per step, K = num_beams
 *      hypotheses per prompt in rows b * K .. b * K + K - 1, M = max(2, 1 + n_eos) * K candidates per prompt. tests/beam_ref.py restates the rules.
 *
 *  beam_topm_rows: per output row r (logits row s = src ? src[r] : r of X f32 [x_rows, ldx]; seen, run_score and the outputs are indexed by r):
 *   y = log_softmax(X[s]) in fp32 (expf / logf); with seen, the repetition penalty ON y - bit i of seen[r] set: y < 0 ? y * penalty : y / penalty
 *   (HF runs its logits processors on the log-probabilities in beam search); acc = y + run_score[r]. cand_score / cand_tok [rows, M]: the M best
 *   entries by (acc descending, token id ascending). A NaN logit counts as -inf; a row without a number has every y = -inf; a NaN acc counts
 *   as -inf; -inf entries fill up in id order. +inf logits are not supported. A src outside [0, x_rows) is never accessed: scores -inf, ids
 *   0 .. M-1. X and seen are only read. No atomics: two launches give the same bits. 2 <= M <= min(32, n), rows <= 65535.
 *
 *  beam_step: one workgroup per prompt. cand_* [B * K, M] as beam_topm_rows wrote them. step = index of the answer token this step selects
 *   (L = step + 1); step 0 starts the prompt: running scores [0, -1e9, ...], an empty finished set, heuristic flag on, not done - whatever the
 *   buffers hold - and merges row b * K only. A prompt whose done[b] != 0 (step > 0) is frozen: nothing of it is written.
 *   candidates  the M best of the K rows' lists by (score descending, beam * V + token ascending)
 *   hit         token in eos[0 .. n_eos), or L == max_new_tokens
 *   running     the K best by score + hit * -1e9 (ties by position) -> next_tok / parent (GLOBAL row b * K + beam) / run_score [B * K], the token
 *               histories hist_out [B * K, T] and per-token transition scores ts_out (score - the parent's running score) gathered by parent from
 *               hist_in / ts_in (the other buffer of a pair) with the new token appended at column step
 *   finished    fin_tok / fin_ts [B * K, T], fin_score / fin_len / fin_flag [B * K], best first: old entries, then the candidates with score / L **
 *               length_penalty, + -1e9 when the heuristic flag is off, + -1e9 when early_stopping is 1 and the set was full, + -1e9 when the
 *               candidate did not hit or is not among the first K; the K best stay (ties by position)
 *   heur[b]     &= any_k(run_score[0] / H ** length_penalty > (fin_flag[k] ? min(fin_score) : -1e9)), H = max_new_tokens when early_stopping is
 *               2 ("never") and length_penalty > 0, else L
 *   done[b]     = heur off, or early_stopping 1 and all K finished, or all M candidates hit
 *   All arithmetic is HF's, in fp32. early_stopping: 0 False, 1 True, 2 "never". K <= 8, K <= M <= 32, n_eos <= 8, step < max_new_tokens <= T.
 *
 *  beam_reorder: re-parents the per-row state in front of the next pass. For layer l < n_layers the first t rows of the T-row tail of row r at
 *   dst_base[l] + r * T * row_bytes come from row parent[r] at src_base[l] (device tables of addresses; the two sets must not overlap;
 *   row_bytes % 16 == 0); seen_dst[r] = seen_src[parent[r]] | bit next_tok[r] (ld_words words per row; a token outside [0, n) marks nothing);
 *   state_dst[r] = state_src[parent[r]]. seen_* / state_* may be NULL in pairs. A parent outside [0, rows) copies nothing for its row and causes
 *   no access.
 *  Refusals return non-zero before any HIP call. Plain arguments: no struct, no ABI bump. */
int ina_beam_topm_rows(const float* X, int32_t ldx, int32_t x_rows, int32_t rows, int32_t n, const uint32_t* seen, int32_t ld_words, float penalty,
                       const float* run_score, const int32_t* src, int32_t M, float* cand_score, int32_t* cand_tok, void* stream);
int ina_beam_step(const float* cand_score, const int32_t* cand_tok, int32_t B, int32_t K, int32_t M, int32_t T, int32_t step, int32_t max_new_tokens,
                  float length_penalty, int32_t early_stopping, const int32_t* eos, int32_t n_eos, float* run_score, int32_t* next_tok, int32_t* parent,
                  const int32_t* hist_in, int32_t* hist_out, const float* ts_in, float* ts_out, int32_t* fin_tok, float* fin_ts, float* fin_score,
                  int32_t* fin_len, int32_t* fin_flag, int32_t* heur, int32_t* done, void* stream);
int ina_beam_reorder(const int64_t* src_base, const int64_t* dst_base, int32_t n_layers, const int32_t* parent, int32_t rows, int32_t T, int32_t t,
                     int64_t row_bytes, const uint32_t* seen_src, uint32_t* seen_dst, int32_t ld_words, const int32_t* next_tok, int32_t n,
                     const int32_t* state_src, int32_t* state_dst, void* stream);

/* ---- logit_rules_rows: transformers' logits processors sequence_bias, no_repeat_ngram_size, bad_words_ids, min_length / min_new_tokens,
 *      forced_eos_token_id, suppress_tokens and begin_suppress_tokens as tables on the device, applied in front of the selection kernels above
 *      (and behind automaton_mask_rows: the forced 0.0 wins over the automaton's -inf, as HF orders them). One workgroup per row; but for the
 *      forced fill the vocabulary is not walked. X f32 [rows, ldx] with n live columns, modified IN PLACE at selection step `col` (0 = the first
 *      answer token). Row r's history is hist[r * ld_hist .. + hist_cap): its prompt's len0[r] real tokens (written by the caller), then its answer.
 *   1 append   col > 0: hist[r][len0[r] + col - 1] = prev_tok[r] (idempotent). The live history is H = len0[r] + col tokens. A row whose
 *              len0[r] is outside [0, hist_cap - col] has NO history: nothing is stored and no history rule fires for it.
 *   2 biases   groups g < n_bias, one per DISTINCT target t = grp_tok[g]: b = grp_base[g]; for s in [grp_ptr[g], grp_ptr[g + 1]) in order, when
 *              sequence s matches, b += seq_bias[s] (fp32); then X[r][t] += b once. Sequence s holds seq_ids[seq_ptr[s] .. seq_ptr[s + 1]) = its
 *              L - 1 tokens before the target (1 <= L - 1 <= 31); it matches iff H >= L and the history ends in them.
 *   3 bans     -inf at: every token that follows an occurrence of the history's last ngram - 1 tokens inside the history (ngram >= 1 and
 *              H >= ngram; ngram 1: every token of the history); the target of every group g in [n_bias, n_groups) one of whose sequences
 *              matches; eos_tok[] while col < eos_first[r].
 *   4 forced   col == forced_col and n_forced > 0: the whole row -inf, then 0.0 at forced_tok[].
 *   5 static   -inf at ban_tok[] (every step) and at begin_tok[] (col == 0) - behind 4, as HF runs suppress_tokens behind forced_eos_token_id.
 *  Ids outside [0, n) - in the history, prev_tok or any list - are compared but never used as an index. Entries no rule names are not
 *  written (a NaN there stays that NaN); columns >= n are never touched; the tables are read-only. No atomics: two launches on the same
 *  inputs give the same bits. Limits: ngram <= 16, n_seqs <= 1024. rows == 0 launches nothing.
 *  Refusals (NULL X / hist / len0, prev_tok NULL with col > 0, a positive count with a NULL table, rows outside [0, 65535], n < 1, ldx < n,
 *  hist_cap < 1, ld_hist < hist_cap, col outside [0, hist_cap], ngram outside [0, 16], n_bias > n_groups, n_seqs > 1024) return non-zero
 *  before any HIP call. Plain arguments: no struct, no ABI bump. */
int ina_logit_rules_rows(float* X, int32_t ldx, int32_t rows, int32_t n, int32_t col, int32_t* hist, int32_t ld_hist, int32_t hist_cap, const int32_t* len0,
                         const int32_t* prev_tok, int32_t ngram, const int32_t* grp_tok, const float* grp_base, const int32_t* grp_ptr, int32_t n_bias,
                         int32_t n_groups, const int32_t* seq_ptr, const int32_t* seq_ids, const float* seq_bias, int32_t n_seqs, int32_t n_ids,
                         const int32_t* ban_tok, int32_t n_ban, const int32_t* begin_tok, int32_t n_begin, const int32_t* eos_tok, int32_t n_eos,
                         const int32_t* eos_first, const int32_t* forced_tok, int32_t n_forced, int32_t forced_col, void* stream);

/* ---- select_traj: per env, rank the S samples by critic value; neg = the k lowest (ascending), pos = the k highest
 *      (descending); trajectories are cumsum_t(sample * scale).  reference: navdp_policy.py:317-320. */
typedef struct ina_select_args {
    const float* critic;    /* f32 [B, S] */
    const float* sample;    /* f32 [B, S, T, 3] */
    float* neg;             /* f32 [B, k, T, 3] */
    float* pos;             /* f32 [B, k, T, 3] */
    float scale;
    int32_t B, S, T, k, _pad;
} ina_select_args;
int ina_select_traj(const ina_select_args* args, void* stream);

/* ---- frame pre-processing on the device, bit-exact with the host path of the reference:
 *      resize_u8: one axis of PIL's 8-bit ImagingResample (Pillow libImaging/Resample.c): tensor [outer, n_in, inner] -> [outer, n_out,
 *      inner], out = clip8((2^21 + sum_x in[xmin + x] * coefs[xx][x]) >> 22); bounds / coefs are PIL's precompute_coeffs +
 *      normalize_coeffs_8bpc tables (internnav_amd/preprocess.py builds them). Image.resize = W pass, then H pass.
 *      reference: internvla_n1_policy.py:105-116, internvla_n1_agent.py:309-320, HF Qwen2VLImageProcessor.resize. */
typedef struct ina_resize_u8_args {
    const void* in;         /* u8 [outer, n_in, inner] */
    void* out;              /* u8 [outer, n_out, inner] */
    const int32_t* bounds;  /* int32 [n_out, 2] = (xmin, count) */
    const int32_t* coefs;   /* int32 [n_out, ksize] 22-bit fixed point */
    int32_t outer, n_in, n_out, inner, ksize, _pad;
} ina_resize_u8_args;
int ina_resize_u8(const ina_resize_u8_args* args, void* stream);

/*      resize_f32: the same for PIL mode "F" images (the depth frames, internvla_n1_agent.py:313,319): double coefficients, double
 *      accumulation in tap order, one rounding to float (ImagingResampleHorizontal_32bpc / Vertical_32bpc). */
typedef struct ina_resize_f32_args {
    const void* in;         /* f32 [outer, n_in, inner] */
    void* out;              /* f32 [outer, n_out, inner] */
    const int32_t* bounds;  /* int32 [n_out, 2] */
    const double* coefs;    /* f64 [n_out, ksize] */
    int32_t outer, n_in, n_out, inner, ksize, _pad;
} ina_resize_f32_args;
int ina_resize_f32(const ina_resize_f32_args* args, void* stream);

/*      qwen_patchify_u8: HF Qwen2VLImageProcessor rescale + normalize (as a 3 x 256 fp32 table computed with the processor's own
 *      arithmetic) + patchify: rows (grid_h/merge, grid_w/merge, merge, merge), columns (C, tdup copies, ps, ps); bf16 out.
 *      reference: transformers image_processing_qwen2_vl.py (_preprocess / patchify), called at internvla_n1_policy.py:163-165. */
typedef struct ina_qwen_patchify_args {
    const void* img;        /* u8 [n, H, W, 3] */
    void* out;              /* bf16 [n * (H/ps) * (W/ps), ldo] */
    const float* lut;       /* f32 [3, 256] */
    int32_t n, H, W, ps, merge, tdup, ldo, _pad;
} ina_qwen_patchify_args;
int ina_qwen_patchify_u8(const ina_qwen_patchify_args* args, void* stream);

/*      u8_lut: out[i] = bf16(lut[in[i]])  (np.array(img) / 255.0 of the System-1 frames, internvla_n1_agent.py:309-317). */
typedef struct ina_u8_lut_args {
    const void* in;         /* u8 [n] */
    void* out;              /* bf16 [n] */
    const float* lut;       /* f32 [256] */
    int64_t n;
} ina_u8_lut_args;
int ina_u8_lut(const ina_u8_lut_args* args, void* stream);

/* ---- dit_rowchain (round 5): everything of a NextDiT block between two attention stages that is local to a row, in one launch:
 *          P  = A . W1^T (bf16)                                     attn2.to_out (K1 = 384) / feed_forward.linear_2 (K1 = 1024)
 *          X += tanh(gate[r/mod_div]) * rmsnorm(P) * gamma1         norm2 / ffn_norm2 + gate + residual (fp32, in place)
 *          H  = rmsnorm(X) * gamma2 * (1 + mod_scale2[r/mod_div])   ffn_norm1 / the next block's norm1 + adaLN scale
 *          C2 = H . W2^T  (glu2: silu(H . Wg^T) * (H . Wu^T), W2 rows interleaved [gate16 | up16])
 *      replaces GEMM + norm launch + GEMM of diffusers' LuminaNextDiTBlock.forward (diffusers==0.33.1) as wired by
 *      nextdit_traj.py:121-178: the projection and H stay in registers. W2 == NULL: no second GEMM (the last block); H != NULL
 *      additionally writes H (bf16) to memory. Built pairs: (K1 = 384, glu2 = 1) and (K1 = 1024, glu2 = 0); N = 384 fixed.
 *      M and mod_div must be multiples of the 128-row panel. */
typedef struct ina_dit_rowchain_args {
    const void* A;          /* bf16 [M,K1], row stride lda */
    const void* W1;         /* bf16 [384,K1], row stride ldw1 */
    const float* gamma1;    /* f32 [384] RMSNorm weight on the projection */
    const float* gate;      /* f32 [M/mod_div, mod_ld] (tanh applied) or NULL */
    float* X;               /* f32 [M,384] residual stream, updated in place, row stride ldx */
    const float* gamma2;    /* f32 [384] or NULL */
    const float* mod_scale2;/* f32 [M/mod_div, mod_ld] or NULL */
    void* H;                /* bf16 [M,384] or NULL, row stride ldh */
    const void* W2;         /* bf16 [N2,384] or NULL, row stride ldw2 */
    void* C2;               /* bf16 [M,N2] (N2/2 columns with glu2), row stride ldc2 */
    int32_t M, K1, N2;
    int32_t lda, ldw1, ldx, ldh, ldw2, ldc2;
    int32_t glu2;
    int32_t mod_div, mod_ld;
    float eps;
    int32_t _reserved;      /* 0 */
    float* seg_stats;       /* f32 [M][N2/384][mean, rstd] or NULL (plain second GEMM, N2 % 384 == 0): LayerNorm statistics (eps seg_eps) of every
                             * 384-wide segment of the C2 rows, from the fp32 accumulators - what ina_dit_attn_args.stats consumes */
    float seg_eps;
    int32_t _pad;
} ina_dit_rowchain_args;
int ina_dit_rowchain(const ina_dit_rowchain_args* args, void* stream);

/* ---- dit_attention: the attention stage of one NextDiT block in one launch:
 *          O = SDPA(LN(q1), LN(k1), v1) + tanh(head_gate[h]) * SDPA(LN(q2), K2, V2)
 *      X rows hold the fused projection [q1 | k1 | v1 | q2], each heads*64 wide; LN = LayerNorm over the whole segment
 *      ("layer_norm_across_heads"); self-attention inside each T-token sequence, cross-attention against the Lz condition rows of
 *      env = seq / seq_per_env.  reference: diffusers LuminaAttnProcessor2_0 + LuminaNextDiTBlock gate (diffusers==0.33.1,
 *      requirements/internvla_n1.txt:3) as wired by nextdit_traj.py:121-188.
 *      V2T is the transposed, key-permuted image of the condition V the kernel consumes; a call with V2T_src != NULL (re)builds it
 *      from V2T_src [env][Lz][heads*64] (strides v2_bs / v2_rs) first, and with X == NULL does only that. */
typedef struct ina_dit_attn_args {
    const void* X;          /* bf16 [nseq*T, 4*heads*64], row stride ldx */
    void* O;                /* bf16 [nseq*T, heads*64], row stride ldo */
    const float* g_q1; const float* b_q1;   /* f32 [heads*64] LayerNorm weight / bias of q1, k1, q2 */
    const float* g_k1; const float* b_k1;
    const float* g_q2; const float* b_q2;
    const void* K2;         /* bf16 condition keys: element (env, row, h, d) at env*k2_bs + row*k2_rs + h*64 + d */
    void* V2T;              /* bf16 [envs, heads, 64, 64] */
    const void* V2T_src;    /* bf16 condition values or NULL */
    const float* head_gate; /* f32 [heads] (tanh applied) or NULL */
    int64_t k2_bs, k2_rs, v2_bs, v2_rs;
    int32_t nseq, T, heads, seq_per_env, Lz, ldx, ldo;
    float scale, eps;
    int32_t stats_ld;       /* floats per row of stats (>= 8) */
    const float* stats;     /* f32 [nseq*T][4 segments][mean, rstd] of the X rows as ina_dit_rowchain_args.seg_stats writes them, or NULL:
                             * the kernel then computes the LayerNorm statistics itself (a second pass over three segments) */
} ina_dit_attn_args;
int ina_dit_attention(const ina_dit_attn_args* args, void* stream);

/* ---- diffusion-policy ConditionalUnet1D head (vendored: internnav/model/encoder/diffusion_policy/model/diffusion/conditional_unet1d.py:14-241,
 *      conv1d_components.py:7-40). Activations are channels-last, sequence-padded: row (b, t) of a level = b * (T + 2 pad) + pad + t.
 *      The Conv1d / ConvTranspose1d themselves run on ina_gemm_bf16 over overlapping row windows (implicit GEMM); these three entry
 *      points are what remains: gn_mish = GroupNorm -> Mish [-> FiLM] [-> + residual] of a Conv1dBlock / ConditionalResidualBlock1D,
 *      pad_rows = zero the pad rows after a strided convolution (+ optional bias on the valid rows), ddim_step = DDIMScheduler.step
 *      (diffusers, eta 0, epsilon prediction, clip_sample, use_clipped_model_output 0|1) on the fp32 sample + refresh of the bf16 network input. */
typedef struct ina_gn_mish_args {
    const void* X;          /* bf16 (f32 when x_f32) conv output, row (b, t) at b * in_seq_stride + t, row stride ldx */
    void* Y;                /* bf16 padded output [seqs, T + 2 pad, C], row stride ldy (pad rows are zeroed) */
    const void* R;          /* bf16 residual in the padded indexing of Y, row stride ldr, or NULL */
    const float* gamma; const float* beta;      /* f32 [C] GroupNorm affine */
    const float* film_env;  /* f32 [envs, film_ld]: this block's [scale C | bias C] at column film_off, or NULL */
    const float* film_step; /* f32 [film_ld]: the timestep part, added to film_env */
    int32_t seqs, T, C, groups, pad, in_seq_stride, ldx, ldy, ldr, seq_per_env, film_ld, film_off;
    float eps;
    int32_t x_f32;
} ina_gn_mish_args;
int ina_gn_mish(const ina_gn_mish_args* args, void* stream);

typedef struct ina_pad_rows_args {
    void* X;                /* bf16 [seqs, T + 2 pad, C] */
    const float* bias;      /* f32 [C] added to the valid rows, or NULL */
    int32_t seqs, T, pad, C, ldx, _pad;
} ina_pad_rows_args;
int ina_pad_rows(const ina_pad_rows_args* args, void* stream);

typedef struct ina_ddim_step_args {
    const float* eps;       /* f32 predicted noise in the padded row indexing, row stride lde */
    float* sample;          /* f32 [seqs * T, D], updated in place */
    void* Xin;              /* bf16 padded network input [seqs, T + 2 pad, ldx], channels [0, D) refreshed */
    int32_t seqs, T, D, pad, lde, ldx;
    float inv_sqrt_a, sqrt_b, sqrt_ap, sqrt_bp, clip;   /* 1/sqrt(abar_t), sqrt(1-abar_t), sqrt(abar_prev), sqrt(1-abar_prev), clip range (0 = off) */
    int32_t use_clipped_model_output;   /* diffusers DDIMScheduler.step(use_clipped_model_output=): 0 (the default, what
                                           diffusion_unet_lowdim_policy.py:87-91 runs: step(model_output, t, trajectory, **{})) keeps the
                                           network's eps in the direction term; 1 re-derives eps from the clipped x0 */
} ina_ddim_step_args;
int ina_ddim_step(const ina_ddim_step_args* args, void* stream);

/* ======================================================================================================================
 * SFT step (BASELINE config #5): backward and optimiser kernels. The reference has no FFI here either:
 * these replace torch autograd of InternVLAN1ForCausalLM.forward(labels=...) (internvla_n1.py:222-286) and the HF Trainer's
 * adamw_torch + clip_grad_norm_ (train_dual_system.sh:72-77). Backward GEMMs go through ina_gemm_bf16 on transposed copies.
 * Tensors with a *_dt field are bf16 (0) or f32 (1).
 * ====================================================================================================================== */
#define INA_ACT_TANH_C 6
#define INA_EW_AFFINE 0     /* Y = A * f(S[r / s_div]) + B + tab[r % tab_mod]   (f: 0 s, 1 1+s, 2 tanh s; S, B, tab optional) */
#define INA_EW_ACT_FWD 1    /* Y = act(A) */
#define INA_EW_ACT_BWD 2    /* Y = B * act'(A)            (A = pre-activation, B = dy) */
#define INA_EW_GLU_FWD 3    /* Y = silu(A) * B */
#define INA_EW_GLU_BWD 4    /* Y = D * B * silu'(A), Y2 = D * silu(A)   (D = dy) */
#define INA_EW_DROPOUT 5    /* Y = A * keep / (1 - p): keep iff ina_hash(drop_seed, r * C + c) >= drop_thresh (nn.Dropout, train mode; the same
                             * call on dy is its backward) */
typedef struct ina_ew_args {
    const void* A; const void* B; const void* D; const void* S;
    void* Y; void* Y2;
    const float* tab;       /* f32 [tab_mod, C] or NULL */
    int32_t op, rows, C;
    int32_t a_dt, b_dt, d_dt, s_dt, y_dt, y2_dt;
    int32_t lda, ldb, ldd, lds, ldy, ldy2;
    int32_t s_div, s_f, tab_mod, act, accumulate; /* accumulate: Y += */
    uint32_t drop_seed, drop_thresh;
    float drop_scale;
    const uint32_t* drop_salt; /* optional device word added to drop_seed (see ina_attn_args.drop_salt) */
} ina_ew_args;
int ina_ew(const ina_ew_args* args, void* stream);

/* out[g, c] (+)= scale * sum_{r in group g} X[r, c] * X2[r, c]  (bias / gain / LayerScale / modulation gradients, squared norms).
 * x_cs / x2_cs: column stride of X / X2 (1 = dense, 0 = broadcast one value per row); out_cs: element stride between output columns. */
typedef struct ina_colsum_args {
    const void* X; const void* X2;  /* X2 optional */
    float* out;
    float* partial;         /* f32 scratch [groups * chunks * C] with chunks = ceil(group_rows / chunk), chunk = 32 rows up to 2048 rows per group, 64 up to 4096,
                             * 128 up to 8192, 256 beyond; needed when a group has more than 32 rows */
    int64_t partial_elems;
    int32_t rows, C, group_rows;    /* group_rows 0 = one group of all rows */
    int32_t x_dt, x2_dt, ldx, ldx2, x_cs, x2_cs, ldo, out_cs;
    int32_t accumulate;
    float scale;            /* 0 means 1 */
} ina_colsum_args;
int ina_colsum(const ina_colsum_args* args, void* stream);

/* backward of y = norm(x) * gamma (+ beta), LayerNorm or RMSNorm over the last dim; DX (+)=; XHAT (bf16, optional) for dgamma */
typedef struct ina_norm_bwd_args {
    const void* X; const void* DY; const float* gamma;
    void* DX; void* XHAT;
    int32_t rows, C, x_dt, dy_dt, dx_dt, ldx, lddy, lddx, ldxh, rms, accumulate;
    float eps;
} ina_norm_bwd_args;
int ina_norm_bwd(const ina_norm_bwd_args* args, void* stream);

/* Y[c, r] = bf16(X[r, c]); Y rows are ldy >= rows long (multiple of 8 for the GEMM), the tail is zero-filled */
typedef struct ina_transpose_args {
    const void* X; void* Y;
    int32_t rows, cols, x_dt, ldx, ldy, _pad;
} ina_transpose_args;
int ina_transpose(const ina_transpose_args* args, void* stream);

/* out[t, :] (+)= sum_j coef[t, j] * in[idx[t, j], :]  (idx < 0 = unused tap): DINOv2 bicubic pos-embed interpolation
 * (dinov2.py:180-211) and, with the transposed tap table, its gradient */
typedef struct ina_sparse_rows_args {
    const float* in; float* out; const int32_t* idx; const float* coef;
    int32_t n_out, C, taps, accumulate;
} ina_sparse_rows_args;
int ina_sparse_rows(const ina_sparse_rows_args* args, void* stream);

/* Y[r, n] = sum_k X[r, k] * W[n * w_ns + k * w_ks] + bias[n] + tab[r % tab_mod, n]: nn.Linear(3, 384) / nn.Linear(384, 3)
 * (internvla_n1_arch.py:129-131) forward and input gradient */
typedef struct ina_small_linear_args {
    const void* X; const float* W; const float* bias; const float* tab; void* Y;
    int32_t rows, N, K, x_dt, y_dt, ldx, ldy, w_ns, w_ks, tab_mod;
} ina_small_linear_args;
int ina_small_linear(const ina_small_linear_args* args, void* stream);

/* masked flow-matching MSE of internvla_n1.py:283-286 and its gradient: pred [nseq * T, D] (row stride ldp), mask [nseq] */
typedef struct ina_mse_args {
    const void* pred; const float* target; const float* mask; float* loss; void* dpred;
    int32_t nseq, T, D, pred_dt, dpred_dt, ldp, lddp;
    float loss_scale;
} ina_mse_args;
int ina_mse_masked(const ina_mse_args* args, void* stream);

/* fused AdamW (torch.optim.AdamW update order) on a flat f32 buffer + clip_grad_norm_(max_norm) + 1 / world averaging + bf16 copy */
typedef struct ina_adamw_args {
    float* p; float* g; float* m; float* v;
    void* p_bf16;               /* bf16 [n] working copy or NULL */
    const float* sumsq_parts;   /* f32 [n_parts]: partial sums of g^2 (ina_colsum with X2 = X), or NULL when max_norm == 0 */
    float* norm_out;            /* f32 [1]: the total gradient norm (after grad_scale), or NULL */
    int64_t n;
    int32_t n_parts, zero_grad;
    float lr, beta1, beta2, eps, wd, bc1, bc2, max_norm, grad_scale;   /* bc = 1 - beta^step */
    int32_t _pad;
} ina_adamw_args;
int ina_adamw(const ina_adamw_args* args, void* stream);

/* partial[(split * 4 + w) * MR + m, k] = sum_{n in slice} X[m, n] * W[n, k]  (MR = 8 for M <= 8, else 16): dX of a frozen nn.Linear
 * whose weight W [N, K] stays in its stored layout; reduce the splits * 4 slots with ina_colsum. M <= 16. */
typedef struct ina_gemm_nn_args {
    const void* X; const void* W; float* partial;
    int64_t partial_elems;
    int32_t M, N, K, ldx, ldw, splits;
} ina_gemm_nn_args;
int ina_gemm_nn_bf16(const ina_gemm_nn_args* args, void* stream);

/* dW[n, k] += sum_r DY[r, n] * X[r, k] and, with db, db[n] += sum_r DY[r, n]: weight / bias gradient of nn.Linear from the row-major operands of
 * the backward tape (DY [rows, N] f32 or bf16 - rounded to bf16 for the MFMAs, the bias sum takes the unrounded values; X [rows, K] bf16), one launch
 * instead of two transposes + a GEMM + two column-sum launches (two launches with `splits` row ranges: long reductions over few tiles). N, K, lddy, ldx
 * multiples of 8, ldw of 4. */
typedef struct ina_gemm_dw_args {
    const void* DY; const void* X;
    float* dW;                  /* f32 [N, ldw], accumulated into */
    float* db;                  /* f32 [N], accumulated into, or NULL */
    float* partial;             /* splits > 1: f32 scratch [splits * N * (K + 1)] (per-range tiles, then per-range bias sums) */
    int64_t partial_elems;
    int32_t rows, N, K, dy_dt, lddy, ldx, ldw;
    int32_t splits;             /* <= 1: one launch, every tile walks all rows; 2 .. 64: the rows in that many ranges (grid.z) + a launch that adds them in order */
} ina_gemm_dw_args;
int ina_gemm_dw(const ina_gemm_dw_args* args, void* stream);

/* backward of ina_attention_bf16 (dense layouts only): f describes the forward call (Q, K, V, O and their strides);
 * dO has O's strides. dQ pass writes lse / delta [B, H, Lq] f32, the dK / dV pass (optional) reads them. dK / dV are indexed by the
 * QUERY head (sum the heads of a GQA group afterwards) and hold the key rows [kv_row0, Lk); kv_row0 = -1: the last Lq key rows of every
 * sequence (max(0, k_len - Lq) .. k_len: the query rows' own keys in a cached causal pass; min(Lq, Lk) rows). Every row of dK / dV is stored:
 * dk / dv rows of keys at or past k_len are written as zero. */
typedef struct ina_attn_bwd_args {
    ina_attn_args f;
    const void* dO; void* dQ; void* dK; void* dV;
    float* lse; float* delta;
    int64_t dq_bs, dq_rs, dq_hs, dkv_bs, dkv_rs, dkv_hs;
    int32_t kv_row0;
    int32_t nsplit;         /* > 1: split the keys of the dQ pass over nsplit workgroups per query tile (few query rows, long key axis):
                             * dQ is then accumulated with f32 atomics into dq32 (dense [B, Lq, H, D], zeroed by the caller; dQ is not written) */
    float* part;            /* f32 scratch [B, H, ceil(Lk / 64), 2, Lq] (nsplit > 1): the statistics of every 64-key block */
    float* dq32;
    int32_t stage, _pad;    /* internal (set by the launcher) */
} ina_attn_bwd_args;
int ina_attention_bwd_bf16(const ina_attn_bwd_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INTERNNAV_AMD_H */
