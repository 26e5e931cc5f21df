// Internal launch API of the gfx950 kernels (host side). Everything here takes raw device pointers and an
// explicit hipStream_t; no torch types. The argument structs are the public C-ABI structs (include/internnav_amd.h);
// always value-initialise them (`GemmArgs p{};`) - zero means "absent"/"default" for every field.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/internnav_amd.h"

using GemmArgs = ina_gemm_args;
using AttnArgs = ina_attn_args;
using NormArgs = ina_norm_args;
using PatchifyArgs = ina_patchify_args;
using Embed3Args = ina_embed3_args;
using Head3Args = ina_head3_args;
using SeqpoolArgs = ina_seqpool_args;
using SelectArgs = ina_select_args;
using PoolActArgs = ina_pool_act_args;
using GatherArgs = ina_gather_args;
using RopeArgs = ina_rope_args;
using MropeTableArgs = ina_mrope_table_args;
using ArgmaxArgs = ina_argmax_args;
using DitAttnArgs = ina_dit_attn_args;
using ResizeU8Args = ina_resize_u8_args;
using QwenPatchifyArgs = ina_qwen_patchify_args;
using U8LutArgs = ina_u8_lut_args;
using ResizeF32Args = ina_resize_f32_args;
using DitRowchainArgs = ina_dit_rowchain_args;
using GnMishArgs = ina_gn_mish_args;
using PadRowsArgs = ina_pad_rows_args;
using DdimStepArgs = ina_ddim_step_args;
using EwArgs = ina_ew_args;
using ColsumArgs = ina_colsum_args;
using NormBwdArgs = ina_norm_bwd_args;
using TransposeArgs = ina_transpose_args;
using SparseRowsArgs = ina_sparse_rows_args;
using SmallLinearArgs = ina_small_linear_args;
using MseArgs = ina_mse_args;
using AdamwArgs = ina_adamw_args;
using GemmNnArgs = ina_gemm_nn_args;
using AttnBwdArgs = ina_attn_bwd_args;

int ina_launch_gemm(const GemmArgs& p, hipStream_t stream);
int ina_plan_gemm(const GemmArgs& p_in, GemmArgs& p, int& kernel);   // validation + kernel selection only (no launch)
int ina_launch_gemm_skinny_prenorm(const GemmArgs& p, hipStream_t stream);   // M <= 16 with the input RMSNorm fused in front (gemm_skinny.hip: the bf16 format of gemm_skinny_core.h)
int ina_launch_gemm_glds(const GemmArgs& p, hipStream_t stream, int cfg);  // direct-to-LDS staged large-K path
int ina_launch_gemm_skinny_fused(const GemmArgs& p, hipStream_t stream);  // M <= 64 weight-streaming, workgroup owns its columns for all K, fused epilogue
int ina_launch_gemm_w8(const GemmArgs& p, const void* W8, const int8_t* wexp, hipStream_t stream);   // gemm_skinny_w8.hip: the weight-streaming kernels (gemm_skinny_core.h) on e4m3 weights with a 2^e scale per row
int ina_launch_gemm_mx4(const GemmArgs& p, const void* W4, const void* wscale, hipStream_t stream);   // gemm_skinny_mx4.hip: the weight-streaming kernels (gemm_skinny_core.h) on MXFP4 weights (e2m1 + an e8m0 scale per 32 k)
int ina_launch_gemm_rowpanel(const GemmArgs& p, hipStream_t stream, int cfg);  // gemm_rowpanel.hip: K = 384, register-resident row panels (cfg 34 / 35)
bool ina_gemm_rowpanel_contract(const GemmArgs& p);
bool ina_gemm_w4_contract(const GemmArgs& p);
int ina_launch_gemm_preshuffle(const void* W, void* Wp, int N, int K, long ldw, hipStream_t stream);   // gemm_w4.hip: W -> MFMA fragment order (cfg 40)
int ina_launch_gemm_w4(const GemmArgs& p, hipStream_t stream, int cfg);        // gemm_w4.hip: 256 x 256 tile on four waves of 128 x 128 (cfg 39 / 40)
int ina_launch_attention(const AttnArgs& p, hipStream_t stream);
bool ina_attention_wide_eligible(const AttnArgs& p);                   // attention_wide.hip: long dense shapes (32 query rows per wave) - the automatic rule
bool ina_attention_wide_contract(const AttnArgs& p);                   // what that kernel can run at all
int ina_launch_attention_wide(const AttnArgs& p, hipStream_t stream);
int ina_launch_norm(const NormArgs& p, hipStream_t stream);
int ina_launch_patchify(const PatchifyArgs& p, hipStream_t stream);
int ina_launch_embed3(const Embed3Args& p, hipStream_t stream);
int ina_launch_goal_slots(void* Y, int ldy, int y_dtype, int L, int slot0, int nslots, const float* P, int B, int D, const int32_t* kind,
                          const int32_t* row, float* embed, const float* point, int n_point, const float* point_w, const float* point_b,
                          const float* image_tok, int n_image, const float* image_w, const float* image_b, const float* pixel_tok,
                          int n_pixel, const float* pixel_w, const float* pixel_b, int ntok, int E, hipStream_t stream);   // goal_slots.hip
int ina_launch_kv_copy(int to_engine, const int64_t* layer_base, int n_layers, const int64_t* seq, int n_seq, long engine_rows, long row_bytes,
                       long max_rows, hipStream_t stream);                                                                   // kv_copy.hip
int ina_launch_attention_prefix(const void* Q, long q_ps, long q_rs, long q_hs, void* O, long o_ps, long o_rs, long o_hs, const void* Kc,
                                const void* Vc, long c_ss, long c_rs, long c_hs, int n_slots, const void* Ks, const void* Vs, long s_ps, long s_rs,
                                long s_hs, const int32_t* slot, const int32_t* pfx_len, const int32_t* suf_len, int P, int m, int H, int Hkv, int D,
                                int max_pfx, float scale, hipStream_t stream);                                               // attention_prefix.hip
int ina_launch_attention_prefix_tail(const void* Q, long q_ps, long q_rs, long q_hs, void* O, long o_ps, long o_rs, long o_hs, const void* Kc,
                                     const void* Vc, long c_ss, long c_rs, long c_hs, int n_slots, const void* Kt, const void* Vt, long t_ps,
                                     long t_rs, long t_hs, int n_tail_rows, const void* Ks, const void* Vs, long s_ps, long s_rs, long s_hs,
                                     const int32_t* slot, const int32_t* pfx_len, const int32_t* tail_row, const int32_t* tail_len,
                                     const int32_t* suf_len, int P, int m, int H, int Hkv, int D, int max_pfx, int max_tail, float scale,
                                     hipStream_t stream);                                                                    // attention_prefix.hip
int ina_launch_attention_shared(const void* Q, long q_rs, long q_hs, void* O, long o_rs, long o_hs, const void* Kc, const void* Vc, long c_ss,
                                long c_rs, long c_hs, int n_slots, const void* Kt, const void* Vt, long t_ps, long t_rs, long t_hs, int T,
                                const int32_t* tile_rows, const int32_t* tile_slot, const int32_t* tile_pfx, const int32_t* tail_len, int n_tiles,
                                int n_rows, int H, int Hkv, int D, int max_pfx, float scale, hipStream_t stream);            // attention_shared.hip
int ina_launch_memory_gather(void* out, long out_env_stride, float* ring, const float* fresh, const float* blank, const float* pe,
                             const int32_t* env, const int32_t* head, const int32_t* count, int n, int max_envs, int M, int ntok, int C, int depth,
                             int stride, hipStream_t stream);                                                                // memory_gather.hip
int ina_launch_traj_actions(void* traj, int traj_dtype, int B, int S, int T, int32_t* actions, int max_actions, int32_t* count, double* traj_out,
                            int scale_in_place, hipStream_t stream);                                                         // traj_actions.hip
int ina_launch_token_seen_set(uint32_t* seen, int ld_words, const int32_t* ids, int ld_ids, const int32_t* lens, int rows, int n,
                              hipStream_t stream);                                                                           // decode_penalty.hip
int ina_launch_argmax_penalty(const float* X, int ldx, int rows, int n, uint32_t* seen, int ld_words, float penalty, int mark, int32_t* out,
                              hipStream_t stream);                                                                           // decode_penalty.hip
int ina_launch_logprob(const float* X, int ldx, int rows, int n, uint32_t* seen, int ld_words, float penalty, int mark, const int32_t* target,
                       int32_t* tok, float* logprob, float* margin, hipStream_t stream);                                     // decode_logprob.hip
int ina_launch_sample(const float* X, int ldx, int x_rows, int rows, int n, uint32_t* seen, int ld_words, float penalty, int mark, float temperature,
                      int top_k, float top_p, const float* u, const int32_t* src, int32_t* tok, float* logprob, int32_t* n_kept, float* thr,
                      hipStream_t stream);                                                                                   // decode_sample.hip
int ina_launch_automaton_mask(float* X, int ldx, int rows, int n, const uint8_t* token_class, int vocab, const uint32_t* allow, const uint8_t* next,
                              int n_states, const int32_t* state_in, const int32_t* prev_tok, int32_t* state_out, hipStream_t stream);   // decode_constrain.hip
int ina_launch_logit_rules(float* X, int ldx, int rows, int n, int col, int32_t* hist, int ld_hist, int hist_cap, const int32_t* len0,
                           const int32_t* prev_tok, int ngram, const int32_t* grp_tok, const float* grp_base, const int32_t* grp_ptr, int n_bias, int n_groups,
                           const int32_t* seq_ptr, const int32_t* seq_ids, const float* seq_bias, int n_seqs, int n_ids, const int32_t* ban_tok, int n_ban,
                           const int32_t* begin_tok, int n_begin, const int32_t* eos_tok, int n_eos, const int32_t* eos_first, const int32_t* forced_tok,
                           int n_forced, int forced_col, hipStream_t stream);                                                 // decode_rules.hip
int ina_launch_beam_topm(const float* X, int ldx, int x_rows, int rows, int n, const uint32_t* seen, int ld_words, float penalty, const float* run_score,
                         const int32_t* src, int M, float* cand_score, int32_t* cand_tok, hipStream_t stream);                 // decode_beam.hip
int ina_launch_beam_step(const float* cand_score, const int32_t* cand_tok, int B, int K, int M, int T, int step, int max_new, float lenpow, float hyppow,
                         int early, const int32_t* eos, int n_eos, float* run_score, int32_t* next_tok, int32_t* parent, const int32_t* hist_in,
                         int32_t* hist_out, const float* ts_in, float* ts_out, int32_t* fin_tok, float* fin_ts, float* fin_score, int32_t* fin_len,
                         int32_t* fin_flag, int32_t* heur, int32_t* done, hipStream_t stream);
int ina_launch_beam_reorder(const int64_t* src_base, const int64_t* dst_base, int n_layers, const int32_t* parent, int rows, int T, int t, long row_bytes,
                            const uint32_t* seen_src, uint32_t* seen_dst, int ld_words, const int32_t* next_tok, int n, const int32_t* state_src,
                            int32_t* state_dst, hipStream_t stream);
int ina_launch_head3(const Head3Args& p, hipStream_t stream);
int ina_launch_seqpool(const SeqpoolArgs& p, hipStream_t stream);
int ina_launch_select(const SelectArgs& p, hipStream_t stream);
int ina_launch_pool_act(const PoolActArgs& p, hipStream_t stream);
int ina_launch_gather(const GatherArgs& p, hipStream_t stream);
int ina_launch_rope(const RopeArgs& p, hipStream_t stream);
int ina_launch_mrope_table(const MropeTableArgs& p, hipStream_t stream);
int ina_launch_argmax(const ArgmaxArgs& p, hipStream_t stream);
int ina_launch_resize_u8(const ResizeU8Args& p, hipStream_t stream);            // one axis of PIL's 8-bit bicubic resample
int ina_launch_qwen_patchify_u8(const QwenPatchifyArgs& p, hipStream_t stream);  // HF Qwen2-VL rescale + normalize + patchify from bytes
int ina_launch_u8_lut(const U8LutArgs& p, hipStream_t stream);
int ina_launch_resize_f32(const ResizeF32Args& p, hipStream_t stream);          // one axis of PIL's float ("F" mode) bicubic resample
int ina_launch_dit_attention(const DitAttnArgs& p, hipStream_t stream);  // q/k-LayerNorm + self-attention + gated cross-attention of a NextDiT block
int ina_launch_dit_rowchain(const DitRowchainArgs& p, hipStream_t stream);  // GEMM + gated rmsnorm + residual + next pre-norm + next GEMM of a NextDiT block, one launch
int ina_launch_gn_mish(const GnMishArgs& p, hipStream_t stream);      // GroupNorm + Mish (+ FiLM, + residual) of a ConditionalUnet1D block
int ina_launch_pad_rows(const PadRowsArgs& p, hipStream_t stream);
int ina_launch_ddim_step(const DdimStepArgs& p, hipStream_t stream);
// SFT step (train.hip, attention_bwd.hip)
int ina_launch_ew(const EwArgs& p, hipStream_t stream);
int ina_launch_colsum(const ColsumArgs& p, hipStream_t stream);
int ina_launch_norm_bwd(const NormBwdArgs& p, hipStream_t stream);
int ina_launch_transpose(const TransposeArgs& p, hipStream_t stream);
int ina_launch_sparse_rows(const SparseRowsArgs& p, hipStream_t stream);
int ina_launch_small_linear(const SmallLinearArgs& p, hipStream_t stream);
int ina_launch_mse(const MseArgs& p, hipStream_t stream);
int ina_launch_adamw(const AdamwArgs& p, hipStream_t stream);
int ina_launch_gemm_nn(const GemmNnArgs& p, hipStream_t stream);
int ina_launch_gemm_dw(const ina_gemm_dw_args& p, hipStream_t stream);
int ina_launch_attention_bwd(const AttnBwdArgs& p, hipStream_t stream);
