// extern "C" entry points of libinternnav_amd.so (declared in include/internnav_amd.h).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <cmath>

#include "common.h"
#include "kernels.h"

static thread_local char g_err[1024] = "";

void ina_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- per-launch event timing -----------------------------------------------------------------------------------
#include <mutex>
#include <vector>
namespace {
struct ProfRec { int kind, sub; hipEvent_t a, b; double flops, bytes; };
thread_local int g_prof_sub = 0;
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::mutex g_prof_mu;
}  // namespace

InaProfScope::InaProfScope(int kind, double flops, double bytes, hipStream_t s) : idx(-1), stream(s) {
    if (!g_prof_on) return;
    ProfRec r{kind, g_prof_sub, nullptr, nullptr, flops, bytes};
    g_prof_sub = 0;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    (void)hipEventRecord(r.a, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(r);
    idx = (int)g_prof.size() - 1;
}
void ina_prof_set_sub(int sub) { g_prof_sub = sub; }

InaProfScope::~InaProfScope() {
    if (idx < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    (void)hipEventRecord(g_prof[idx].b, stream);
}

// ---- workspace slots -----------------------------------------------------------------------------------------------
// The scratch pointer is baked into every graph captured under a slot, so a buffer that a graph has seen is NEVER freed: when a
// later (eager) launch needs more, a new buffer is allocated for new launches and the old one is retired but kept alive until the
// process ends (graphs captured earlier keep replaying into it). The current slot is per host thread, like the error string.
namespace {
thread_local int g_ws_slot = 0;
float* g_ws_ptr[INA_WS_KINDS][INA_WS_SLOTS] = {};
size_t g_ws_cap[INA_WS_KINDS][INA_WS_SLOTS] = {};
bool g_ws_captured[INA_WS_KINDS][INA_WS_SLOTS] = {};
std::vector<float*> g_ws_retired;
std::mutex g_ws_mu;
}  // namespace

int ina_workspace(int kind, size_t bytes, hipStream_t stream, float** out) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    const int slot = g_ws_slot;
    float*& ptr = g_ws_ptr[kind][slot];
    size_t& cap = g_ws_cap[kind][slot];
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &st);
    if (bytes > cap) {
        INA_REQUIRE(st == hipStreamCaptureStatusNone,
                    "workspace (kind %d, slot %d) of %zu bytes needed during graph capture: run the shape once eagerly under this slot first", kind,
                    slot, bytes);
        if (ptr) {
            if (g_ws_captured[kind][slot]) {
                g_ws_retired.push_back(ptr);              // a captured graph still points here: keep the memory alive
            } else {
                INA_HIP_CHECK(hipDeviceSynchronize());
                INA_HIP_CHECK(hipFree(ptr));
            }
            ptr = nullptr;
            cap = 0;
        }
        const size_t want = bytes < (size_t)(32u << 20) ? (size_t)(32u << 20) : bytes * 2;
        INA_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ptr), want));
        cap = want;
        g_ws_captured[kind][slot] = false;
    }
    if (st != hipStreamCaptureStatusNone) g_ws_captured[kind][slot] = true;
    *out = ptr;
    return 0;
}

extern "C" {

int ina_workspace_retired(void) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    return (int)g_ws_retired.size();
}

int ina_set_workspace_slot(int slot) {
    INA_REQUIRE(slot >= 0 && slot < INA_WS_SLOTS, "workspace slot %d out of range [0, %d)", slot, INA_WS_SLOTS);
    g_ws_slot = slot;
    return 0;
}

int ina_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof.clear();
    g_prof_on = on != 0;
    return 0;
}

static int prof_read_impl(int kind, int sub, double* ms_total, int64_t* launches, double* flops, double* bytes) {
    INA_REQUIRE(kind >= 0 && kind < INA_PROF_KINDS, "prof_read: bad kind %d", kind);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    double ms = 0, fl = 0, by = 0;
    int64_t n = 0;
    for (auto& r : g_prof) {
        if (r.kind != kind || (sub >= 0 && r.sub != sub)) continue;
        INA_HIP_CHECK(hipEventSynchronize(r.b));
        float t = 0.f;
        INA_HIP_CHECK(hipEventElapsedTime(&t, r.a, r.b));
        ms += t; fl += r.flops; by += r.bytes; ++n;
    }
    if (ms_total) *ms_total = ms;
    if (launches) *launches = n;
    if (flops) *flops = fl;
    if (bytes) *bytes = by;
    return 0;
}

int ina_prof_read(int kind, double* ms_total, int64_t* launches, double* flops, double* bytes) {
    return prof_read_impl(kind, -1, ms_total, launches, flops, bytes);
}

int ina_prof_read_sub(int kind, int sub, double* ms_total, int64_t* launches, double* flops, double* bytes) {
    return prof_read_impl(kind, sub, ms_total, launches, flops, bytes);
}

int ina_abi_version(void) { return INA_ABI_VERSION; }

const char* ina_last_error(void) { return g_err; }

int ina_device_check(char* name, int n) {
    int dev = 0;
    INA_HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    INA_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (name && n > 0) {
        strncpy(name, prop.gcnArchName, (size_t)n - 1);
        name[n - 1] = 0;
    }
    INA_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, "internnav_amd is built for gfx950 only, device is %s", prop.gcnArchName);
    return 0;
}

int ina_gemm_bf16(const ina_gemm_args* args, void* stream) {
    INA_REQUIRE(args != nullptr, "gemm: null args");
    return ina_launch_gemm(*args, reinterpret_cast<hipStream_t>(stream));
}

int ina_gemm_w8(const ina_gemm_args* args, const void* W8, const int8_t* wexp, void* stream) {
    INA_REQUIRE(args != nullptr, "gemm_w8: null args");
    return ina_launch_gemm_w8(*args, W8, wexp, reinterpret_cast<hipStream_t>(stream));
}

int ina_gemm_mx4(const ina_gemm_args* args, const void* W4, const void* wscale, void* stream) {
    INA_REQUIRE(args != nullptr, "gemm_mx4: null args");
    return ina_launch_gemm_mx4(*args, W4, wscale, reinterpret_cast<hipStream_t>(stream));
}

int ina_gemm_preshuffle(const void* W, void* Wp, int32_t N, int32_t K, int64_t ldw, void* stream) {
    return ina_launch_gemm_preshuffle(W, Wp, N, K, (long)ldw, reinterpret_cast<hipStream_t>(stream));
}

int ina_goal_slots(void* Y, int32_t ldy, int32_t y_dtype, int32_t L, int32_t slot0, int32_t nslots, const float* P, int32_t B, int32_t D,
                   const int32_t* kind, const int32_t* row, float* embed, const float* point, int32_t n_point, const float* point_w,
                   const float* point_b, const float* image_tok, int32_t n_image, const float* image_w, const float* image_b,
                   const float* pixel_tok, int32_t n_pixel, const float* pixel_w, const float* pixel_b, int32_t ntok, int32_t E, void* stream) {
    return ina_launch_goal_slots(Y, ldy, y_dtype, L, slot0, nslots, P, B, D, kind, row, embed, point, n_point, point_w, point_b, image_tok, n_image,
                                 image_w, image_b, pixel_tok, n_pixel, pixel_w, pixel_b, ntok, E, reinterpret_cast<hipStream_t>(stream));
}

int ina_kv_copy(int32_t to_engine, const int64_t* layer_base, int32_t n_layers, const int64_t* seq, int32_t n_seq, int64_t engine_rows,
                int64_t row_bytes, int64_t max_rows, void* stream) {
    return ina_launch_kv_copy(to_engine, layer_base, n_layers, seq, n_seq, (long)engine_rows, (long)row_bytes, (long)max_rows,
                              reinterpret_cast<hipStream_t>(stream));
}

int ina_attention_prefix(const void* Q, int64_t q_ps, int64_t q_rs, int64_t q_hs, void* O, int64_t o_ps, int64_t o_rs, int64_t o_hs,
                         const void* k_cache, const void* v_cache, int64_t c_ss, int64_t c_rs, int64_t c_hs, int32_t n_slots, const void* k_suf,
                         const void* v_suf, int64_t s_ps, int64_t s_rs, int64_t s_hs, const int32_t* slot, const int32_t* pfx_len,
                         const int32_t* suf_len, int32_t P, int32_t m, int32_t H, int32_t Hkv, int32_t D, int32_t max_pfx, float scale, void* stream) {
    return ina_launch_attention_prefix(Q, (long)q_ps, (long)q_rs, (long)q_hs, O, (long)o_ps, (long)o_rs, (long)o_hs, k_cache, v_cache, (long)c_ss,
                                       (long)c_rs, (long)c_hs, n_slots, k_suf, v_suf, (long)s_ps, (long)s_rs, (long)s_hs, slot, pfx_len, suf_len, P, m,
                                       H, Hkv, D, max_pfx, scale, reinterpret_cast<hipStream_t>(stream));
}

int ina_attention_prefix_tail(const void* Q, int64_t q_ps, int64_t q_rs, int64_t q_hs, void* O, int64_t o_ps, int64_t o_rs, int64_t o_hs,
                              const void* k_cache, const void* v_cache, int64_t c_ss, int64_t c_rs, int64_t c_hs, int32_t n_slots, const void* k_tail,
                              const void* v_tail, int64_t t_ps, int64_t t_rs, int64_t t_hs, int32_t n_tail_rows, const void* k_suf, const void* v_suf,
                              int64_t s_ps, int64_t s_rs, int64_t s_hs, const int32_t* slot, const int32_t* pfx_len, const int32_t* tail_row,
                              const int32_t* tail_len, const int32_t* suf_len, int32_t P, int32_t m, int32_t H, int32_t Hkv, int32_t D,
                              int32_t max_pfx, int32_t max_tail, float scale, void* stream) {
    return ina_launch_attention_prefix_tail(Q, (long)q_ps, (long)q_rs, (long)q_hs, O, (long)o_ps, (long)o_rs, (long)o_hs, k_cache, v_cache, (long)c_ss,
                                            (long)c_rs, (long)c_hs, n_slots, k_tail, v_tail, (long)t_ps, (long)t_rs, (long)t_hs, n_tail_rows, k_suf,
                                            v_suf, (long)s_ps, (long)s_rs, (long)s_hs, slot, pfx_len, tail_row, tail_len, suf_len, P, m, H, Hkv, D,
                                            max_pfx, max_tail, scale, reinterpret_cast<hipStream_t>(stream));
}

int ina_attention_shared(const void* Q, int64_t q_rs, int64_t q_hs, void* O, int64_t o_rs, int64_t o_hs, const void* k_cache, const void* v_cache,
                         int64_t c_ss, int64_t c_rs, int64_t c_hs, int32_t n_slots, const void* k_tail, const void* v_tail, int64_t t_ps, int64_t t_rs,
                         int64_t t_hs, int32_t T, const int32_t* tile_rows, const int32_t* tile_slot, const int32_t* tile_pfx, const int32_t* tail_len,
                         int32_t n_tiles, int32_t n_rows, int32_t H, int32_t Hkv, int32_t D, int32_t max_pfx, float scale, void* stream) {
    return ina_launch_attention_shared(Q, (long)q_rs, (long)q_hs, O, (long)o_rs, (long)o_hs, k_cache, v_cache, (long)c_ss, (long)c_rs, (long)c_hs,
                                       n_slots, k_tail, v_tail, (long)t_ps, (long)t_rs, (long)t_hs, T, tile_rows, tile_slot, tile_pfx, tail_len,
                                       n_tiles, n_rows, H, Hkv, D, max_pfx, scale, reinterpret_cast<hipStream_t>(stream));
}

int ina_memory_gather(void* out, int64_t out_env_stride, float* ring, const float* fresh, const float* blank, const float* pe, const int32_t* env,
                      const int32_t* head, const int32_t* count, int32_t n, int32_t max_envs, int32_t M, int32_t ntok, int32_t C, int32_t depth,
                      int32_t stride, void* stream) {
    return ina_launch_memory_gather(out, (long)out_env_stride, ring, fresh, blank, pe, env, head, count, n, max_envs, M, ntok, C, depth, stride,
                                    reinterpret_cast<hipStream_t>(stream));
}

int ina_traj_actions(void* traj, int32_t traj_dtype, int32_t B, int32_t S, int32_t T, int32_t* actions, int32_t max_actions, int32_t* count,
                     double* traj_out, int32_t scale_in_place, void* stream) {
    return ina_launch_traj_actions(traj, traj_dtype, B, S, T, actions, max_actions, count, traj_out, scale_in_place, reinterpret_cast<hipStream_t>(stream));
}

int ina_token_seen_set(uint32_t* seen, int32_t ld_words, const int32_t* ids, int32_t ld_ids, const int32_t* lens, int32_t rows, int32_t n, void* stream) {
    return ina_launch_token_seen_set(seen, ld_words, ids, ld_ids, lens, rows, n, reinterpret_cast<hipStream_t>(stream));
}

int ina_argmax_penalty_rows(const float* X, int32_t ldx, int32_t rows, int32_t n, uint32_t* seen, int32_t ld_words, float penalty, int32_t mark,
                            int32_t* out, void* stream) {
    return ina_launch_argmax_penalty(X, ldx, rows, n, seen, ld_words, penalty, mark, out, reinterpret_cast<hipStream_t>(stream));
}

int ina_automaton_mask_rows(float* X, int32_t ldx, int32_t rows, int32_t n, const uint8_t* token_class, int32_t vocab, const uint32_t* allow,
                            const uint8_t* next, int32_t n_states, const int32_t* state_in, const int32_t* prev_tok, int32_t* state_out, void* stream) {
    return ina_launch_automaton_mask(X, ldx, rows, n, token_class, vocab, allow, next, n_states, state_in, prev_tok, state_out,
                                     reinterpret_cast<hipStream_t>(stream));
}

int ina_logit_rules_rows(float* X, int32_t ldx, int32_t rows, int32_t n, int32_t col, int32_t* hist, int32_t ld_hist, int32_t hist_cap, const int32_t* len0,
                         const int32_t* prev_tok, int32_t ngram, const int32_t* grp_tok, const float* grp_base, const int32_t* grp_ptr, int32_t n_bias,
                         int32_t n_groups, const int32_t* seq_ptr, const int32_t* seq_ids, const float* seq_bias, int32_t n_seqs, int32_t n_ids,
                         const int32_t* ban_tok, int32_t n_ban, const int32_t* begin_tok, int32_t n_begin, const int32_t* eos_tok, int32_t n_eos,
                         const int32_t* eos_first, const int32_t* forced_tok, int32_t n_forced, int32_t forced_col, void* stream) {
    return ina_launch_logit_rules(X, ldx, rows, n, col, hist, ld_hist, hist_cap, len0, prev_tok, ngram, grp_tok, grp_base, grp_ptr, n_bias, n_groups, seq_ptr,
                                  seq_ids, seq_bias, n_seqs, n_ids, ban_tok, n_ban, begin_tok, n_begin, eos_tok, n_eos, eos_first, forced_tok, n_forced,
                                  forced_col, reinterpret_cast<hipStream_t>(stream));
}

int ina_logprob_rows(const float* X, int32_t ldx, int32_t rows, int32_t n, uint32_t* seen, int32_t ld_words, float penalty, int32_t mark,
                     const int32_t* target, int32_t* tok, float* logprob, float* margin, void* stream) {
    INA_REQUIRE(X && tok && logprob, "logprob_rows: X, tok and logprob required");
    INA_REQUIRE(rows >= 0 && n >= 1 && ldx >= n, "logprob_rows: bad arguments rows=%d n=%d ldx=%d (rows >= 0, n >= 1, ldx >= n)", rows, n, ldx);
    if (seen) {
        INA_REQUIRE((long)ld_words * 32 >= (long)n, "logprob_rows: ld_words=%d holds fewer than n=%d bits", ld_words, n);
        INA_REQUIRE(std::isfinite(penalty) && penalty > 0.f, "logprob_rows: repetition penalty %g is not a strictly positive finite float", (double)penalty);
    }
    INA_REQUIRE(!mark || (seen && !target), "logprob_rows: mark needs a seen set and is refused with a target (teacher forcing selects nothing)");
    if (rows == 0) return 0;
    return ina_launch_logprob(X, ldx, rows, n, seen, ld_words, penalty, mark, target, tok, logprob, margin, reinterpret_cast<hipStream_t>(stream));
}

int ina_beam_topm_rows(const float* X, int32_t ldx, int32_t x_rows, int32_t rows, int32_t n, const uint32_t* seen, int32_t ld_words, float penalty,
                       const float* run_score, const int32_t* src, int32_t M, float* cand_score, int32_t* cand_tok, void* stream) {
    INA_REQUIRE(X && run_score && cand_score && cand_tok, "beam_topm_rows: X, run_score, cand_score and cand_tok required");
    INA_REQUIRE(rows >= 0 && rows <= 65535 && x_rows >= 1 && n >= 1 && ldx >= n,
                "beam_topm_rows: bad arguments rows=%d x_rows=%d n=%d ldx=%d (0 <= rows <= 65535, x_rows >= 1, n >= 1, ldx >= n)", rows, x_rows, n, ldx);
    INA_REQUIRE(src || rows <= x_rows, "beam_topm_rows: rows=%d output rows of x_rows=%d logits rows need a src table", rows, x_rows);
    INA_REQUIRE(M >= 2 && M <= 32 && M <= n, "beam_topm_rows: M=%d candidates per row outside [2, min(32, n=%d)]", M, n);
    if (seen) {
        INA_REQUIRE((long)ld_words * 32 >= (long)n, "beam_topm_rows: ld_words=%d holds fewer than n=%d bits", ld_words, n);
        INA_REQUIRE(std::isfinite(penalty) && penalty > 0.f, "beam_topm_rows: repetition penalty %g is not a strictly positive finite float", (double)penalty);
    }
    if (rows == 0) return 0;
    return ina_launch_beam_topm(X, ldx, x_rows, rows, n, seen, ld_words, penalty, run_score, src, M, cand_score, cand_tok,
                                reinterpret_cast<hipStream_t>(stream));
}

int ina_beam_step(const float* cand_score, const int32_t* cand_tok, int32_t B, int32_t K, int32_t M, int32_t T, int32_t step, int32_t max_new_tokens,
                  float length_penalty, int32_t early_stopping, const int32_t* eos, int32_t n_eos, float* run_score, int32_t* next_tok, int32_t* parent,
                  const int32_t* hist_in, int32_t* hist_out, const float* ts_in, float* ts_out, int32_t* fin_tok, float* fin_ts, float* fin_score,
                  int32_t* fin_len, int32_t* fin_flag, int32_t* heur, int32_t* done, void* stream) {
    INA_REQUIRE(cand_score && cand_tok && run_score && next_tok && parent && hist_in && hist_out && ts_in && ts_out && fin_tok && fin_ts && fin_score &&
                    fin_len && fin_flag && heur && done, "beam_step: every buffer but eos is required");
    INA_REQUIRE(B >= 0 && B <= 65535 && K >= 1 && K <= 8 && M >= 2 && M >= K && M <= 32,
                "beam_step: bad arguments B=%d K=%d M=%d (0 <= B <= 65535, 1 <= K <= 8, max(2, K) <= M <= 32)", B, K, M);
    INA_REQUIRE(max_new_tokens >= 1 && max_new_tokens <= T && step >= 0 && step < max_new_tokens,
                "beam_step: step=%d max_new_tokens=%d T=%d (0 <= step < max_new_tokens <= T)", step, max_new_tokens, T);
    INA_REQUIRE(n_eos >= 0 && n_eos <= 8 && (n_eos == 0 || eos), "beam_step: n_eos=%d outside [0, 8], or no table", n_eos);
    INA_REQUIRE(std::isfinite(length_penalty), "beam_step: length_penalty %g is not finite", (double)length_penalty);
    INA_REQUIRE(early_stopping >= 0 && early_stopping <= 2, "beam_step: early_stopping mode %d (0 False, 1 True, 2 never)", early_stopping);
    INA_REQUIRE(hist_in != hist_out && ts_in != ts_out, "beam_step: the histories are read from one buffer of a pair and written to the other");
    if (B == 0) return 0;
    // HF's python-float powers, rounded to fp32 once: the answer length of this step, and the heuristic's hypothetical length
    const double L = (double)(step + 1), H = (early_stopping == 2 && length_penalty > 0.f) ? (double)max_new_tokens : L;
    const float lenpow = (float)std::pow(L, (double)length_penalty), hyppow = (float)std::pow(H, (double)length_penalty);
    return ina_launch_beam_step(cand_score, cand_tok, B, K, M, T, step, max_new_tokens, lenpow, hyppow, early_stopping, eos, n_eos, run_score, next_tok,
                                parent, hist_in, hist_out, ts_in, ts_out, fin_tok, fin_ts, fin_score, fin_len, fin_flag, heur, done,
                                reinterpret_cast<hipStream_t>(stream));
}

int ina_beam_reorder(const int64_t* src_base, const int64_t* dst_base, int32_t n_layers, const int32_t* parent, int32_t rows, int32_t T, int32_t t,
                     int64_t row_bytes, const uint32_t* seen_src, uint32_t* seen_dst, int32_t ld_words, const int32_t* next_tok, int32_t n,
                     const int32_t* state_src, int32_t* state_dst, void* stream) {
    INA_REQUIRE(parent && rows >= 0 && rows <= 65535 && n_layers >= 0 && n_layers < 65535, "beam_reorder: parent required, rows=%d layers=%d", rows, n_layers);
    INA_REQUIRE(n_layers == 0 || (src_base && dst_base && src_base != dst_base), "beam_reorder: two distinct layer base tables required");
    INA_REQUIRE(T >= 1 && t >= 0 && t <= T, "beam_reorder: t=%d tail rows of T=%d", t, T);
    INA_REQUIRE(n_layers == 0 || (row_bytes > 0 && row_bytes % 16 == 0), "beam_reorder: row_bytes=%ld must be a positive multiple of 16", (long)row_bytes);
    INA_REQUIRE((!seen_src && !seen_dst) || (seen_src && seen_dst && seen_src != seen_dst), "beam_reorder: the seen sets are two distinct buffers, or both NULL");
    INA_REQUIRE(!seen_src || (next_tok && ld_words >= 1 && n >= 1 && (long)ld_words * 32 >= (long)n),
                "beam_reorder: the seen gather needs next_tok and ld_words=%d * 32 >= n=%d", ld_words, n);
    INA_REQUIRE((!state_src && !state_dst) || (state_src && state_dst && state_src != state_dst), "beam_reorder: the automaton states are two distinct buffers, or both NULL");
    if (rows == 0) return 0;
    return ina_launch_beam_reorder(src_base, dst_base, n_layers, parent, rows, T, t, (long)row_bytes, seen_src, seen_dst, ld_words, next_tok, n, state_src,
                                   state_dst, reinterpret_cast<hipStream_t>(stream));
}

int ina_sample_rows(const float* X, int32_t ldx, int32_t x_rows, int32_t rows, int32_t n, uint32_t* seen, int32_t ld_words, float penalty, int32_t mark,
                    float temperature, int32_t top_k, float top_p, const float* u, const int32_t* src, int32_t* tok, float* logprob, int32_t* n_kept,
                    float* thr, void* stream) {
    INA_REQUIRE(X && tok && logprob && u, "sample_rows: X, tok, logprob and u required");
    INA_REQUIRE(rows >= 0 && x_rows >= 1 && n >= 1 && ldx >= n, "sample_rows: bad arguments rows=%d x_rows=%d n=%d ldx=%d (rows >= 0, x_rows >= 1, n >= 1, ldx >= n)",
                rows, x_rows, n, ldx);
    INA_REQUIRE(src || rows <= x_rows, "sample_rows: rows=%d output rows of x_rows=%d logits rows need a src table", rows, x_rows);
    INA_REQUIRE(n <= 262144, "sample_rows: a vocabulary of %d tokens exceeds 262144 (the fixed-point mass sum and the seen bitmap)", n);
    INA_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "sample_rows: temperature %g is not a strictly positive finite float", (double)temperature);
    INA_REQUIRE(top_k >= 0, "sample_rows: top_k=%d is negative (0 switches top-k off)", top_k);
    INA_REQUIRE(top_p > 0.f && top_p <= 1.f, "sample_rows: top_p=%g is outside (0, 1] (1 switches top-p off)", (double)top_p);
    if (seen) {
        INA_REQUIRE((long)ld_words * 32 >= (long)n, "sample_rows: ld_words=%d holds fewer than n=%d bits", ld_words, n);
        INA_REQUIRE(std::isfinite(penalty) && penalty > 0.f, "sample_rows: repetition penalty %g is not a strictly positive finite float", (double)penalty);
    }
    INA_REQUIRE(!mark || seen, "sample_rows: mark needs a seen set");
    if (rows == 0) return 0;
    return ina_launch_sample(X, ldx, x_rows, rows, n, seen, ld_words, penalty, mark, temperature, top_k, top_p, u, src, tok, logprob, n_kept, thr,
                             reinterpret_cast<hipStream_t>(stream));
}

int ina_gemm_select(const ina_gemm_args* args, int* kernel) {
    INA_REQUIRE(args != nullptr && kernel != nullptr, "gemm_select: null argument");
    GemmArgs p;
    return ina_plan_gemm(*args, p, *kernel);
}

int ina_attention_bf16(const ina_attn_args* args, void* stream) {
    INA_REQUIRE(args != nullptr, "attention: null args");
    return ina_launch_attention(*args, reinterpret_cast<hipStream_t>(stream));
}

int ina_norm_bf16(const ina_norm_args* args, void* stream) {
    INA_REQUIRE(args != nullptr, "norm: null args");
    return ina_launch_norm(*args, reinterpret_cast<hipStream_t>(stream));
}

/* sizeof() of the k-th argument struct (layout check of the ctypes mirrors): 0 gemm, 1 attn, 2 norm, 3 patchify, 4 embed3, 5 head3, 6 seqpool, 7 select, 8 pool_act, 9 gather, 10 rope, 11 mrope_table, 12 argmax, 13 dit_attn, 14 resize_u8, 15 qwen_patchify, 16 u8_lut, 17 resize_f32, 18 gn_mish, 19 pad_rows, 20 ddim_step, 21 ew, 22 colsum, 23 norm_bwd, 24 transpose, 25 sparse_rows, 26 small_linear, 27 mse, 28 adamw, 29 gemm_nn, 30 attn_bwd, 31 dit_rowchain, 32 gemm_dw */
int ina_struct_size(int k) {
    switch (k) {
        case 0: return (int)sizeof(ina_gemm_args);
        case 1: return (int)sizeof(ina_attn_args);
        case 2: return (int)sizeof(ina_norm_args);
        case 3: return (int)sizeof(ina_patchify_args);
        case 4: return (int)sizeof(ina_embed3_args);
        case 5: return (int)sizeof(ina_head3_args);
        case 6: return (int)sizeof(ina_seqpool_args);
        case 7: return (int)sizeof(ina_select_args);
        case 8: return (int)sizeof(ina_pool_act_args);
        case 9: return (int)sizeof(ina_gather_args);
        case 10: return (int)sizeof(ina_rope_args);
        case 11: return (int)sizeof(ina_mrope_table_args);
        case 12: return (int)sizeof(ina_argmax_args);
        case 13: return (int)sizeof(ina_dit_attn_args);
        case 14: return (int)sizeof(ina_resize_u8_args);
        case 15: return (int)sizeof(ina_qwen_patchify_args);
        case 16: return (int)sizeof(ina_u8_lut_args);
        case 17: return (int)sizeof(ina_resize_f32_args);
        case 18: return (int)sizeof(ina_gn_mish_args);
        case 19: return (int)sizeof(ina_pad_rows_args);
        case 20: return (int)sizeof(ina_ddim_step_args);
        case 21: return (int)sizeof(ina_ew_args);
        case 22: return (int)sizeof(ina_colsum_args);
        case 23: return (int)sizeof(ina_norm_bwd_args);
        case 24: return (int)sizeof(ina_transpose_args);
        case 25: return (int)sizeof(ina_sparse_rows_args);
        case 26: return (int)sizeof(ina_small_linear_args);
        case 27: return (int)sizeof(ina_mse_args);
        case 28: return (int)sizeof(ina_adamw_args);
        case 29: return (int)sizeof(ina_gemm_nn_args);
        case 30: return (int)sizeof(ina_attn_bwd_args);
        case 31: return (int)sizeof(ina_dit_rowchain_args);
        case 32: return (int)sizeof(ina_gemm_dw_args);
        default: return -1;
    }
}

#define INA_ENTRY(name, T, launch)                                             \
    int name(const T* args, void* stream) {                                     \
        INA_REQUIRE(args != nullptr, #name ": null args");                      \
        return launch(*args, reinterpret_cast<hipStream_t>(stream));            \
    }
INA_ENTRY(ina_patchify, ina_patchify_args, ina_launch_patchify)
INA_ENTRY(ina_embed3, ina_embed3_args, ina_launch_embed3)
INA_ENTRY(ina_head3, ina_head3_args, ina_launch_head3)
INA_ENTRY(ina_seqpool_head, ina_seqpool_args, ina_launch_seqpool)
INA_ENTRY(ina_select_traj, ina_select_args, ina_launch_select)
INA_ENTRY(ina_pool_act, ina_pool_act_args, ina_launch_pool_act)
INA_ENTRY(ina_gather_rows, ina_gather_args, ina_launch_gather)
INA_ENTRY(ina_rope_bf16, ina_rope_args, ina_launch_rope)
INA_ENTRY(ina_mrope_table, ina_mrope_table_args, ina_launch_mrope_table)
INA_ENTRY(ina_dit_attention, ina_dit_attn_args, ina_launch_dit_attention)
INA_ENTRY(ina_resize_u8, ina_resize_u8_args, ina_launch_resize_u8)
INA_ENTRY(ina_qwen_patchify_u8, ina_qwen_patchify_args, ina_launch_qwen_patchify_u8)
INA_ENTRY(ina_u8_lut, ina_u8_lut_args, ina_launch_u8_lut)
INA_ENTRY(ina_resize_f32, ina_resize_f32_args, ina_launch_resize_f32)
INA_ENTRY(ina_argmax_rows, ina_argmax_args, ina_launch_argmax)
INA_ENTRY(ina_dit_rowchain, ina_dit_rowchain_args, ina_launch_dit_rowchain)
INA_ENTRY(ina_gn_mish, ina_gn_mish_args, ina_launch_gn_mish)
INA_ENTRY(ina_pad_rows, ina_pad_rows_args, ina_launch_pad_rows)
INA_ENTRY(ina_ddim_step, ina_ddim_step_args, ina_launch_ddim_step)
INA_ENTRY(ina_ew, ina_ew_args, ina_launch_ew)
INA_ENTRY(ina_colsum, ina_colsum_args, ina_launch_colsum)
INA_ENTRY(ina_norm_bwd, ina_norm_bwd_args, ina_launch_norm_bwd)
INA_ENTRY(ina_transpose, ina_transpose_args, ina_launch_transpose)
INA_ENTRY(ina_sparse_rows, ina_sparse_rows_args, ina_launch_sparse_rows)
INA_ENTRY(ina_small_linear, ina_small_linear_args, ina_launch_small_linear)
INA_ENTRY(ina_mse_masked, ina_mse_args, ina_launch_mse)
INA_ENTRY(ina_adamw, ina_adamw_args, ina_launch_adamw)
INA_ENTRY(ina_gemm_nn_bf16, ina_gemm_nn_args, ina_launch_gemm_nn)
INA_ENTRY(ina_gemm_dw, ina_gemm_dw_args, ina_launch_gemm_dw)
INA_ENTRY(ina_attention_bwd_bf16, ina_attn_bwd_args, ina_launch_attention_bwd)
#undef INA_ENTRY

}  // extern "C"
