// Host entry points of the langstream_amd HIP kernels: the ONE place a function that is
// defined in one .hip and used in another (bindings.hip, runner.hip, the split-K launch
// helpers) is declared.  Every .hip that defines one of these includes this header, so a
// changed signature is a compile error, not a new overload found at link or import time.
// Default argument values live in the py::arg lists of bindings.hip, never here.
//
// Also the two readers every LS_* environment knob goes through (env_flag, env_int).
#pragma once
#include <torch/extension.h>
#include <torch/csrc/distributed/c10d/ProcessGroup.hpp>

#include <cstdlib>
#include <memory>
#include <vector>

#include "common.h"

// ------------------------------------------------------------------------------- knobs
// An integer knob: unset -> dflt, otherwise the leading decimal integer of the value
// (atoll: "" and words read as 0).
inline int64_t env_int(const char* name, int64_t dflt) {
  const char* v = getenv(name);
  return v ? atoll(v) : dflt;
}
// An on/off knob: unset -> dflt, otherwise on iff env_int reads a non-zero integer ("1",
// "2": on; "0", "", "false": off).  Neither helper caches: a knob read once per process
// is a `static const` at its use site, one read per launch or per construction is a
// plain call.
inline bool env_flag(const char* name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; }

// ------------------------------------------------------------------------ fp8 KV cache
// The paged caches are bf16 or, opt-in, OCP e4m3 (torch.float8_e4m3fn; format in common.h).
// True for an fp8 pair, false for a bf16 pair; anything else (mixed K / V included) raises.
inline bool kv_is_fp8(const at::Tensor& k_cache, const at::Tensor& v_cache, const char* who) {
  const auto kt = k_cache.scalar_type(), vt = v_cache.scalar_type();
  TORCH_CHECK(kt == vt && (kt == at::kBFloat16 || kt == at::kFloat8_e4m3fn), who,
              ": k_cache and v_cache must both be bf16 or both float8_e4m3fn");
  return kt == at::kFloat8_e4m3fn;
}
// Entry points that write bf16 into the cache and have no fp8 form.
inline void kv_require_bf16(const at::Tensor& k_cache, const at::Tensor& v_cache, const char* who) {
  TORCH_CHECK(k_cache.scalar_type() == at::kBFloat16 && v_cache.scalar_type() == at::kBFloat16, who,
              ": writes bf16 K/V and does not support an fp8 (float8_e4m3fn) KV cache; use rope_and_cache or "
              "decode_gemm_qkv_rope for fp8 caches");
}
// 1 / scale, once, as the f32 every writer multiplies by.
inline float kv_inv_scale(double scale) {
  TORCH_CHECK(scale > 0.0, "KV cache scale must be positive");
  return 1.0f / (float)scale;
}

// ---------------------------------------------------------------------------- qkv bias
// The optional bias of a fused QKV projection (Qwen2): bf16 [(Hq + 2 Hkv) D] in the packed
// order q heads, k heads, v heads, added in f32 before the rotation.  Returns its data
// pointer, nullptr without a bias; `who` names the op in the messages.
inline const bf16* qkv_bias_ptr(const char* who, const c10::optional<at::Tensor>& bias, const at::Tensor& qkv,
                                int64_t width) {
  if (!bias.has_value()) return nullptr;
  const at::Tensor& b = *bias;
  TORCH_CHECK(b.is_cuda() && b.device() == qkv.device(), who, ": bias must be on the device of qkv");
  TORCH_CHECK(b.scalar_type() == at::kBFloat16, who, ": bias must be bf16");
  TORCH_CHECK(b.is_contiguous(), who, ": bias must be contiguous");
  TORCH_CHECK(b.numel() == width, who, ": bias has ", b.numel(), " elements, (Hq + 2 Hkv) D = ", width);
  TORCH_CHECK((reinterpret_cast<uintptr_t>(b.data_ptr()) & 15) == 0, who, ": bias must be 16-byte aligned");
  return reinterpret_cast<const bf16*>(b.data_ptr());
}

// ---------------------------------------------------------------------------- q / k norm
// The optional per-head RMSNorm of the q and the k heads (Qwen3): one bf16 [D] weight
// shared by all q heads and one by all k heads, applied in f32 over the head dimension
// after the bias and before the rotation; v heads are not normed.  Both weights or neither.
struct QkNorm {
  const bf16* q = nullptr;   // nullptr: no norm
  const bf16* k = nullptr;
  float eps = 0.f;
};
inline QkNorm qk_norm_args(const char* who, const c10::optional<at::Tensor>& q_norm,
                           const c10::optional<at::Tensor>& k_norm, double eps, const at::Tensor& qkv, int64_t D) {
  QkNorm n;
  TORCH_CHECK(q_norm.has_value() == k_norm.has_value(), who, ": q_norm and k_norm are given together or not at all");
  if (!q_norm.has_value()) return n;
  TORCH_CHECK(eps > 0.0, who, ": norm_eps must be positive with q_norm / k_norm");
  const at::Tensor* ws[2] = {&*q_norm, &*k_norm};
  const char* names[2] = {"q_norm", "k_norm"};
  for (int i = 0; i < 2; ++i) {
    const at::Tensor& w = *ws[i];
    TORCH_CHECK(w.is_cuda() && w.device() == qkv.device(), who, ": ", names[i], " must be on the device of qkv");
    TORCH_CHECK(w.scalar_type() == at::kBFloat16, who, ": ", names[i], " must be bf16");
    TORCH_CHECK(w.is_contiguous(), who, ": ", names[i], " must be contiguous");
    TORCH_CHECK(w.numel() == D, who, ": ", names[i], " has ", w.numel(), " elements, head_dim = ", D);
    TORCH_CHECK((reinterpret_cast<uintptr_t>(w.data_ptr()) & 15) == 0, who, ": ", names[i],
                " must be 16-byte aligned");
  }
  n.q = reinterpret_cast<const bf16*>(q_norm->data_ptr());
  n.k = reinterpret_cast<const bf16*>(k_norm->data_ptr());
  n.eps = (float)eps;
  return n;
}

// ---------------------------------------------------------------------------- norm.hip
void rmsnorm(at::Tensor out, at::Tensor x, at::Tensor w, double eps);
void fused_add_rmsnorm(at::Tensor x, at::Tensor residual, at::Tensor w, double eps);
void layernorm(at::Tensor out, at::Tensor x, c10::optional<at::Tensor> bias, c10::optional<at::Tensor> residual,
               at::Tensor g, at::Tensor b, double eps);
void embed_layernorm(at::Tensor out, at::Tensor ids, at::Tensor pos_ids, c10::optional<at::Tensor> type_ids,
                     at::Tensor wte, at::Tensor wpe, at::Tensor wtt, at::Tensor g, at::Tensor b, double eps);

// ---------------------------------------------------------------------- activation.hip
void silu_and_mul(at::Tensor out, at::Tensor x);
void bias_gelu(at::Tensor x, c10::optional<at::Tensor> bias);

// ---------------------------------------------------------------------------- rope.hip
void rope_and_cache(at::Tensor qkv, at::Tensor pos, at::Tensor cos_sin, at::Tensor slots, at::Tensor k_cache,
                    at::Tensor v_cache, int64_t Hq, int64_t Hkv, bool apply_rope, double k_scale, double v_scale,
                    c10::optional<at::Tensor> bias, c10::optional<at::Tensor> q_norm = c10::nullopt,
                    c10::optional<at::Tensor> k_norm = c10::nullopt, double norm_eps = 1e-6);

// ---------------------------------------------------------------- attention_decode.hip
void paged_decode_attention(at::Tensor out, at::Tensor q, at::Tensor k_cache, at::Tensor v_cache,
                            at::Tensor block_tables, at::Tensor ctx_lens, double scale, int64_t nsplit,
                            int64_t blocks_per_split, at::Tensor workspace, double k_scale, double v_scale,
                            int64_t window);
void paged_decode_attention_rope(at::Tensor out, at::Tensor qkv, at::Tensor pos, at::Tensor cos_sin,
                                 at::Tensor slots, at::Tensor k_cache, at::Tensor v_cache, at::Tensor block_tables,
                                 at::Tensor ctx_lens, double scale, int64_t nsplit, int64_t min_bps,
                                 at::Tensor workspace, int64_t window);

// --------------------------------------------------------------- attention_prefill.hip
void paged_prefill_attention(at::Tensor out, at::Tensor q, at::Tensor k_cache, at::Tensor v_cache,
                             at::Tensor block_tables, at::Tensor q_start, at::Tensor q_len, at::Tensor ctx_len,
                             at::Tensor tiles, int64_t Hq, double scale, double k_scale, double v_scale,
                             int64_t window);
void varlen_encoder_attention(at::Tensor out, at::Tensor qkv, at::Tensor q_start, at::Tensor q_len,
                              at::Tensor tiles, int64_t Hq, int64_t Hkv, double scale);

// ------------------------------------------------------------------------ sampling.hip
void sample_tokens(at::Tensor logits, at::Tensor temperature, at::Tensor top_k, at::Tensor top_p, at::Tensor seeds,
                   at::Tensor steps, at::Tensor out_tok, at::Tensor out_lp, at::Tensor top_ids, at::Tensor top_lps,
                   int64_t n_top);
void apply_logit_deltas(at::Tensor logits, at::Tensor rows, at::Tensor toks, at::Tensor delta);
void tp_sample_stats(at::Tensor logits, int64_t vstart, at::Tensor stats);
void tp_sample_hist(at::Tensor logits, int64_t vtot, at::Tensor temperature, at::Tensor top_k, at::Tensor top_p,
                    at::Tensor stats_all, int64_t world, at::Tensor hist);
void tp_sample_pick(at::Tensor logits, int64_t vstart, int64_t vtot, at::Tensor temperature, at::Tensor top_k,
                    at::Tensor top_p, at::Tensor seeds, at::Tensor steps, at::Tensor stats_all, int64_t world,
                    at::Tensor hist_all, int64_t n_top, at::Tensor cand);
void tp_sample_final(at::Tensor stats_all, at::Tensor cand_all, int64_t world, int64_t rows, at::Tensor temperature,
                     int64_t n_top, at::Tensor out_tok, at::Tensor out_lp, at::Tensor top_ids, at::Tensor top_lps);

// ------------------------------------------------------------------------- pooling.hip
void pool_embeddings(at::Tensor out, at::Tensor x, at::Tensor start, at::Tensor len, int64_t mode, bool normalize);
void l2_normalize_rows(at::Tensor out, at::Tensor x);

// ----------------------------------------------------------------------- allreduce.hip
class OneShotAllReduce;
std::shared_ptr<OneShotAllReduce> make_oneshot_allreduce(c10::intrusive_ptr<::c10d::ProcessGroup> pg,
                                                         int64_t max_elems);
void oneshot_allreduce_run(const std::shared_ptr<OneShotAllReduce>& ar, at::Tensor t);
void oneshot_allreduce_i64(const std::shared_ptr<OneShotAllReduce>& ar, at::Tensor t);
void oneshot_allgather32(const std::shared_ptr<OneShotAllReduce>& ar, const at::Tensor& in, at::Tensor out);
int64_t oneshot_capacity_bytes(const std::shared_ptr<OneShotAllReduce>& ar);
bool oneshot_route_sum_i64(const std::shared_ptr<OneShotAllReduce>& ar,
                           const c10::intrusive_ptr<::c10d::ProcessGroup>& pg, at::Tensor t);
bool oneshot_route_gather32(const std::shared_ptr<OneShotAllReduce>& ar,
                            const c10::intrusive_ptr<::c10d::ProcessGroup>& pg, const at::Tensor& src,
                            const at::Tensor& dst);
const int* oneshot_allreduce_err(const std::shared_ptr<OneShotAllReduce>& ar);
std::vector<at::Tensor> oneshot_allreduce_sim(std::vector<at::Tensor> inputs, int64_t calls, int64_t stall_rank);
int64_t oneshot_allreduce_selftest(pybind11::object process_group, at::Tensor t);
bool oneshot_flags_uncached(pybind11::object process_group);
std::vector<at::Tensor> oneshot_collectives_selftest(pybind11::object process_group, at::Tensor bf, at::Tensor g32,
                                                     at::Tensor i64, int64_t cap);
std::vector<at::Tensor> oneshot_route_selftest(pybind11::object process_group, at::Tensor g32, at::Tensor i64,
                                               int64_t cap);

// ----------------------------------------------------------------------------- knn.hip
void knn_topk(at::Tensor X, at::Tensor Q, int64_t K, at::Tensor out_s, at::Tensor out_i, at::Tensor ws_s,
              at::Tensor ws_i, int64_t sample);
void knn_topk_masked(at::Tensor X, at::Tensor Q, int64_t K, at::Tensor out_s, at::Tensor out_i, at::Tensor ws_s,
                     at::Tensor ws_i, int64_t sample, at::Tensor mask, at::Tensor qmask);
void knn_topk_biased(at::Tensor X, at::Tensor Q, int64_t K, at::Tensor out_s, at::Tensor out_i, at::Tensor ws_s,
                     at::Tensor ws_i, int64_t sample, at::Tensor bias, at::Tensor mask, at::Tensor qmask);
void knn_topk_ablate(at::Tensor X, at::Tensor Q, int64_t K, at::Tensor out_s, at::Tensor out_i, at::Tensor ws_s,
                     at::Tensor ws_i, int64_t sample, int64_t abl);
int64_t knn_default_sample();

// --------------------------------------------------------------------- gemm_skinny.hip
void skinny_gemm(at::Tensor out, at::Tensor x, at::Tensor w);
void skinny_gemm_silu(at::Tensor out, at::Tensor x, at::Tensor w);
void skinny_gemm_add_rmsnorm(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor residual, at::Tensor norm_w,
                             double eps);
// Launch helpers for the split-K reductions, shared with gemm_decode.hip and gemm_prefill.hip.
void splitk_reduce_launch(const float* part, int S, int M, int N, bf16* out, int64_t ldo, hipStream_t st);
void splitk_add_rmsnorm_launch(const float* part, int S, int M, int N, bf16* residual, const bf16* norm_w, float eps,
                               bf16* out, hipStream_t st);

// ----------------------------------------------------------------------- gemm_gemv.hip
void gemv(at::Tensor out, at::Tensor x, at::Tensor w);
bool gemv_supported(const at::Tensor& w, bool silu);
void gemv_silu(at::Tensor out, at::Tensor x, at::Tensor w);
void gemv_add_rmsnorm(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor residual, at::Tensor norm_w,
                      double eps, at::Tensor counter);
void gemv_norm(at::Tensor out, at::Tensor o, at::Tensor res, at::Tensor res_out, at::Tensor norm_w, double eps,
               at::Tensor w);
void gemv_silu_norm(at::Tensor out, at::Tensor o, at::Tensor res, at::Tensor res_out, at::Tensor norm_w, double eps,
                    at::Tensor w);
void gemv_qkv(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor pos, at::Tensor cos_sin, at::Tensor slots,
              at::Tensor k_cache, at::Tensor v_cache, int64_t Hq, int64_t Hkv, bool apply_rope,
              c10::optional<at::Tensor> o, c10::optional<at::Tensor> res, c10::optional<at::Tensor> res_out,
              c10::optional<at::Tensor> norm_w, double eps);

// ---------------------------------------------------------------------- gemm_fused.hip
void gemm_fused(at::Tensor out, at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias, bool gelu,
                c10::optional<at::Tensor> residual, c10::optional<at::Tensor> ln_stats_in, int64_t ln_width,
                c10::optional<at::Tensor> c1, c10::optional<at::Tensor> c2, c10::optional<at::Tensor> res_g,
                c10::optional<at::Tensor> res_b, double eps, c10::optional<at::Tensor> stats_out);

// -------------------------------------------------------------------- gemm_prefill.hip
void gemm_prefill(at::Tensor out, at::Tensor x, at::Tensor w, bool silu, int64_t variant);
bool gemm_prefill_supported(const at::Tensor& w, bool silu);
void gemm_prefill_f32(at::Tensor out, at::Tensor x, at::Tensor w);
bool gemm_prefill_f32_supported(const at::Tensor& w);

// --------------------------------------------------------------------- gemm_decode.hip
bool decode_gemm_supported(const at::Tensor& w, bool silu);
int64_t decode_gemm_workspace(int64_t M, int64_t N, int64_t K, bool silu);
void decode_gemm(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor workspace, c10::optional<at::Tensor> residual,
                 c10::optional<at::Tensor> norm_w, double eps, int64_t bn_force, int64_t splits_force);
void decode_gemm_qkv_rope(at::Tensor qkv, at::Tensor x, at::Tensor w, at::Tensor workspace, at::Tensor pos,
                          at::Tensor cos_sin, at::Tensor slots, at::Tensor k_cache, at::Tensor v_cache, int64_t Hq,
                          int64_t Hkv, double k_scale, double v_scale, c10::optional<at::Tensor> bias,
                          c10::optional<at::Tensor> q_norm = c10::nullopt,
                          c10::optional<at::Tensor> k_norm = c10::nullopt, double norm_eps = 1e-6);
bool decode_gemm_f32_supported(const at::Tensor& w, int64_t M);
void decode_gemm_f32(at::Tensor out, at::Tensor x, at::Tensor w, int64_t bn_force);
void decode_gemm_silu(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor workspace, at::Tensor tickets,
                      at::Tensor err, int64_t splits);
void decode_gemm_ablate(at::Tensor x, at::Tensor w, at::Tensor workspace, int64_t abl, int64_t splits,
                        int64_t split_outer);
int64_t decode_gemm_cmb_splits(int64_t N, int64_t K);
void decode_gemm_res(at::Tensor y_out, at::Tensor x, at::Tensor w, at::Tensor workspace, at::Tensor counters,
                     at::Tensor residual, at::Tensor norm_g, at::Tensor sumsq_out, at::Tensor err);
void decode_gemm_qkv_cmb(at::Tensor qkv, at::Tensor x, at::Tensor w, at::Tensor workspace, at::Tensor counters,
                         at::Tensor sumsq_in, double eps, at::Tensor pos, at::Tensor cos_sin, at::Tensor slots,
                         at::Tensor k_cache, at::Tensor v_cache, int64_t Hq, int64_t Hkv, at::Tensor err);
void decode_gemm_silu_r(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor sumsq_in, double eps);
pybind11::dict decode_gemm_launch_counts(bool reset);
void rms_prep(at::Tensor y, at::Tensor sumsq, at::Tensor h, at::Tensor g);
void rows_rms_scale(at::Tensor out, at::Tensor y, at::Tensor sumsq, double eps);

// ------------------------------------------------------------------------ gemm_w8.hip
// W8A16 projections: e4m3fn weight codes [N, K] with one f32 scale per output row.
bool w8_supported(const at::Tensor& w);
bool w8_gemv_supported(const at::Tensor& w);
int64_t w8_gemm_workspace(int64_t M, int64_t N, int64_t K);
void w8_gemm(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor s, at::Tensor workspace, int64_t splits_force);
void w8_gemv(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor s);
void linear_w8(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor s, at::Tensor workspace, int64_t splits_force);
pybind11::dict w8_launch_counts(bool reset);

// -------------------------------------------------------------------------- runner.hip
void bind_runners(pybind11::module_& m);
