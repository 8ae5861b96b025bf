// Python bindings for the langstream_amd HIP kernels (module `_hip_ops`).
#include "ops.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "langstream_amd CDNA4 (gfx950) kernels";
  m.def("rmsnorm", &rmsnorm);
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm);
  m.def("layernorm", &layernorm);
  m.def("embed_layernorm", &embed_layernorm);
  m.def("silu_and_mul", &silu_and_mul);
  m.def("bias_gelu", &bias_gelu);
  // window (the attention ops): > 0 limits a query at position p to the keys p - window < key <= p; 0: no window
  // k_scale / v_scale: the per-engine scales of an fp8 (float8_e4m3fn) KV cache; bf16 caches ignore them
  m.def("rope_and_cache", &rope_and_cache, py::arg("qkv"), py::arg("pos"), py::arg("cos_sin"), py::arg("slots"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("Hq"), py::arg("Hkv"), py::arg("apply_rope"),
        py::arg("k_scale") = 1.0, py::arg("v_scale") = 1.0, py::arg("bias") = py::none(),
        py::arg("q_norm") = py::none(), py::arg("k_norm") = py::none(), py::arg("norm_eps") = 1e-6);
  m.def("paged_decode_attention", &paged_decode_attention, py::arg("out"), py::arg("q"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("block_tables"), py::arg("ctx_lens"), py::arg("scale"), py::arg("nsplit"),
        py::arg("blocks_per_split"), py::arg("workspace"), py::arg("k_scale") = 1.0, py::arg("v_scale") = 1.0,
        py::arg("window") = 0);
  m.def("paged_decode_attention_rope", &paged_decode_attention_rope, py::arg("out"), py::arg("qkv"), py::arg("pos"),
        py::arg("cos_sin"), py::arg("slots"), py::arg("k_cache"), py::arg("v_cache"), py::arg("block_tables"),
        py::arg("ctx_lens"), py::arg("scale"), py::arg("nsplit"), py::arg("blocks_per_split"), py::arg("workspace"),
        py::arg("window") = 0);
  m.def("paged_prefill_attention", &paged_prefill_attention, py::arg("out"), py::arg("q"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("block_tables"), py::arg("q_start"), py::arg("q_len"), py::arg("ctx_len"),
        py::arg("tiles"), py::arg("Hq"), py::arg("scale"), py::arg("k_scale") = 1.0, py::arg("v_scale") = 1.0,
        py::arg("window") = 0);
  m.def("varlen_encoder_attention", &varlen_encoder_attention);
  m.def("sample_tokens", &sample_tokens);
  m.def("apply_logit_deltas", &apply_logit_deltas);
  m.def("pool_embeddings", &pool_embeddings);
  m.def("l2_normalize_rows", &l2_normalize_rows);
  m.def("knn_topk", &knn_topk);
  m.def("oneshot_allreduce_sim", &oneshot_allreduce_sim, py::arg("inputs"), py::arg("calls"),
        py::arg("stall_rank") = -1);
  m.def("oneshot_allreduce_selftest", &oneshot_allreduce_selftest);
  m.def("oneshot_flags_uncached", &oneshot_flags_uncached);
  m.def("oneshot_collectives_selftest", &oneshot_collectives_selftest);
  m.def("oneshot_route_selftest", &oneshot_route_selftest);
  m.def("tp_sample_stats", &tp_sample_stats);
  m.def("tp_sample_hist", &tp_sample_hist);
  m.def("tp_sample_pick", &tp_sample_pick);
  m.def("tp_sample_final", &tp_sample_final);
  m.def("knn_default_sample", &knn_default_sample);
  m.def("knn_topk_ablate", &knn_topk_ablate);
  m.def("knn_topk_masked", &knn_topk_masked);
  m.def("knn_topk_biased", &knn_topk_biased);
  m.def("skinny_gemm", &skinny_gemm);
  m.def("gemv", &gemv);
  m.def("gemv_supported", &gemv_supported);
  m.def("gemv_silu", &gemv_silu);
  m.def("gemv_add_rmsnorm", &gemv_add_rmsnorm);
  m.def("gemv_norm", &gemv_norm);
  m.def("gemv_silu_norm", &gemv_silu_norm);
  m.def("gemv_qkv", &gemv_qkv);
  m.def("skinny_gemm_silu", &skinny_gemm_silu);
  m.def("gemm_fused", &gemm_fused, py::arg("out"), py::arg("x"), py::arg("w"), py::arg("bias") = py::none(),
        py::arg("gelu") = false, py::arg("residual") = py::none(), py::arg("ln_stats_in") = py::none(),
        py::arg("ln_width") = 0, py::arg("c1") = py::none(), py::arg("c2") = py::none(),
        py::arg("res_g") = py::none(), py::arg("res_b") = py::none(), py::arg("eps") = 1e-12,
        py::arg("stats_out") = py::none());
  m.def("skinny_gemm_add_rmsnorm", &skinny_gemm_add_rmsnorm);
  m.def("gemm_prefill", &gemm_prefill, py::arg("out"), py::arg("x"), py::arg("w"), py::arg("silu"), py::arg("variant") = -1);
  m.def("gemm_prefill_supported", &gemm_prefill_supported);
  m.def("gemm_prefill_f32", &gemm_prefill_f32, "out[M, N] (f32) = x . w^T on the ping-pong MFMA kernel");
  m.def("gemm_prefill_f32_supported", &gemm_prefill_f32_supported);
  m.def("decode_gemm_supported", &decode_gemm_supported);
  m.def("decode_gemm_workspace", &decode_gemm_workspace);
  m.def("decode_gemm", &decode_gemm, py::arg("out"), py::arg("x"), py::arg("w"), py::arg("workspace"),
        py::arg("residual") = py::none(), py::arg("norm_w") = py::none(), py::arg("eps") = 1e-5,
        py::arg("bn") = 0, py::arg("splits") = 0);
  m.def("decode_gemm_ablate", &decode_gemm_ablate);
  m.def("decode_gemm_qkv_rope", &decode_gemm_qkv_rope, py::arg("qkv"), py::arg("x"), py::arg("w"),
        py::arg("workspace"), py::arg("pos"), py::arg("cos_sin"), py::arg("slots"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("Hq"), py::arg("Hkv"), py::arg("k_scale") = 1.0, py::arg("v_scale") = 1.0,
        py::arg("bias") = py::none(), py::arg("q_norm") = py::none(), py::arg("k_norm") = py::none(),
        py::arg("norm_eps") = 1e-6);
  m.def("decode_gemm_f32_supported", &decode_gemm_f32_supported);
  m.def("decode_gemm_f32", &decode_gemm_f32, py::arg("out"), py::arg("x"), py::arg("w"), py::arg("bn") = 0);
  m.def("decode_gemm_silu", &decode_gemm_silu, py::arg("out"), py::arg("x"), py::arg("w"), py::arg("workspace"),
        py::arg("tickets"), py::arg("err"), py::arg("splits") = 0);
  m.def("decode_gemm_cmb_splits", &decode_gemm_cmb_splits);
  m.def("decode_gemm_res", &decode_gemm_res);
  m.def("decode_gemm_qkv_cmb", &decode_gemm_qkv_cmb);
  m.def("decode_gemm_silu_r", &decode_gemm_silu_r);
  m.def("decode_gemm_launch_counts", &decode_gemm_launch_counts, py::arg("reset") = false);
  m.def("rms_prep", &rms_prep);
  m.def("rows_rms_scale", &rows_rms_scale);
  m.def("w8_supported", &w8_supported);
  m.def("w8_gemv_supported", &w8_gemv_supported);
  m.def("w8_gemm_workspace", &w8_gemm_workspace);
  m.def("w8_gemm", &w8_gemm, py::arg("out"), py::arg("x"), py::arg("w"), py::arg("s"), py::arg("workspace"),
        py::arg("splits") = 0);
  m.def("w8_gemv", &w8_gemv);
  m.def("linear_w8", &linear_w8, py::arg("out"), py::arg("x"), py::arg("w"), py::arg("s"), py::arg("workspace"),
        py::arg("splits") = 0);
  m.def("w8_launch_counts", &w8_launch_counts, py::arg("reset") = false);
  bind_runners(m);
}
