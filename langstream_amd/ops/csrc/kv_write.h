// The paged-KV write contract, once: what a kernel that rotates q / k with RoPE and files a
// new token's K and V into the paged caches needs (KvWrite), how it is validated on the
// host (make_kv_write) and the device steps themselves.  The writers -- rope.hip,
// gemm_decode.hip (split-K reduce and the CMB_QKV epilogue), gemm_gemv.hip (EPI_QKV) and
// attention_decode.hip (ROPE) -- differ only in which thread holds which dims.
//
// cos_sin  : [max_pos, D] f32; cols [0, D/2) = cos, [D/2, D) = sin; dim d pairs with d + D/2
// slots    : [T] int64 cache slot = block * BS + offset; outside [0, nslots): not cached
// k_cache  : [NB, Hkv, BS, D]        token-major rows
// v_cache  : [NB, Hkv, BS/8, D, 8]   V^T in 8-key groups (common.h vt_off)
// bf16 or e4m3 caches (common.h "FP8 KV cache": same element offsets at 1 byte each, the
// codes made from the bf16-rounded values the qkv row gets).
#pragma once
#include "ops.h"

struct KvWrite {
  const int32_t* pos = nullptr;    // [T] absolute positions, clamped to the table
  const float* cos_sin = nullptr;
  int max_pos = 0;
  const int64_t* slots = nullptr;  // [T]
  int64_t nslots = 0;              // NB * BS
  void* kc = nullptr;              // bf16 or fp8_t elements
  void* vc = nullptr;
  int Hq = 0, Hkv = 0, BS = 0;
  float inv_k = 1.f, inv_v = 1.f;  // 1 / scale of the fp8 codes
};

// Where a token's K / V go: block and offset inside the block.
struct KvSlot {
  int64_t blk, off;
};

// The cos/sin table row of token t.
__device__ __forceinline__ const float* kv_cos_sin_row(const KvWrite& kw, int64_t t, int D) {
  const int p = min(max(kw.pos[t], 0), kw.max_pos - 1);
  return kw.cos_sin + (int64_t)p * D;
}

// cos / sin of dims d0 .. d0+N-1 (d0 < D/2) from a table row; float4 loads for N = 4, 8.
template <int N>
__device__ __forceinline__ void kv_load_cos_sin(const float* cs, int D, int d0, float* co, float* si) {
  static_assert(N == 1 || N == 4 || N == 8);
  if constexpr (N == 1) {
    co[0] = cs[d0];
    si[0] = cs[D / 2 + d0];
  } else {
#pragma unroll
    for (int j = 0; j < N; j += 4) {
      *reinterpret_cast<float4*>(co + j) = *reinterpret_cast<const float4*>(cs + d0 + j);
      *reinterpret_cast<float4*>(si + j) = *reinterpret_cast<const float4*>(cs + D / 2 + d0 + j);
    }
  }
}

// Rotates N pairs (a[j], b[j]) = dims (d0 + j, D/2 + d0 + j) in place, in f32.  Which of
// the two products of a line is fused into an fma is the compiler's choice per call site
// (-ffp-contract=fast), so two writers may differ in the last f32 bit; spelling the fmas
// out cost the ROPE attention kernel its last free VGPRs (4 spilled at D = 128, WPP = 4).
template <int N>
__device__ __forceinline__ void kv_rotate(const float* co, const float* si, float* a, float* b) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float x1 = a[j], x2 = b[j];
    a[j] = x1 * co[j] - x2 * si[j];
    b[j] = x2 * co[j] + x1 * si[j];
  }
}

// False when token t is not cached.
__device__ __forceinline__ bool kv_slot(const KvWrite& kw, int64_t t, KvSlot& s) {
  const int64_t sl = kw.slots[t];
  if (sl < 0 || sl >= kw.nslots) return false;
  s.blk = sl / kw.BS;
  s.off = sl - s.blk * kw.BS;
  return true;
}

// K: dims d0 .. d0+N-1 of kv head h (v: bf16, bf16x4 or bf16x8), one store: bf16 2 / 8 /
// 16 B; fp8 4 / 8 B.
template <bool F8, int N, typename V>
__device__ __forceinline__ void kv_store_k(const KvWrite& kw, KvSlot s, int h, int D, int d0, V v) {
  static_assert((N == 1 || N == 4 || N == 8) && sizeof(V) == 2 * N);
  const int64_t ko = ((s.blk * kw.Hkv + h) * kw.BS + s.off) * D + d0;
  if constexpr (F8) {
    static_assert(N != 1);
    fp8_t* kd = static_cast<fp8_t*>(kw.kc) + ko;
    if constexpr (N == 4)
      *reinterpret_cast<uint32_t*>(kd) = fp8_pack4((float)v[0], (float)v[1], (float)v[2], (float)v[3], kw.inv_k);
    else
      *reinterpret_cast<uint2*>(kd) = fp8_pack8(v, kw.inv_k);
  } else {
    *reinterpret_cast<V*>(static_cast<bf16*>(kw.kc) + ko) = v;
  }
}

// V^T: dims d0 .. d0+N-1 of kv head h at the slot's key, N scalar stores.
template <bool F8, int N, typename V>
__device__ __forceinline__ void kv_store_v(const KvWrite& kw, KvSlot s, int h, int D, int d0, V v) {
  static_assert(sizeof(V) == 2 * N);
  const int64_t vo = ((s.blk * kw.Hkv + h) * (int64_t)D) * kw.BS;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    bf16 e;
    if constexpr (N == 1) e = v;
    else e = v[j];
    const int64_t o = vo + vt_off(d0 + j, (int)s.off, D);
    if constexpr (F8) static_cast<fp8_t*>(kw.vc)[o] = fp8_from_bf16(e, kw.inv_v);
    else static_cast<bf16*>(kw.vc)[o] = e;
  }
}

// The descriptor for T tokens, with every check the writers share.  `who` names the entry
// point in the messages; allow_fp8 = false refuses e4m3 caches (kv_require_bf16).  Returns
// the cache dtype through is_fp8 when given.
inline KvWrite make_kv_write(const char* who, const at::Tensor& pos, const at::Tensor& cos_sin,
                             const at::Tensor& slots, const at::Tensor& k_cache, const at::Tensor& v_cache, int64_t T,
                             int64_t Hq, int64_t Hkv, bool allow_fp8, double k_scale = 1.0, double v_scale = 1.0,
                             bool* is_fp8 = nullptr) {
  bool f8 = false;
  if (allow_fp8) f8 = kv_is_fp8(k_cache, v_cache, who);
  else kv_require_bf16(k_cache, v_cache, who);
  if (is_fp8) *is_fp8 = f8;
  TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && k_cache.dim() == 4 && v_cache.dim() == 5 &&
                  k_cache.is_contiguous() && v_cache.is_contiguous(),
              who, ": contiguous k_cache [NB, Hkv, BS, D] and v_cache [NB, Hkv, BS/8, D, 8]");
  const int64_t NB = k_cache.size(0), BS = k_cache.size(2), D = k_cache.size(3);
  TORCH_CHECK(k_cache.size(1) == Hkv && v_cache.size(1) == Hkv, who, ": Hkv = ", Hkv, " but the caches hold ",
              k_cache.size(1), " (K) and ", v_cache.size(1), " (V) heads");
  TORCH_CHECK(v_cache.size(0) == NB && BS % 8 == 0 && v_cache.size(2) == BS / 8 && v_cache.size(3) == D &&
                  v_cache.size(4) == 8, who, ": v_cache must be [NB, Hkv, BS/8, D, 8] for k_cache [NB, Hkv, BS, D]");
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous() && cos_sin.dim() == 2 &&
                  cos_sin.size(1) == D && cos_sin.size(0) >= 1, who, ": cos_sin f32 [max_pos >= 1, D] contiguous");
  TORCH_CHECK(pos.scalar_type() == at::kInt && pos.numel() >= T, who, ": pos int32, one per token");
  TORCH_CHECK(slots.scalar_type() == at::kLong && slots.numel() >= T, who, ": slots int64, one per token");
  KvWrite kw;
  kw.pos = pos.data_ptr<int32_t>();
  kw.cos_sin = cos_sin.data_ptr<float>();
  kw.max_pos = (int)cos_sin.size(0);
  kw.slots = slots.data_ptr<int64_t>();
  kw.nslots = NB * BS;
  kw.kc = k_cache.data_ptr();
  kw.vc = v_cache.data_ptr();
  kw.Hq = (int)Hq;
  kw.Hkv = (int)Hkv;
  kw.BS = (int)BS;
  kw.inv_k = kv_inv_scale(k_scale);
  kw.inv_v = kv_inv_scale(v_scale);
  return kw;
}
