// RoPE + paged-KV cache write, fused (one pass over the QKV projection output).
//
// qkv      : [T, (Hq + 2*Hkv) * D] bf16, rotated IN PLACE for the q and k heads
// pos      : [T] int32 absolute positions
// cos_sin  : [max_pos, D] f32 table; cols [0, D/2) = cos, [D/2, D) = sin (host-built,
//            includes any rope scaling; no device trig -- guide App. B "element-wise")
// slots    : [T] int64 cache slot = block * BS + offset (-1 = do not cache)
// k_cache  : [NB, Hkv, BS, D]   (token-major rows: 256-B contiguous per token & head)
// v_cache  : [NB, Hkv, BS/8, D, 8]   (TRANSPOSED in 8-key groups: 8 keys of one dim are
//            16 contiguous bytes, so attention reads V^T MFMA fragments with one 16-B load
//            per lane; a token's V lands at a 16-B stride -- common.h vt_off)
// The rotation, the slot test and the cache stores are those of kv_write.h.
//
// Grid: x = tiles of TOK tokens, y = head groups.  y < nq: rotate HG query heads;
// nq <= y < nq+nk: rotate HG key heads and store them to the K cache; the last Hkv
// y-slices write one kv head of V transposed, with lane == token inside a tile so a
// wave's 2-B stores for one head-dim row land on consecutive cache addresses.
// Many small workgroups: a decode step (T = batch) still spreads over
// (T/16) x (Hq/8 + Hkv/8 + Hkv) workgroups instead of one.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "kv_write.h"

namespace {

// Tokens per workgroup tile: 16 for prefill-sized T; 2 for decode-sized T, so a
// B=256 decode step launches ~1.7k workgroups with one task per thread instead of
// 208 workgroups looping over dependent pos -> cos/sin loads (12 us -> latency of one).
constexpr int TOK_LARGE = 16;
constexpr int TOK_SMALL = 2;
constexpr int64_t SMALL_T = 2048;
constexpr int HG = 8;    // heads per rotate workgroup

// F8: e4m3 caches (kv_write.h): K as one 8-byte store per 8 rotated values, V as 1-byte
// stores at an 8-byte stride.
// BIAS: a bf16 bias [(Hq + 2 Hkv) D] (q, k, v heads in the packed order: a QKV projection
// with bias, Qwen2) is added in f32 before the rotation, one rounding as without it.  V
// gets it too, so the V branch then writes bf16(v + b) back into the row as well as into
// the cache -- the cache holds the bf16 value of the row (kv_write.h) for all three parts
// -- and does so for tokens that are not cached.
// NORM: a per-head RMSNorm of the q and the k heads (Qwen3) after the bias and before the
// rotation, all in f32: x * rsqrt(mean(x^2) + eps) * w[d], with one bf16 [D] weight for all
// q heads (nw.q) and one for all k heads (nw.k).  A head's D values sit in VPH adjacent
// lanes, 16 each, so the mean is a sum in registers and an xor-shuffle over that group.
// V heads are not normed: the V branch is the same with and without NORM.
template <int D, int TOK, bool F8, bool BIAS, bool NORM>
__global__ void __launch_bounds__(256) rope_cache_kernel(bf16* __restrict__ qkv, KvWrite kw, int64_t T,
                                                         int apply_rope, const bf16* __restrict__ bias, QkNorm nw) {
  constexpr int HALF = D / 2;
  constexpr int VPH = HALF / 8;  // 16-B vectors per half head
  const int Hq = kw.Hq, Hkv = kw.Hkv;
  const int64_t t0 = (int64_t)blockIdx.x * TOK;
  const int ntok = (int)min((int64_t)TOK, T - t0);
  const int row_elems = (Hq + 2 * Hkv) * D;
  const int nq = (Hq + HG - 1) / HG, nk = (Hkv + HG - 1) / HG;
  const int y = blockIdx.y;
  if (y < nq + nk) {
    // ---- rotate a group of q (or k) heads for the tile's tokens
    const bool is_k = y >= nq;
    const int h0 = is_k ? Hq + (y - nq) * HG : y * HG;
    const int hend = is_k ? Hq + Hkv : Hq;
    const int nh = min(HG, hend - h0);
    const int tasks = ntok * nh * VPH;
    for (int i = threadIdx.x; i < tasks; i += blockDim.x) {
      const int tl = i / (nh * VPH);
      const int rem = i - tl * nh * VPH;
      const int h = h0 + rem / VPH, c = rem % VPH;
      const int64_t t = t0 + tl;
      bf16* base = qkv + t * row_elems + h * D;
      float a[8], b[8];
      unpack8(ld16(base + c * 8), a);
      unpack8(ld16(base + HALF + c * 8), b);
      if constexpr (BIAS) {
        float ba[8], bb[8];
        unpack8(ld16(bias + h * D + c * 8), ba);
        unpack8(ld16(bias + h * D + HALF + c * 8), bb);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          a[j] += ba[j];
          b[j] += bb[j];
        }
      }
      if constexpr (NORM) {
        // i = (tl * nh + head) * VPH + c and blockDim.x is a multiple of VPH, so the VPH
        // lanes of a head are an aligned group of one wave; tasks is a multiple of VPH, so
        // a group is wholly inside or wholly outside this loop and every lane the shuffle
        // reads is active.
        float wa[8], wb[8];
        const bf16* w = is_k ? nw.k : nw.q;
        unpack8(ld16(w + c * 8), wa);
        unpack8(ld16(w + HALF + c * 8), wb);
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += a[j] * a[j] + b[j] * b[j];
#pragma unroll
        for (int o = VPH / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, VPH);
        const float r = rsqrtf(ss * (1.f / D) + nw.eps);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          a[j] = a[j] * r * wa[j];
          b[j] = b[j] * r * wb[j];
        }
      }
      if (apply_rope) {
        float co[8], si[8];
        kv_load_cos_sin<8>(kv_cos_sin_row(kw, t, D), D, c * 8, co, si);
        kv_rotate<8>(co, si, a, b);
      }
      const uint4 pa = pack8(a), pb = pack8(b);
      st16(base + c * 8, pa);
      st16(base + HALF + c * 8, pb);
      KvSlot s;
      if (is_k && kv_slot(kw, t, s)) {
        kv_store_k<F8, 8>(kw, s, h - Hq, D, c * 8, __builtin_bit_cast(bf16x8, pa));
        kv_store_k<F8, 8>(kw, s, h - Hq, D, HALF + c * 8, __builtin_bit_cast(bf16x8, pb));
      }
    }
    return;
  }
  // ---- V of one kv head, transposed into the cache.  thread -> (token lane, d-row)
  const int hv = y - nq - nk;
  const int tl = threadIdx.x % TOK;
  const int dr = threadIdx.x / TOK;  // 0..256/TOK-1
  if (tl >= ntok) return;
  const int64_t t = t0 + tl;
  KvSlot s;
  if constexpr (BIAS) {
    const bool cached = kv_slot(kw, t, s);
    bf16* row = qkv + t * row_elems + (Hq + Hkv + hv) * D;
    const bf16* bv = bias + (Hq + Hkv + hv) * D;
    for (int d = dr; d < D; d += 256 / TOK) {
      const bf16 v = (bf16)((float)row[d] + (float)bv[d]);
      row[d] = v;
      if (cached) kv_store_v<F8, 1>(kw, s, hv, D, d, v);
    }
  } else {
    if (!kv_slot(kw, t, s)) return;
    const bf16* src = qkv + t * row_elems + (Hq + Hkv + hv) * D;
    for (int d = dr; d < D; d += 256 / TOK) kv_store_v<F8, 1>(kw, s, hv, D, d, src[d]);
  }
}

}  // namespace

void rope_and_cache(at::Tensor qkv, at::Tensor pos, at::Tensor cos_sin, at::Tensor slots, at::Tensor k_cache,
                    at::Tensor v_cache, int64_t Hq, int64_t Hkv, bool apply_rope, double k_scale,
                    double v_scale, c10::optional<at::Tensor> bias, c10::optional<at::Tensor> q_norm,
                    c10::optional<at::Tensor> k_norm, double norm_eps) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.is_contiguous());
  TORCH_CHECK(k_cache.dim() == 4, "k_cache [NB, Hkv, BS, D], v_cache [NB, Hkv, BS/8, D, 8]");
  const int D = k_cache.size(3);
  TORCH_CHECK(qkv.size(-1) == (Hq + 2 * Hkv) * D);
  const int64_t T = qkv.numel() / qkv.size(-1);
  bool f8;
  const KvWrite kw = make_kv_write("rope_and_cache", pos, cos_sin, slots, k_cache, v_cache, T, Hq, Hkv, true,
                                   k_scale, v_scale, &f8);
  TORCH_CHECK(pos.numel() == T && slots.numel() == T);
  const bf16* bp = qkv_bias_ptr("rope_and_cache", bias, qkv, (Hq + 2 * Hkv) * D);
  const QkNorm nw = qk_norm_args("rope_and_cache", q_norm, k_norm, norm_eps, qkv, D);
  if (T == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  const int nq = (int)((Hq + HG - 1) / HG), nk = (int)((Hkv + HG - 1) / HG);
  const bool small = T <= SMALL_T;
  const int tok = small ? TOK_SMALL : TOK_LARGE;
  dim3 grid((unsigned)((T + tok - 1) / tok), nq + nk + (int)Hkv);
#define LAUNCH_N(DD, TT, FF, BB, NN)                                                                     \
  rope_cache_kernel<DD, TT, FF, BB, NN><<<grid, 256, 0, stream>>>((bf16*)qkv.data_ptr(), kw, T, apply_rope ? 1 : 0, \
                                                                  bp, nw)
#define LAUNCH_B(DD, TT, FF, BB) \
  if (nw.q) LAUNCH_N(DD, TT, FF, BB, true); else LAUNCH_N(DD, TT, FF, BB, false)
#define LAUNCH_F(DD, TT, FF) \
  if (bp) { LAUNCH_B(DD, TT, FF, true); } else { LAUNCH_B(DD, TT, FF, false); }
#define LAUNCH(DD, TT) \
  if (f8) { LAUNCH_F(DD, TT, true); } else { LAUNCH_F(DD, TT, false); }
  if (D == 128) { if (small) { LAUNCH(128, TOK_SMALL); } else { LAUNCH(128, TOK_LARGE); } }
  else if (D == 64) { if (small) { LAUNCH(64, TOK_SMALL); } else { LAUNCH(64, TOK_LARGE); } }
  else TORCH_CHECK(false, "unsupported head dim ", D);
#undef LAUNCH
#undef LAUNCH_F
#undef LAUNCH_B
#undef LAUNCH_N
}
