// Sparse mixture-of-experts MLP (Qwen3-MoE, Mixtral) for T rows of x (bf16 [T, H]):
//
//   logits = x . Wr^T (f32), p = softmax(logits) over the E experts, the k largest p per row
//   (lower expert index on a tie) are the row's slots, optionally renormalised to sum 1;
//   act = bf16(silu(x_t . Wg[e]^T) * (x_t . Wu[e]^T)),  y[t, s] = bf16(topk_w[t, s] * (act . Wd[e]^T)),
//   out[t] = bf16(sum_s y[t, s]) summed in f32 in slot order.
//   gate_up_w [E, 2F, H] holds the F gate rows then the F up rows of an expert, down_w [E, H, F].
//
// Four launches on the current stream, none with a data-dependent grid or a host sync, so a
// decode step replays as a graph:
//
// moe_route   router GEMM + softmax + top-k in one kernel; the logits live in LDS only.
//   T >= 16: a workgroup owns 16 rows, Wr streams through LDS once per workgroup in 64-column
//   slabs, wave w runs the 16x16x32 bf16 MFMA on the expert tiles w, w + 4, ...  T < 16: a
//   workgroup owns one row and its waves take the experts as 16-B dot products (a one-row MFMA
//   tile would leave 15/16 of the unit idle and T workgroups stream Wr in parallel).  Both end
//   in the same tail: a wave per row holds the E logits four per lane, forms the softmax, and
//   selects by k rounds of a wave-wide arg-max over (logit, index) -- softmax is monotonic, so
//   this is the order of the exact p, free of f32 ties between unequal logits.
// moe_align   one workgroup turns topk_ids into the tile schedule: per-expert counts (LDS
//   atomics), an exclusive scan of the counts rounded up to the tile height BM, sorted_rows
//   (flat slot index t k + s per padded row, -1 for padding), tile_expert and num_tiles.
//   Sizes depend on T, k, E and BM only: at most ceil(T k / BM) + min(E, T k) tiles.  Slots
//   whose id is outside [0, E) are dropped here and skipped by moe_combine.
// moe_gemm    the grouped GEMM, one template, two modes.  A workgroup (4 waves) owns one BM-row
//   tile of one expert and 64 output columns, reads its expert from tile_expert and leaves at
//   once when its tile index is past num_tiles.  Per 64-wide K step a thread moves its 16-B
//   chunks global -> registers -> LDS with the next step's loads in flight during the MFMAs
//   (two LDS stages where they fit in 64 KB, one otherwise).
//     gate_up: the A rows are gathered -- row r is x[sorted_rows[r] / k], padding rows are
//       zeros and read nothing; the weight slab is the tile's 64 gate rows and the matching
//       64 up rows, so SwiGLU runs in the epilogue on the f32 accumulators and act is stored
//       in sorted order [padded rows, F].
//     down: the A rows are the tile's contiguous act rows; the epilogue multiplies by the
//       row's topk_w, rounds once and scatters to y[sorted_rows[r]].  Padding rows store nothing.
//   BM = 32 (waves side by side along the columns; weights on non-temporal loads, each byte
//   is used once) serves decode, BM = 128 (waves stacked along the rows) prefill; tile_rows()
//   is the rule.
// moe_gemm_w8 the same grouped GEMM over fp8 (e4m3fn) expert weights with one f32 scale per (expert,
//   weight row), W8A16: y = (a . code^T) * s.  A code decodes to bf16 exactly, so the products run
//   on the bf16 MFMA; the weights cross HBM, L2 and LDS as bytes and are expanded at the MFMA
//   operand (fp8_unpack8).  The scale multiplies the f32 accumulator once, in the epilogue: the
//   gate and the up scale before SwiGLU, the down scale before topk_w and the one rounding.
//   K STEP: BM = 32 steps K by 128 codes, BM = 128 by 64.  The 32-row form lives on the bytes
//   it keeps in flight; with a 64-code step a thread would issue half the 16-B weight loads per
//   step that the bf16 kernel does (a row of 64 codes is four chunks, not eight), so its step is
//   doubled to keep the same four (gate_up) or two (down) loads per thread in flight.  A K that
//   is an odd multiple of 64 ends in a half step whose upper chunks are zeros.  Measured at
//   T = 16 (profiles/moe_fp8/README.md): 143 us against 186 us with a 64-code step on the
//   Qwen3-30B-A3B shape, 347 against 510 us on the Mixtral shape.  BM = 128 is compute-bound and
//   keeps 64: two stages of its A tile and a 128-code weight tile would not fit in 64 KB.
// moe_gemm_w4 the same grouped GEMM over int4 expert weights, the format of gemm_w4.hip per expert (W4A16):
//   packed 4-bit codes, one f32 scale and one zero point per (expert, weight row, group of G input
//   columns), y = sum_g s_g * sum_{k in g} a_k (q_k - z_g).  q - z is exact in bf16, so the products run
//   on the bf16 MFMA into a per-group f32 partial that is folded into the accumulator with s_g where
//   the group ends: the scales are in the main loop, not only in the epilogue.  BM = 32 keeps the
//   weights nibbles from HBM to LDS and expands them at the MFMA operand (w4_unpack8), as the fp8
//   form does with bytes; BM = 128, where all four waves need every weight row, expands a 16-B chunk
//   once, in the thread that carries it, and stores bf16 of q - z in the bf16 kernel's LDS layout.
//   K STEP: BM = 32 steps K by 256 codes, the byte count of the fp8 form's 128-code step (four or two
//   16-B weight loads per thread in flight); its two stages take 69 KB (gate_up) of the 160 KB of LDS.
//   Measured at T = 16 against a 128-code step (profiles/moe_int4/README.md): 212 against 225 us on the
//   Qwen3-30B-A3B shape, 562 against 556 us on the Mixtral shape; the 128-code build was dropped.
//   BM = 128 steps by 64 with two stages (72 KB in gate_up mode).
// moe_combine out[t] = bf16(sum_s y[t, s]) with 16-B loads.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <atomic>
#include <string>

#include "ops.h"

namespace {

constexpr int kMaxE = 256, kMaxK = 16;
constexpr int BN = 64, BK = 64;
constexpr int LDT = BK + 8;   // LDS row, bf16 elements (144 B: the 16 rows of an MFMA operand read hit distinct banks)

__device__ __forceinline__ bf16x8 lds8(const char* p) { return __builtin_bit_cast(bf16x8, ld16(p)); }

// ------------------------------------------------------------------------------ moe_route
// RB = 16: MFMA form, RB = 1: dot form.  grid = ceil(T / RB).
template <int RB>
__global__ void __launch_bounds__(256) moe_route_kernel(const bf16* __restrict__ x, int64_t ldx,
                                                        const bf16* __restrict__ wr, int T, int H, int E, int k,
                                                        int norm, int* __restrict__ ids, float* __restrict__ wts) {
  __shared__ float lg[RB][kMaxE + 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int r0 = blockIdx.x * RB;
  if constexpr (RB == 16) {
    __shared__ __attribute__((aligned(16))) char xs[16 * LDT * 2];
    __shared__ __attribute__((aligned(16))) char ws[kMaxE * LDT * 2];
    const int EP = (E + 15) & ~15, NT = EP >> 4;   // experts padded to whole MFMA tiles (zero rows)
    const int fr = lane & 15, fk = 8 * (lane >> 4);
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < H; k0 += BK) {
      if (tid < 128) {
        const int row = tid >> 3, c = tid & 7;
        const uint4 v = r0 + row < T ? ld16(x + (int64_t)(r0 + row) * ldx + k0 + c * 8) : make_uint4(0, 0, 0, 0);
        st16(xs + (row * LDT + c * 8) * 2, v);
      }
      for (int q = tid; q < EP * 8; q += 256) {
        const int row = q >> 3, c = q & 7;
        const uint4 v = row < E ? ld16(wr + (int64_t)row * H + k0 + c * 8) : make_uint4(0, 0, 0, 0);
        st16(ws + (row * LDT + c * 8) * 2, v);
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 a = lds8(xs + (fr * LDT + 32 * ks + fk) * 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int t = wid + 4 * j;   // wave-uniform
          if (t < NT)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, lds8(ws + ((16 * t + fr) * LDT + 32 * ks + fk) * 2),
                                                             acc[j], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    // acc[j][r] = logit of row 4 (lane >> 4) + r, expert 16 (wid + 4 j) + fr
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = wid + 4 * j;
      if (t < NT)
#pragma unroll
        for (int r = 0; r < 4; ++r) lg[4 * (lane >> 4) + r][16 * t + fr] = acc[j][r];
    }
  } else {
    const bf16* xr = x + (int64_t)r0 * ldx;
    for (int e = wid; e < E; e += 4) {
      const bf16* we = wr + (int64_t)e * H;
      float s = 0.f;
      for (int c = lane; c < (H >> 3); c += 64) {
        float a[8], b[8];
        unpack8(ld16(xr + c * 8), a);
        unpack8(ld16(we + c * 8), b);
#pragma unroll
        for (int i = 0; i < 8; ++i) s += a[i] * b[i];
      }
      s = wave_sum(s);
      if (lane == 0) lg[0][e] = s;
    }
  }
  __syncthreads();
  // tail: one wave per row, expert lane + 64 j in v[j]
  for (int r = wid; r < RB; r += 4) {
    const int t = r0 + r;
    if (t >= T) break;   // wave-uniform
    float v[4], p[4];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = lane + 64 * j < E ? lg[r][lane + 64 * j] : -INFINITY;
      m = fmaxf(m, v[j]);
    }
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      p[j] = lane + 64 * j < E ? expf(v[j] - m) : 0.f;
      s += p[j];
    }
    s = wave_sum(s);
    float mine = 0.f;   // lane i: exp(logit - max) of the i-th selected expert
    int mine_id = 0;
    for (int i = 0; i < k; ++i) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (v[j] > bv) {   // ascending j is ascending index: strict > keeps the lower one
          bv = v[j];
          bi = lane + 64 * j;
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      // every lane now holds the winner; its owner hands over the weight and retires it
      float pw = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (bi == lane + 64 * j) {
          pw = p[j];
          v[j] = -INFINITY;
        }
      pw = __shfl(pw, bi & 63, 64);
      if (lane == i) {
        mine = pw;
        mine_id = bi;
      }
    }
    const float sel = wave_sum(lane < k ? mine : 0.f);
    if (lane < k) {
      ids[(int64_t)t * k + lane] = mine_id;
      wts[(int64_t)t * k + lane] = mine / (norm ? sel : s);
    }
  }
}

// ------------------------------------------------------------------------------ moe_align
// One workgroup.  n = T k slots; num_tiles, tile_expert [max tiles], sorted_rows [max tiles x BM].
__global__ void __launch_bounds__(1024) moe_align_kernel(const int* __restrict__ ids, int n, int E, int BM,
                                                         int* __restrict__ num_tiles, int* __restrict__ tile_expert,
                                                         int* __restrict__ sorted_rows) {
  __shared__ int cnt[kMaxE], off[kMaxE + 1], cur[kMaxE];
  const int tid = threadIdx.x;
  if (tid < kMaxE) cnt[tid] = cur[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const int e = ids[i];
    if ((unsigned)e < (unsigned)E) atomicAdd(&cnt[e], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int e = 0; e < E; ++e) {
      off[e] = o;
      o += (cnt[e] + BM - 1) / BM * BM;
    }
    off[E] = o;
    *num_tiles = o / BM;
  }
  __syncthreads();
  for (int e = tid; e < E; e += 1024)
    for (int t = off[e] / BM; t < off[e + 1] / BM; ++t) tile_expert[t] = e;
  for (int i = tid; i < off[E]; i += 1024) sorted_rows[i] = -1;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const int e = ids[i];
    if ((unsigned)e < (unsigned)E) sorted_rows[off[e] + atomicAdd(&cur[e], 1)] = i;
  }
}

// ------------------------------------------------------------------------------- moe_gemm
// grid = (N / 64, max tiles).  gate_up (DOWN = false): a = x [T, lda], w = gate_up_w [E, 2 N, K],
// N = F, K = H, out = act [padded rows, F].  down: a = act [padded rows, K], w = down_w [E, N, K],
// N = H, K = F, out = y [T k, H].
template <int BM, bool DOWN>
__global__ void __launch_bounds__(256) moe_gemm_kernel(const bf16* __restrict__ a, int64_t lda,
                                                       const bf16* __restrict__ w, const int* __restrict__ num_tiles,
                                                       const int* __restrict__ tile_expert,
                                                       const int* __restrict__ sorted_rows,
                                                       const float* __restrict__ topk_w, int kk, int K, int N,
                                                       bf16* __restrict__ out) {
  constexpr int NW = DOWN ? BN : 2 * BN;            // weight rows per K step
  constexpr int AS = BM * LDT * 2, WS = NW * LDT * 2, STAGE = AS + WS;
  constexpr int ST = 2 * STAGE <= 65536 ? 2 : 1;    // LDS stages
  constexpr int AC = BM * 8 / 256, WC = NW * 8 / 256;   // 16-B chunks per thread per K step
  constexpr int WAVES_M = BM == 128 ? 4 : 1, WAVES_N = 4 / WAVES_M;
  constexpr int IT = BM / WAVES_M / 16, JT = BN / WAVES_N / 16;
  static_assert(BM == 32 || BM == 128, "tile heights");
  __shared__ __attribute__((aligned(16))) char lds[ST * STAGE];
  __shared__ int srow[BM];
  const int tile = blockIdx.y;
  if (tile >= *num_tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int e = tile_expert[tile];
  const int n0 = blockIdx.x * BN;
  const int64_t prow0 = (int64_t)tile * BM;
  if (tid < BM) srow[tid] = sorted_rows[prow0 + tid];
  __syncthreads();

  const bf16* ap[AC];
  bool aok[AC];
#pragma unroll
  for (int i = 0; i < AC; ++i) {
    const int q = tid + 256 * i, row = q >> 3, c = q & 7;
    const int idx = srow[row];
    aok[i] = idx >= 0;
    const int64_t grow = DOWN ? prow0 + row : (aok[i] ? idx / kk : 0);
    ap[i] = a + grow * lda + c * 8;
  }
  const bf16* wp[WC];
  const bf16* wbase = w + (int64_t)e * (DOWN ? N : 2 * N) * K;
#pragma unroll
  for (int i = 0; i < WC; ++i) {
    const int q = tid + 256 * i, row = q >> 3, c = q & 7;
    const int grow = DOWN || row < BN ? n0 + row : N + n0 + row - BN;   // gate rows, then the matching up rows
    wp[i] = wbase + (int64_t)grow * K + c * 8;
  }
  uint4 ra[AC], rw[WC];
  auto gload = [&](int kt) {
    const int ko = kt * BK;
#pragma unroll
    for (int i = 0; i < AC; ++i) ra[i] = aok[i] ? ld16(ap[i] + ko) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < WC; ++i) rw[i] = BM == 32 ? ld16_nt(wp[i] + ko) : ld16(wp[i] + ko);
  };
  auto lstore = [&](int buf) {
    char* la = lds + buf * STAGE;
    char* lw = la + AS;
#pragma unroll
    for (int i = 0; i < AC; ++i) {
      const int q = tid + 256 * i;
      st16(la + ((q >> 3) * LDT + (q & 7) * 8) * 2, ra[i]);
    }
#pragma unroll
    for (int i = 0; i < WC; ++i) {
      const int q = tid + 256 * i;
      st16(lw + ((q >> 3) * LDT + (q & 7) * 8) * 2, rw[i]);
    }
  };

  const int rb = (BM == 128 ? wid : 0) * (BM / WAVES_M);    // first tile row of this wave
  const int cb = (BM == 128 ? 0 : wid) * (BN / WAVES_N);    // first tile column of this wave
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  f32x4 accg[IT][JT], accu[DOWN ? 1 : IT][DOWN ? 1 : JT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      accg[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (!DOWN) accu[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  const int nk = K / BK;
  gload(0);
  lstore(0);
  if (nk > 1) gload(1);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* la = lds + (kt % ST) * STAGE;
    const char* lw = la + AS;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 av[IT];
#pragma unroll
      for (int i = 0; i < IT; ++i) av[i] = lds8(la + ((rb + 16 * i + fr) * LDT + 32 * ks + fk) * 2);
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        const bf16x8 bg = lds8(lw + ((cb + 16 * j + fr) * LDT + 32 * ks + fk) * 2);
#pragma unroll
        for (int i = 0; i < IT; ++i) accg[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bg, accg[i][j], 0, 0, 0);
        if constexpr (!DOWN) {
          const bf16x8 bu = lds8(lw + ((BN + cb + 16 * j + fr) * LDT + 32 * ks + fk) * 2);
#pragma unroll
          for (int i = 0; i < IT; ++i)
            accu[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bu, accu[i][j], 0, 0, 0);
        }
      }
    }
    if (kt + 1 < nk) {
      if (ST == 1) __syncthreads();   // one stage: every wave is done reading it
      lstore((kt + 1) % ST);
      if (kt + 2 < nk) gload(kt + 2);
    }
    __syncthreads();
  }

  // acc[i][j][r] = C[rb + 16 i + 4 (lane >> 4) + r][cb + 16 j + fr] (tile-local)
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rb + 16 * i + 4 * (lane >> 4) + r;
      const int idx = srow[row];
      if (idx < 0) continue;   // padding row
      const float tw = DOWN ? topk_w[idx] : 0.f;
      bf16* orow = out + (DOWN ? (int64_t)idx : prow0 + row) * N + n0 + cb + fr;
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        if constexpr (DOWN) {
          orow[16 * j] = (bf16)(tw * accg[i][j][r]);
        } else {
          const float g = accg[i][j][r];
          orow[16 * j] = (bf16)(g / (1.f + expf(-g)) * accu[i][j][r]);
        }
      }
    }
}

// ---------------------------------------------------------------------------- moe_gemm_w8
// The grouped GEMM over fp8 expert weights (W8A16): w holds e4m3fn codes, one byte each, sc one
// f32 scale per (expert, weight row) -- [E, 2 N] in gate_up mode, [E, N] in down mode.  Schedule,
// gather, scatter, tile heights and grid are those of moe_gemm_kernel; A stays bf16 in LDS.  The
// weight tile stays codes from HBM to LDS (rows of BKW + 16 bytes) and a lane expands the 8 codes
// of an MFMA operand from one 8-B LDS read (fp8_unpack8, exact).  The scales touch only the f32
// accumulators in the epilogue and are loaded ahead of the K loop.  A K that is an odd multiple
// of 64 ends the 128-code form in a half step: its upper chunks are zeros and read nothing.
template <int BM, bool DOWN>
__global__ void __launch_bounds__(256) moe_gemm_w8_kernel(const bf16* __restrict__ a, int64_t lda,
                                                          const fp8_t* __restrict__ w, const float* __restrict__ sc,
                                                          const int* __restrict__ num_tiles,
                                                          const int* __restrict__ tile_expert,
                                                          const int* __restrict__ sorted_rows,
                                                          const float* __restrict__ topk_w, int kk, int K, int N,
                                                          bf16* __restrict__ out) {
  constexpr int BKW = BM == 32 ? 128 : 64;          // K step in codes (file header: K STEP)
  constexpr int NW = DOWN ? BN : 2 * BN;            // weight rows per K step
  constexpr int LDA = BKW + 8;                      // A LDS row, bf16 elements
  constexpr int LDW = BKW + 16;                     // W LDS row, bytes (80 / 144: 16-B stores and 8-B reads stay aligned)
  constexpr int AS = BM * LDA * 2, WS = NW * LDW, STAGE = AS + WS;
  constexpr int ACR = BKW / 8, WCR = BKW / 16;      // 16-B chunks per A row (8 bf16) and per W row (16 codes)
  constexpr int AC = BM * ACR / 256, WC = NW * WCR / 256;   // chunks per thread per K step
  constexpr int WAVES_M = BM == 128 ? 4 : 1, WAVES_N = 4 / WAVES_M;
  constexpr int IT = BM / WAVES_M / 16, JT = BN / WAVES_N / 16;
  static_assert(BM == 32 || BM == 128, "tile heights");
  static_assert(2 * STAGE <= 65536 - 4 * BM, "two LDS stages");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  __shared__ int srow[BM];
  const int tile = blockIdx.y;
  if (tile >= *num_tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int e = tile_expert[tile];
  const int n0 = blockIdx.x * BN;
  const int64_t prow0 = (int64_t)tile * BM;
  if (tid < BM) srow[tid] = sorted_rows[prow0 + tid];
  __syncthreads();

  const bf16* ap[AC];
  bool aok[AC];
#pragma unroll
  for (int i = 0; i < AC; ++i) {
    const int q = tid + 256 * i, row = q / ACR, c = q % ACR;
    const int idx = srow[row];
    aok[i] = idx >= 0;
    const int64_t grow = DOWN ? prow0 + row : (aok[i] ? idx / kk : 0);
    ap[i] = a + grow * lda + c * 8;
  }
  const fp8_t* wp[WC];
  const fp8_t* wbase = w + (int64_t)e * (DOWN ? N : 2 * N) * K;
#pragma unroll
  for (int i = 0; i < WC; ++i) {
    const int q = tid + 256 * i, row = q / WCR, c = q % WCR;
    const int grow = DOWN || row < BN ? n0 + row : N + n0 + row - BN;   // gate rows, then the matching up rows
    wp[i] = wbase + (int64_t)grow * K + c * 16;
  }
  uint4 ra[AC], rw[WC];
  auto gload = [&](int kt) {
    const int ko = kt * BKW;
#pragma unroll
    for (int i = 0; i < AC; ++i) {
      const bool in = BKW == 64 || ko + ((tid + 256 * i) % ACR) * 8 < K;   // false past K in a half step
      ra[i] = aok[i] && in ? ld16(ap[i] + ko) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WC; ++i) {
      const bool in = BKW == 64 || ko + ((tid + 256 * i) % WCR) * 16 < K;
      rw[i] = !in ? make_uint4(0, 0, 0, 0) : BM == 32 ? ld16_nt(wp[i] + ko) : ld16(wp[i] + ko);
    }
  };
  auto lstore = [&](int buf) {
    char* la = lds + buf * STAGE;
    char* lw = la + AS;
#pragma unroll
    for (int i = 0; i < AC; ++i) {
      const int q = tid + 256 * i;
      st16(la + ((q / ACR) * LDA + (q % ACR) * 8) * 2, ra[i]);
    }
#pragma unroll
    for (int i = 0; i < WC; ++i) {
      const int q = tid + 256 * i;
      st16(lw + (q / WCR) * LDW + (q % WCR) * 16, rw[i]);
    }
  };

  const int rb = (BM == 128 ? wid : 0) * (BM / WAVES_M);    // first tile row of this wave
  const int cb = (BM == 128 ? 0 : wid) * (BN / WAVES_N);    // first tile column of this wave
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  // this lane's output columns are n0 + cb + 16 j + fr: their scales, once per tile
  float sg[JT], su[DOWN ? 1 : JT];
  const float* se = sc + (int64_t)e * (DOWN ? N : 2 * N) + n0 + cb + fr;
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    sg[j] = se[16 * j];
    if constexpr (!DOWN) su[j] = se[N + 16 * j];
  }
  f32x4 accg[IT][JT], accu[DOWN ? 1 : IT][DOWN ? 1 : JT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      accg[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (!DOWN) accu[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  const int nk = (K + BKW - 1) / BKW;
  gload(0);
  lstore(0);
  if (nk > 1) gload(1);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* la = lds + (kt & 1) * STAGE;
    const char* lw = la + AS;
#pragma unroll
    for (int ks = 0; ks < BKW / 32; ++ks) {
      bf16x8 av[IT];
#pragma unroll
      for (int i = 0; i < IT; ++i) av[i] = lds8(la + ((rb + 16 * i + fr) * LDA + 32 * ks + fk) * 2);
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        const bf16x8 bg = fp8_unpack8(*reinterpret_cast<const uint2*>(lw + (cb + 16 * j + fr) * LDW + 32 * ks + fk));
#pragma unroll
        for (int i = 0; i < IT; ++i) accg[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bg, accg[i][j], 0, 0, 0);
        if constexpr (!DOWN) {
          const bf16x8 bu =
              fp8_unpack8(*reinterpret_cast<const uint2*>(lw + (BN + cb + 16 * j + fr) * LDW + 32 * ks + fk));
#pragma unroll
          for (int i = 0; i < IT; ++i)
            accu[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bu, accu[i][j], 0, 0, 0);
        }
      }
    }
    if (kt + 1 < nk) {
      lstore((kt + 1) & 1);
      if (kt + 2 < nk) gload(kt + 2);
    }
    __syncthreads();
  }

  // acc[i][j][r] = C[rb + 16 i + 4 (lane >> 4) + r][cb + 16 j + fr] (tile-local), still unscaled
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rb + 16 * i + 4 * (lane >> 4) + r;
      const int idx = srow[row];
      if (idx < 0) continue;   // padding row
      const float tw = DOWN ? topk_w[idx] : 0.f;
      bf16* orow = out + (DOWN ? (int64_t)idx : prow0 + row) * N + n0 + cb + fr;
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        if constexpr (DOWN) {
          orow[16 * j] = (bf16)(tw * (accg[i][j][r] * sg[j]));
        } else {
          const float g = accg[i][j][r] * sg[j];
          orow[16 * j] = (bf16)(g / (1.f + expf(-g)) * (accu[i][j][r] * su[j]));
        }
      }
    }
}

// ---------------------------------------------------------------------------- moe_gemm_w4
// The grouped GEMM over int4 expert weights (W4A16): w holds packed 4-bit codes (two per byte, the
// word order of w4_unpack8), sc one f32 scale and zp one zero point per (expert, weight row, group
// of G input columns) -- [E, 2 N, K / G] in gate_up mode, [E, N, K / G] in down mode; G % 64 == 0.
// Schedule, gather, scatter, tile heights and grid are those of moe_gemm_kernel; A stays bf16 in
// LDS.  The MFMAs of a 64-code block accumulate into a per-group partial (gate and up each) that
// is folded into the main f32 accumulator with the lane's scale where the group ends.  A lane's
// scales (and, BM = 32, zero points) are fetched with the loads of the step in which a group
// begins and staged in registers one step ahead, per 64-code block of the step.
//   BM = 32: the weight tile stays nibbles from HBM to LDS (rows of BKW / 2 + 16 bytes); a lane
//     expands the 8 codes of an MFMA operand from one 4-B LDS read with its column's zero point.
//     A step may span several groups; a K that is no multiple of the step ends in a partial
//     step whose upper chunks are zeros and read nothing, and whose empty blocks are skipped.
//   BM = 128: the thread that carries a 16-B chunk (32 codes, inside one group) fetches the row's
//     zero point with it and expands it to 32 bf16 of q - z on the way into LDS, so the weight tile
//     has the bf16 kernel's layout and every code is decoded once, not once per wave.
template <int BM, bool DOWN>
__global__ void __launch_bounds__(256) moe_gemm_w4_kernel(const bf16* __restrict__ a, int64_t lda,
                                                          const uint8_t* __restrict__ w, const float* __restrict__ sc,
                                                          const uint8_t* __restrict__ zp,
                                                          const int* __restrict__ num_tiles,
                                                          const int* __restrict__ tile_expert,
                                                          const int* __restrict__ sorted_rows,
                                                          const float* __restrict__ topk_w, int kk, int K, int N, int G,
                                                          bf16* __restrict__ out) {
  constexpr bool EXP = BM == 128;                   // expand once per workgroup: W is bf16 of q - z in LDS
  constexpr int BKW = BM == 32 ? 256 : 64;          // K step in codes (file header: moe_gemm_w4, K STEP)
  constexpr int NH = BKW / 64;                      // 64-code blocks per step: a block lies inside one group
  constexpr int NW = DOWN ? BN : 2 * BN;            // weight rows per K step
  constexpr int LDA = BKW + 8;                      // A LDS row, bf16 elements
  constexpr int LDW = EXP ? LDA * 2 : BKW / 2 + 16; // W LDS row, bytes (bf16 of q - z, or nibbles + pad)
  constexpr int AS = BM * LDA * 2, WS = NW * LDW, STAGE = AS + WS;
  constexpr int ACR = BKW / 8, WCR = BKW / 32;      // 16-B chunks per A row (8 bf16) and per W row (32 codes)
  constexpr int AC = BM * ACR / 256;                // A chunks per thread per K step
  constexpr int WCH = NW * WCR, WC = (WCH + 255) / 256;   // W chunks per step, per thread (BM = 128 down: threads < 128)
  constexpr int WAVES_M = BM == 128 ? 4 : 1, WAVES_N = 4 / WAVES_M;
  constexpr int IT = BM / WAVES_M / 16, JT = BN / WAVES_N / 16;
  constexpr int U = DOWN ? 1 : 2;                   // gate only, or gate and up
  static_assert(BM == 32 || BM == 128, "tile heights");
  static_assert(2 * STAGE + 4 * BM <= 160 * 1024, "two LDS stages");
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  __shared__ int srow[BM];
  const int tile = blockIdx.y;
  if (tile >= *num_tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int e = tile_expert[tile];
  const int n0 = blockIdx.x * BN;
  const int NG = K / G;
  const int64_t prow0 = (int64_t)tile * BM;
  if (tid < BM) srow[tid] = sorted_rows[prow0 + tid];
  __syncthreads();

  const bf16* ap[AC];
  bool aok[AC];
#pragma unroll
  for (int i = 0; i < AC; ++i) {
    const int q = tid + 256 * i, row = q / ACR, c = q % ACR;
    const int idx = srow[row];
    aok[i] = idx >= 0;
    const int64_t grow = DOWN ? prow0 + row : (aok[i] ? idx / kk : 0);
    ap[i] = a + grow * lda + c * 8;
  }
  const int64_t erow0 = (int64_t)e * (DOWN ? N : 2 * N);   // the expert's first row in w, sc and zp
  const uint8_t* wp[WC];
  const uint8_t* zc[WC];   // BM = 128: the zero points of the chunk's row
  bool wok[WC];
#pragma unroll
  for (int i = 0; i < WC; ++i) {
    const int q = tid + 256 * i, row = q / WCR, c = q % WCR;
    wok[i] = q < WCH;
    const int grow = !wok[i] ? n0 : DOWN || row < BN ? n0 + row : N + n0 + row - BN;   // gate rows, then the matching up rows
    wp[i] = w + (erow0 + grow) * (K / 2) + c * 16;
    zc[i] = zp + (erow0 + grow) * NG;
  }
  const int rb = (BM == 128 ? wid : 0) * (BM / WAVES_M);    // first tile row of this wave
  const int cb = (BM == 128 ? 0 : wid) * (BN / WAVES_N);    // first tile column of this wave
  const int fr = lane & 15, fq = lane >> 4, fk = 8 * fq;
  // this lane's output columns are n0 + cb + 16 j + fr: gate row n, up row N + n of the expert
  const float* sp[JT][U];
  const uint8_t* zq[JT][U];
#pragma unroll
  for (int j = 0; j < JT; ++j)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = erow0 + u * N + n0 + cb + 16 * j + fr;
      sp[j][u] = sc + row * NG;
      zq[j][u] = zp + row * NG;
    }
  uint4 ra[AC], rw[WC];
  float rzc[WC];                             // BM = 128: zero point of the chunk in rw
  float rs[NH][JT][U], rz[NH][JT][U];        // fetched: per block of the step last loaded
  float cs[NH][JT][U], cz[NH][JT][U];        // staged: per block of the step in LDS
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
      for (int u = 0; u < U; ++u) rs[h][j][u] = rz[h][j][u] = 0.f;
  auto gload = [&](int kt) {
    const int ko = kt * BKW;
#pragma unroll
    for (int i = 0; i < AC; ++i) {
      const bool in = NH == 1 || ko + ((tid + 256 * i) % ACR) * 8 < K;   // false past K in a partial step
      ra[i] = aok[i] && in ? ld16(ap[i] + ko) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WC; ++i) {
      const int kc = ko + ((tid + 256 * i) % WCR) * 32;
      const bool in = wok[i] && (NH == 1 || kc < K);
      rw[i] = !in ? make_uint4(0, 0, 0, 0) : BM == 32 ? ld16_nt(wp[i] + ko / 2) : ld16(wp[i] + ko / 2);
      if constexpr (EXP) rzc[i] = in ? (float)zc[i][kc / G] : 0.f;
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int k = ko + 64 * h;
      const bool begins = k < K && k % G == 0;   // wave-uniform
      const int g = k / G;
#pragma unroll
      for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          // a block inside a group inherits from the block before it (the last one of the previous step)
          const int hp = h == 0 ? NH - 1 : h - 1;
          rs[h][j][u] = begins ? sp[j][u][g] : rs[hp][j][u];
          if constexpr (!EXP) rz[h][j][u] = begins ? (float)zq[j][u][g] : rz[hp][j][u];
        }
    }
  };
  auto lstore = [&](int buf) {
    char* la = lds + buf * STAGE;
    char* lw = la + AS;
#pragma unroll
    for (int i = 0; i < AC; ++i) {
      const int q = tid + 256 * i;
      st16(la + ((q / ACR) * LDA + (q % ACR) * 8) * 2, ra[i]);
    }
#pragma unroll
    for (int i = 0; i < WC; ++i) {
      const int q = tid + 256 * i;
      if (!wok[i]) continue;
      if constexpr (EXP) {
        const uint32_t words[4] = {rw[i].x, rw[i].y, rw[i].z, rw[i].w};
#pragma unroll
        for (int v = 0; v < 4; ++v)   // word v holds codes 8 v .. 8 v + 7 of the chunk
          st16(lw + (q / WCR) * LDW + ((q % WCR) * 32 + 8 * v) * 2,
               __builtin_bit_cast(uint4, w4_unpack8(words[v], rzc[i])));
      } else {
        st16(lw + (q / WCR) * LDW + (q % WCR) * 16, rw[i]);
      }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          cs[h][j][u] = rs[h][j][u];
          cz[h][j][u] = rz[h][j][u];
        }
  };

  f32x4 acc[IT][JT][U], grp[IT][JT][U];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
      for (int u = 0; u < U; ++u) acc[i][j][u] = grp[i][j][u] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (K + BKW - 1) / BKW;
  gload(0);
  lstore(0);
  if (nk > 1) gload(1);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* la = lds + (kt & 1) * STAGE;
    const char* lw = la + AS;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int k = kt * BKW + 64 * h;
      if (NH > 1 && k >= K) continue;   // an empty block of the partial last step (wave-uniform)
#pragma unroll
      for (int ks = 2 * h; ks < 2 * h + 2; ++ks) {
        bf16x8 av[IT];
#pragma unroll
        for (int i = 0; i < IT; ++i) av[i] = lds8(la + ((rb + 16 * i + fr) * LDA + 32 * ks + fk) * 2);
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const char* wrow = lw + (u * BN + cb + 16 * j + fr) * LDW;
            bf16x8 b;
            if constexpr (EXP) b = lds8(wrow + (32 * ks + fk) * 2);
            else b = w4_unpack8(*reinterpret_cast<const uint32_t*>(wrow + 16 * ks + 4 * fq), cz[h][j][u]);
#pragma unroll
            for (int i = 0; i < IT; ++i)
              grp[i][j][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], b, grp[i][j][u], 0, 0, 0);
          }
      }
      // the group ends with this block (K % G == 0: the last block ends one): fold its partial in with the scale
      if ((k + 64) % G == 0) {
#pragma unroll
        for (int i = 0; i < IT; ++i)
#pragma unroll
          for (int j = 0; j < JT; ++j)
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[i][j][u][r] = fmaf(grp[i][j][u][r], cs[h][j][u], acc[i][j][u][r]);
              grp[i][j][u] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
      }
    }
    if (kt + 1 < nk) {
      lstore((kt + 1) & 1);
      if (kt + 2 < nk) gload(kt + 2);
    }
    __syncthreads();
  }

  // acc[i][j][u][r] = C[rb + 16 i + 4 (lane >> 4) + r][cb + 16 j + fr] (tile-local), u = 1: the up half
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rb + 16 * i + 4 * fq + r;
      const int idx = srow[row];
      if (idx < 0) continue;   // padding row
      const float tw = DOWN ? topk_w[idx] : 0.f;
      bf16* orow = out + (DOWN ? (int64_t)idx : prow0 + row) * N + n0 + cb + fr;
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        const float g = acc[i][j][0][r];
        if constexpr (DOWN) orow[16 * j] = (bf16)(tw * g);
        else orow[16 * j] = (bf16)(g / (1.f + expf(-g)) * acc[i][j][U - 1][r]);
      }
    }
}

// ---------------------------------------------------------------------------- moe_combine
// One thread per 16-B chunk of out.
__global__ void __launch_bounds__(256) moe_combine_kernel(const bf16* __restrict__ y, const int* __restrict__ ids,
                                                          int T, int k, int E, int H, bf16* __restrict__ out,
                                                          int64_t ldo) {
  const int hc = H >> 3;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t t = g / hc;
  const int c = (int)(g % hc);
  if (t >= T) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < k; ++s) {
    if ((unsigned)ids[t * k + s] >= (unsigned)E) continue;   // a slot moe_align dropped
    float v[8];
    unpack8(ld16(y + (t * k + s) * H + c * 8), v);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += v[i];
  }
  st16(out + t * ldo + c * 8, pack8(acc));
}

// Host-side launch census (moe_launch_counts), relaxed atomics on the host only.
std::atomic<int64_t> g_route[2], g_align, g_gemm[2][2], g_combine;   // route [mfma]; gemm [BM == 128][down]
std::atomic<int64_t> g_gemm_w8[2][2];                                // the fp8-code GEMMs, likewise
std::atomic<int64_t> g_gemm_w4[2][2];                                // the int4-code GEMMs, likewise

bool aligned16(const at::Tensor& t) { return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0; }

void check_x(const char* who, const at::Tensor& x, int64_t H) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.size(1) == H && x.size(0) >= 1 &&
                  x.stride(1) == 1 && (x.size(0) == 1 || x.stride(0) % 8 == 0) && aligned16(x),
              who, ": x must be a 16-byte aligned bf16 [T >= 1, H = ", H,
              "] on the GPU with unit inner stride and a row stride that is a multiple of 8");
  TORCH_CHECK(x.size(0) < (int64_t(1) << 24), who, ": T too large");
}

// The rule between the two row-tile heights, a function of the mean rows per expert T k / E:
// from a mean of 64 rows the 128-row tile (half full or better on average), below it the
// 32-row tile, where a layer is a weight stream and short tiles waste the fewest MFMA rows.
int tile_rows(int64_t T, int64_t k, int64_t E) { return T * k >= 64 * E ? 128 : 32; }

template <int BM>
void gemm_launch(hipStream_t st, const at::Tensor& x, const at::Tensor& gate_up_w, const at::Tensor& down_w,
                 const int* meta, int64_t max_tiles, const float* wts, int k, bf16* act, bf16* y) {
  const int H = (int)x.size(1), F = (int)down_w.size(2);
  const int* tile_expert = meta + 1;
  const int* sorted_rows = meta + 1 + max_tiles;
  g_gemm[BM == 128][0].fetch_add(1, std::memory_order_relaxed);
  g_gemm[BM == 128][1].fetch_add(1, std::memory_order_relaxed);
  moe_gemm_kernel<BM, false><<<dim3(F / BN, (unsigned)max_tiles), 256, 0, st>>>(
      (const bf16*)x.data_ptr(), x.stride(0), (const bf16*)gate_up_w.data_ptr(), meta, tile_expert, sorted_rows,
      nullptr, k, H, F, act);
  moe_gemm_kernel<BM, true><<<dim3(H / BN, (unsigned)max_tiles), 256, 0, st>>>(
      act, F, (const bf16*)down_w.data_ptr(), meta, tile_expert, sorted_rows, wts, k, F, H, y);
}

// The same two launches over fp8 codes and their scales.
template <int BM>
void gemm_w8_launch(hipStream_t st, const at::Tensor& x, const at::Tensor& gate_up_w, const at::Tensor& down_w,
                    const at::Tensor& gate_up_s, const at::Tensor& down_s, const int* meta, int64_t max_tiles,
                    const float* wts, int k, bf16* act, bf16* y) {
  const int H = (int)x.size(1), F = (int)down_w.size(2);
  const int* tile_expert = meta + 1;
  const int* sorted_rows = meta + 1 + max_tiles;
  g_gemm_w8[BM == 128][0].fetch_add(1, std::memory_order_relaxed);
  g_gemm_w8[BM == 128][1].fetch_add(1, std::memory_order_relaxed);
  moe_gemm_w8_kernel<BM, false><<<dim3(F / BN, (unsigned)max_tiles), 256, 0, st>>>(
      (const bf16*)x.data_ptr(), x.stride(0), (const fp8_t*)gate_up_w.data_ptr(), gate_up_s.data_ptr<float>(), meta,
      tile_expert, sorted_rows, nullptr, k, H, F, act);
  moe_gemm_w8_kernel<BM, true><<<dim3(H / BN, (unsigned)max_tiles), 256, 0, st>>>(
      act, F, (const fp8_t*)down_w.data_ptr(), down_s.data_ptr<float>(), meta, tile_expert, sorted_rows, wts, k, F, H,
      y);
}

// The same two launches over int4 codes, their group scales and zero points; the group sizes
// are read from the scales' last dimension.
template <int BM>
void gemm_w4_launch(hipStream_t st, const at::Tensor& x, const at::Tensor& gate_up_w, const at::Tensor& down_w,
                    const at::Tensor& gate_up_s, const at::Tensor& down_s, const at::Tensor& gate_up_z,
                    const at::Tensor& down_z, const int* meta, int64_t max_tiles, const float* wts, int k, bf16* act,
                    bf16* y) {
  const int H = (int)x.size(1), F = (int)(2 * down_w.size(2));
  const int* tile_expert = meta + 1;
  const int* sorted_rows = meta + 1 + max_tiles;
  g_gemm_w4[BM == 128][0].fetch_add(1, std::memory_order_relaxed);
  g_gemm_w4[BM == 128][1].fetch_add(1, std::memory_order_relaxed);
  moe_gemm_w4_kernel<BM, false><<<dim3(F / BN, (unsigned)max_tiles), 256, 0, st>>>(
      (const bf16*)x.data_ptr(), x.stride(0), gate_up_w.data_ptr<uint8_t>(), gate_up_s.data_ptr<float>(),
      gate_up_z.data_ptr<uint8_t>(), meta, tile_expert, sorted_rows, nullptr, k, H, F, H / (int)gate_up_s.size(2), act);
  moe_gemm_w4_kernel<BM, true><<<dim3(H / BN, (unsigned)max_tiles), 256, 0, st>>>(
      act, F, down_w.data_ptr<uint8_t>(), down_s.data_ptr<float>(), down_z.data_ptr<uint8_t>(), meta, tile_expert,
      sorted_rows, wts, k, F, H, F / (int)down_s.size(2), y);
}

// Every guard of the int4 form of moe_experts: codes uint8 [E, 2F, H / 2] and [E, H, F / 2], scales
// f32 and zero points uint8 [E, rows, K / G].
void check_w4_experts(const at::Tensor& gate_up_w, const at::Tensor& down_w, const at::Tensor& gate_up_s,
                      const at::Tensor& down_s, const at::Tensor& gate_up_z, const at::Tensor& down_z) {
  TORCH_CHECK(gate_up_w.scalar_type() == at::kByte && down_w.scalar_type() == at::kByte,
              "moe_experts: with gate_up_z / down_z the expert weights must be uint8 int4 codes (two per byte), got ",
              gate_up_w.scalar_type(), " and ", down_w.scalar_type());
  TORCH_CHECK(gate_up_w.is_cuda() && down_w.is_cuda() && gate_up_w.dim() == 3 && down_w.dim() == 3 &&
                  gate_up_w.is_contiguous() && down_w.is_contiguous() && aligned16(gate_up_w) && aligned16(down_w),
              "moe_experts: int4 gate_up_w [E, 2F, H / 2] and down_w [E, H, F / 2] must be contiguous 16-byte aligned "
              "uint8 on the GPU");
  const int64_t E = gate_up_w.size(0), H = 2 * gate_up_w.size(2), F = 2 * down_w.size(2);
  const at::Tensor* ss[2] = {&gate_up_s, &down_s};
  const at::Tensor* zs[2] = {&gate_up_z, &down_z};
  const char* names[2] = {"gate_up", "down"};
  const int64_t rows[2] = {2 * F, H}, Ks[2] = {H, F};
  for (int i = 0; i < 2; ++i) {
    const at::Tensor &s = *ss[i], &z = *zs[i];
    const char* n = names[i];
    TORCH_CHECK(s.is_cuda() && z.is_cuda() && s.device() == gate_up_w.device() && z.device() == gate_up_w.device(),
                "moe_experts: ", n, "_s and ", n, "_z must be on the device of the weights");
    TORCH_CHECK(s.scalar_type() == at::kFloat, "moe_experts: ", n, "_s must be float32, got ", s.scalar_type());
    TORCH_CHECK(z.scalar_type() == at::kByte, "moe_experts: ", n, "_z must be uint8, got ", z.scalar_type());
    TORCH_CHECK(s.dim() == 3 && s.size(0) == E && s.size(1) == rows[i] && s.size(2) >= 1 && Ks[i] % s.size(2) == 0 &&
                    (Ks[i] / s.size(2)) % 64 == 0,
                "moe_experts: ", n, "_s has shape ", s.sizes(), ", expected [", E, ", ", rows[i],
                ", K / G] with a group size G that is a multiple of 64 and divides K = ", Ks[i]);
    TORCH_CHECK(z.sizes() == s.sizes(), "moe_experts: ", n, "_z has shape ", z.sizes(), ", expected the shape of ", n,
                "_s ", s.sizes());
    TORCH_CHECK(s.is_contiguous() && z.is_contiguous(), "moe_experts: ", n, "_s and ", n, "_z must be contiguous");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(s.data_ptr()) & 3) == 0, "moe_experts: ", n, "_s must be 4-byte aligned");
  }
}

}  // namespace

// The shape rule of the MoE kernels.
bool moe_supported(int64_t H, int64_t F, int64_t E, int64_t k) {
  return H >= 64 && H % 64 == 0 && F >= 64 && F % 64 == 0 && E >= 1 && E <= kMaxE && k >= 1 &&
         k <= std::min<int64_t>(E, kMaxK);
}

void moe_route(at::Tensor ids, at::Tensor wts, at::Tensor x, at::Tensor router_w, bool norm_topk) {
  TORCH_CHECK(router_w.is_cuda() && router_w.scalar_type() == at::kBFloat16 && router_w.dim() == 2 &&
                  router_w.is_contiguous() && aligned16(router_w),
              "moe_route: router_w must be a contiguous 16-byte aligned bf16 [E, H] on the GPU");
  const int64_t E = router_w.size(0), H = router_w.size(1);
  check_x("moe_route", x, H);
  const int64_t T = x.size(0);
  TORCH_CHECK(ids.dim() == 2 && ids.size(0) == T, "moe_route: topk_ids must be [T, k]");
  const int64_t k = ids.size(1);
  TORCH_CHECK(moe_supported(H, 64, E, k), "moe_route: H = ", H, ", E = ", E, ", k = ", k,
              " is outside the MoE shape rule (H % 64 == 0, E <= 256, 1 <= k <= min(E, 16))");
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kInt && ids.is_contiguous() && wts.is_cuda() &&
                  wts.scalar_type() == at::kFloat && wts.is_contiguous() && wts.sizes() == ids.sizes(),
              "moe_route: topk_ids int32 and topk_w float32, both contiguous [T, k] on the GPU");
  TORCH_CHECK(x.device() == router_w.device() && x.device() == ids.device() && x.device() == wts.device(),
              "moe_route: tensors on different devices");
  auto st = at::hip::getCurrentHIPStream();
  const bool mfma = T >= 16;
  g_route[mfma].fetch_add(1, std::memory_order_relaxed);
  if (mfma)
    moe_route_kernel<16><<<(unsigned)((T + 15) / 16), 256, 0, st>>>(
        (const bf16*)x.data_ptr(), x.stride(0), (const bf16*)router_w.data_ptr(), (int)T, (int)H, (int)E, (int)k,
        norm_topk, ids.data_ptr<int>(), wts.data_ptr<float>());
  else
    moe_route_kernel<1><<<(unsigned)T, 256, 0, st>>>((const bf16*)x.data_ptr(), x.stride(0),
                                                     (const bf16*)router_w.data_ptr(), (int)T, (int)H, (int)E,
                                                     (int)k, norm_topk, ids.data_ptr<int>(), wts.data_ptr<float>());
}

// out[t] = sum over the k slots of row t of topk_w * expert(x_t): moe_align, the two grouped
// GEMMs and moe_combine.  tile_rows_force: 0 for the rule, else 32 or 128.  With the scales
// gate_up_s f32 [E, 2F] and down_s f32 [E, H] (together or not at all) the weights are
// float8_e4m3fn codes and the W8 kernels run; without them the weights are bf16.  With the zero
// points gate_up_z / down_z as well (uint8, together or not at all, they need the scales) the
// weights are packed int4 codes uint8 [E, 2F, H / 2] and [E, H, F / 2], scales and zero points
// are [E, rows, K / G] per matrix, and the W4 kernels run.
void moe_experts(at::Tensor out, at::Tensor x, at::Tensor gate_up_w, at::Tensor down_w, at::Tensor ids,
                 at::Tensor wts, int64_t tile_rows_force, c10::optional<at::Tensor> gate_up_s,
                 c10::optional<at::Tensor> down_s, c10::optional<at::Tensor> gate_up_z,
                 c10::optional<at::Tensor> down_z) {
  TORCH_CHECK(gate_up_s.has_value() == down_s.has_value(),
              "moe_experts: gate_up_s and down_s are given together or not at all");
  TORCH_CHECK(gate_up_z.has_value() == down_z.has_value(),
              "moe_experts: gate_up_z and down_z are given together or not at all");
  const bool w4 = gate_up_z.has_value();
  TORCH_CHECK(!w4 || gate_up_s.has_value(),
              "moe_experts: the zero points gate_up_z / down_z need the scales gate_up_s / down_s");
  if (w4) check_w4_experts(gate_up_w, down_w, *gate_up_s, *down_s, *gate_up_z, *down_z);
  const bool w8 = gate_up_s.has_value() && !w4;
  const auto wt = gate_up_w.scalar_type();
  TORCH_CHECK(w4 || (wt != at::kByte && down_w.scalar_type() != at::kByte),
              "moe_experts: the expert weights hold uint8 int4 codes but no scales and zero points (gate_up_s, "
              "gate_up_z, down_s, down_z) were given");
  TORCH_CHECK(w8 || (wt != at::kFloat8_e4m3fn && down_w.scalar_type() != at::kFloat8_e4m3fn),
              "moe_experts: the expert weights hold float8_e4m3fn codes but no scales (gate_up_s, down_s) were given");
  TORCH_CHECK(w4 || !w8 || (wt == at::kFloat8_e4m3fn && down_w.scalar_type() == at::kFloat8_e4m3fn),
              "moe_experts: with gate_up_s / down_s the expert weights must be float8_e4m3fn codes, got ", wt, " and ",
              down_w.scalar_type());
  TORCH_CHECK(gate_up_w.is_cuda() && down_w.is_cuda() && (w8 || w4 || wt == at::kBFloat16) &&
                  down_w.scalar_type() == wt && gate_up_w.dim() == 3 && down_w.dim() == 3 &&
                  gate_up_w.is_contiguous() && down_w.is_contiguous() && aligned16(gate_up_w) && aligned16(down_w),
              "moe_experts: gate_up_w [E, 2F, H] and down_w [E, H, F] must be contiguous 16-byte aligned bf16 (with "
              "scales: float8_e4m3fn) on the GPU");
  const int64_t E = gate_up_w.size(0), H = (w4 ? 2 : 1) * gate_up_w.size(2), F = (w4 ? 2 : 1) * down_w.size(2);
  TORCH_CHECK(gate_up_w.size(1) == 2 * F && down_w.size(0) == E && down_w.size(1) == H,
              "moe_experts: gate_up_w ", gate_up_w.sizes(), " and down_w ", down_w.sizes(),
              " are not [E, 2F, H] and [E, H, F]");
  if (w8) {
    const at::Tensor* ss[2] = {&*gate_up_s, &*down_s};
    const char* names[2] = {"gate_up_s", "down_s"};
    const int64_t rows[2] = {2 * F, H};
    for (int i = 0; i < 2; ++i) {
      const at::Tensor& s = *ss[i];
      TORCH_CHECK(s.is_cuda() && s.device() == gate_up_w.device(), "moe_experts: ", names[i],
                  " must be on the device of the weights");
      TORCH_CHECK(s.scalar_type() == at::kFloat, "moe_experts: ", names[i], " must be float32, got ", s.scalar_type());
      TORCH_CHECK(s.dim() == 2 && s.size(0) == E && s.size(1) == rows[i], "moe_experts: ", names[i], " has shape ",
                  s.sizes(), ", expected one scale per (expert, row) [", E, ", ", rows[i], "]");
      TORCH_CHECK(s.is_contiguous(), "moe_experts: ", names[i], " must be contiguous");
      TORCH_CHECK((reinterpret_cast<uintptr_t>(s.data_ptr()) & 3) == 0, "moe_experts: ", names[i],
                  " must be 4-byte aligned");
    }
  }
  check_x("moe_experts", x, H);
  const int64_t T = x.size(0);
  TORCH_CHECK(ids.dim() == 2 && ids.size(0) == T, "moe_experts: topk_ids must be [T, k]");
  const int64_t k = ids.size(1);
  TORCH_CHECK(moe_supported(H, F, E, k), "moe_experts: H = ", H, ", F = ", F, ", E = ", E, ", k = ", k,
              " is outside the MoE shape rule (H % 64 == 0, F % 64 == 0, E <= 256, 1 <= k <= min(E, 16))");
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kInt && ids.is_contiguous() && wts.is_cuda() &&
                  wts.scalar_type() == at::kFloat && wts.is_contiguous() && wts.sizes() == ids.sizes(),
              "moe_experts: topk_ids int32 and topk_w float32, both contiguous [T, k] on the GPU");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 && out.dim() == 2 && out.size(0) == T &&
                  out.size(1) == H && out.stride(1) == 1 && (T == 1 || out.stride(0) % 8 == 0) && aligned16(out),
              "moe_experts: out must be a 16-byte aligned bf16 [T, H] with unit inner stride and a row stride that "
              "is a multiple of 8");
  for (const at::Tensor* t : {&gate_up_w, &down_w, &ids, &wts, &out})
    TORCH_CHECK(t->device() == x.device(), "moe_experts: tensors on different devices");
  TORCH_CHECK(tile_rows_force == 0 || tile_rows_force == 32 || tile_rows_force == 128,
              "moe_experts: tile_rows is 0 (the rule), 32 or 128");
  const int BM = tile_rows_force ? (int)tile_rows_force : tile_rows(T, k, E);
  const int64_t n = T * k;
  const int64_t max_tiles = (n + BM - 1) / BM + std::min(E, n);
  TORCH_CHECK(max_tiles <= 65535, "moe_experts: T k = ", n, " needs more than 65535 row tiles");
  // schedule words: num_tiles | tile_expert [max_tiles] | sorted_rows [max_tiles BM]
  at::Tensor meta = at::empty({1 + max_tiles + max_tiles * BM}, x.options().dtype(at::kInt));
  at::Tensor act = at::empty({max_tiles * BM, F}, x.options());
  at::Tensor y = at::empty({n, H}, x.options());
  auto st = at::hip::getCurrentHIPStream();
  int* mp = meta.data_ptr<int>();
  g_align.fetch_add(1, std::memory_order_relaxed);
  moe_align_kernel<<<1, 1024, 0, st>>>(ids.data_ptr<int>(), (int)n, (int)E, BM, mp, mp + 1, mp + 1 + max_tiles);
  if (w4 && BM == 32)
    gemm_w4_launch<32>(st, x, gate_up_w, down_w, *gate_up_s, *down_s, *gate_up_z, *down_z, mp, max_tiles,
                       wts.data_ptr<float>(), (int)k, (bf16*)act.data_ptr(), (bf16*)y.data_ptr());
  else if (w4)
    gemm_w4_launch<128>(st, x, gate_up_w, down_w, *gate_up_s, *down_s, *gate_up_z, *down_z, mp, max_tiles,
                        wts.data_ptr<float>(), (int)k, (bf16*)act.data_ptr(), (bf16*)y.data_ptr());
  else if (w8 && BM == 32)
    gemm_w8_launch<32>(st, x, gate_up_w, down_w, *gate_up_s, *down_s, mp, max_tiles, wts.data_ptr<float>(), (int)k,
                       (bf16*)act.data_ptr(), (bf16*)y.data_ptr());
  else if (w8)
    gemm_w8_launch<128>(st, x, gate_up_w, down_w, *gate_up_s, *down_s, mp, max_tiles, wts.data_ptr<float>(), (int)k,
                        (bf16*)act.data_ptr(), (bf16*)y.data_ptr());
  else if (BM == 32)
    gemm_launch<32>(st, x, gate_up_w, down_w, mp, max_tiles, wts.data_ptr<float>(), (int)k, (bf16*)act.data_ptr(),
                    (bf16*)y.data_ptr());
  else
    gemm_launch<128>(st, x, gate_up_w, down_w, mp, max_tiles, wts.data_ptr<float>(), (int)k, (bf16*)act.data_ptr(),
                     (bf16*)y.data_ptr());
  g_combine.fetch_add(1, std::memory_order_relaxed);
  const int64_t chunks = T * (H / 8);
  moe_combine_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, st>>>(
      (const bf16*)y.data_ptr(), ids.data_ptr<int>(), (int)T, (int)k, (int)E, (int)H, (bf16*)out.data_ptr(),
      out.stride(0));
}

// The launch census since the last reset: {"route_mfma": n, "route_dot": n, "align": n,
// "gate_up_bm32": n, "down_bm128": n, "gate_up_w8_bm32": n, "down_w8_bm128": n, "gate_up_w4_bm32": n,
// "down_w4_bm128": n, "combine": n} (keys with a zero count are left out; the w8 keys count the
// fp8-code GEMMs, the w4 keys the int4-code GEMMs).
pybind11::dict moe_launch_counts(bool reset) {
  pybind11::dict d;
  auto put = [&](const std::string& key, std::atomic<int64_t>& c) {
    const int64_t n = reset ? c.exchange(0) : c.load();
    if (n) d[pybind11::str(key)] = n;
  };
  put("route_dot", g_route[0]);
  put("route_mfma", g_route[1]);
  put("align", g_align);
  for (int b = 0; b < 2; ++b) {
    put(std::string("gate_up_bm") + (b ? "128" : "32"), g_gemm[b][0]);
    put(std::string("down_bm") + (b ? "128" : "32"), g_gemm[b][1]);
    put(std::string("gate_up_w8_bm") + (b ? "128" : "32"), g_gemm_w8[b][0]);
    put(std::string("down_w8_bm") + (b ? "128" : "32"), g_gemm_w8[b][1]);
    put(std::string("gate_up_w4_bm") + (b ? "128" : "32"), g_gemm_w4[b][0]);
    put(std::string("down_w4_bm") + (b ? "128" : "32"), g_gemm_w4[b][1]);
  }
  put("combine", g_combine);
  return d;
}
