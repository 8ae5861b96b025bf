// W8A8 projections: FP8 (OCP e4m3fn) activations times FP8 weights on the gfx950 FP8 matrix
// instruction v_mfma_scale_f32_16x16x128_f8f6f4 (both operands e4m3, E8M0 block scales 2^0).
//
//   out[m, n] = bf16(acc[m, n] * xs[m] * ws[n]),  acc = f32 sum_k code_x[m, k] * code_w[n, k]
//
// with one dynamic f32 scale per activation row (xs) and one f32 scale per weight row (ws).
//
// quantize_rows_fp8: one 256-thread workgroup per row.  A thread keeps its 16-B chunks of the
//   row (8 bf16 each, chunk c of thread t is global chunk t + 256 c) in registers between the
//   amax pass and the pack pass -- K <= 28672 is 14 chunks = 56 VGPRs -- so x is read once.
//   amax = max |f32(x)|; xs = amax / 448 (1 for a zero row); inv = 1.0f / xs; code =
//   e4m3(RNE(clamp(f32(x) * inv, -448, 448))) (fp8_pack4 of common.h); 16-B loads, 8-B stores.
//   The silu_mul mode reads gu [M, 2F] and quantises a = bf16(silu(g) * u), formed with the
//   arithmetic of silu_and_mul_kernel (activation.hip) and rounded to bf16 like it, so the
//   [M, F] intermediate never goes to memory.
//
// w8a8_gemm: tile BM x BN x 128 codes, WM x WN waves, a wave owns a (BM / WM) x (BN / WN)
//   block of 16x16 f32 accumulators:
//     BM = 64  (M <= 64):   64 x 128, 4 waves 1 x 4  (wave  64 x 32)
//     BM = 128 (M < 512):  128 x 128, 4 waves 2 x 2  (wave  64 x 64)
//     BM = 256 (M >= 512): 256 x 128, 8 waves 4 x 2  (wave  64 x 64; 2 x 48 KB of LDS)
//   STAGING: codes move global -> registers -> LDS as bytes, 16 B per lane; two LDS stages;
//   the loads of K step kt + 2 are issued right after step kt + 1's registers went to LDS and
//   are in flight during the MFMAs of step kt + 1 (the structure of w8_gemm / gemm_skinny).
//   LDS LAYOUT: one row of a stage is the 128 codes of one x or w row for this K step (128 B
//   = 8 chunks of 16 B), x rows first, then w rows.  128-B rows put every second row on the
//   same banks (64 banks x 4 B), so chunk c of row r is stored at chunk c ^ ((r >> 1) & 7)
//   (XOR swizzle, no padding): the 16 lanes of a ds_read_b128 phase -- 16 consecutive rows,
//   one logical chunk -- and the 16 lanes of a store phase -- 2 rows x 8 chunks -- each hit
//   16 distinct 16-B slots of the 256-B bank window.
//   OPERANDS: lane l of the MFMA supplies 32 codes of row (l & 15) of A and of B for K group
//   l >> 4, and holds D[4 (l >> 4) + r][l & 15].  Group g takes chunks 2g and 2g + 1 of the
//   LDS row for BOTH operands, so whatever order the instruction gives the 32 codes inside a
//   group, A and B are paired code by code and the dot product is the same.
//   SPLIT-K: where the tiles are fewer than the chip, K is cut into S <= 16 slices of whole K
//   steps (gridDim.y, any S, uneven slices allowed); a slice stores f32 partials, ALREADY
//   multiplied by xs[m] * ws[n], into workspace slabs [S, M, N] that splitk_reduce_launch sums.
//   Shape rule: N % 128 == 0, K % 128 == 0.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <atomic>
#include <string>

#include "ops.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 128;          // codes per K step = bytes per LDS row
constexpr int kQuantMaxK = 28672;

// -------------------------------------------------------------------------- quantiser
// NCH: 16-B chunks (8 elements) per thread, NCH * 256 * 8 >= K.
template <int NCH, bool SILU>
__global__ void __launch_bounds__(256) quantize_rows_kernel(const bf16* __restrict__ x, int64_t ldx, int K,
                                                            fp8_t* __restrict__ xq, float* __restrict__ xs) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t m = blockIdx.x;
  const bf16* row = x + m * ldx;
  const int nch = K >> 3;
  uint4 r[NCH];
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int q = tid + 256 * c;
    r[c] = make_uint4(0, 0, 0, 0);
    if (q < nch) {
      if constexpr (SILU) {
        float g[8], u[8], o[8];
        unpack8(ld16(row + q * 8), g);
        unpack8(ld16(row + K + q * 8), u);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = g[j] / (1.f + __expf(-g[j])) * u[j];
        r[c] = pack8(o);
      } else {
        r[c] = ld16(row + q * 8);
      }
    }
    float f[8];
    unpack8(r[c], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
  }
  amax = block_max(amax, red);
  const float s = amax > 0.f ? amax / 448.f : 1.f;
  const float inv = 1.0f / s;
  if (tid == 0) xs[m] = s;
  fp8_t* orow = xq + m * (int64_t)K;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int q = tid + 256 * c;
    if (q < nch) *reinterpret_cast<uint2*>(orow + q * 8) = fp8_pack8(__builtin_bit_cast(bf16x8, r[c]), inv);
  }
}

// ------------------------------------------------------------------------------- GEMM
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * BK + ((chunk ^ ((row >> 1) & 7)) << 4); }

template <int BM, int BN, int WM, int WN, bool PARTIAL>
__global__ void __launch_bounds__(64 * WM * WN) w8a8_gemm_kernel(const fp8_t* __restrict__ xq, const fp8_t* __restrict__ w,
                                                                 const float* __restrict__ xs, const float* __restrict__ wsc,
                                                                 int M, int N, int K, int S, bf16* __restrict__ out,
                                                                 int64_t ldo, float* __restrict__ part, int MT) {
  constexpr int NT = 64 * WM * WN;
  constexpr int STAGE = (BM + BN) * BK;          // bytes per stage
  constexpr int NC = (BM + BN) * 8 / NT;         // 16-B chunks per thread per K step
  constexpr int NCX = BM * 8 / NT;               // of which the first NCX are x chunks
  static_assert((BM * 8) % NT == 0 && (BN * 8) % NT == 0, "x / w chunks split evenly over the threads");
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = logical % MT, nt = logical / MT;
  const int m0 = mt * BM, n0 = nt * BN;
  // K steps [k0, k1) of slice blockIdx.y (S <= K / 128, host-checked: every slice has a step)
  const int nkt = K / BK;
  const int k0 = (int)((int64_t)blockIdx.y * nkt / S), k1 = (int)((int64_t)(blockIdx.y + 1) * nkt / S);
  const int nk = k1 - k0;

  // chunk i of this thread: LDS row (tid >> 3) + RS i (x rows [0, BM), w rows [BM, BM + BN)),
  // chunk (tid & 7) of that row's 128 codes; RS is a multiple of 16 rows, so the swizzle term
  // is the same for every i.  Rows past M / N are not loaded and stage zeros.
  constexpr int RS = NT / 8;
  const int r0 = tid >> 3, c = tid & 7;
  const int lo0 = lds_off(r0, c);
  // wave-uniform tile bases + one 32-bit lane offset (BM, BN <= 256 rows of K <= 2^22 bytes)
  const fp8_t* xt = xq + (int64_t)m0 * K + (int64_t)k0 * BK;
  const fp8_t* wt = w + (int64_t)n0 * K + (int64_t)k0 * BK;
  const unsigned go = (unsigned)r0 * (unsigned)K + c * 16;
  const int xrows = M - m0 - r0, wrows = N - n0 - r0;   // row RS i of this thread exists iff RS i < xrows / wrows
  uint4 rg[NC];
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      if (i < NCX)
        rg[i] = RS * i < xrows ? ld16(xt + (go + (unsigned)(RS * i) * (unsigned)K + kt * BK)) : make_uint4(0, 0, 0, 0);
      else
        rg[i] = RS * (i - NCX) < wrows ? ld16(wt + (go + (unsigned)(RS * (i - NCX)) * (unsigned)K + kt * BK))
                                       : make_uint4(0, 0, 0, 0);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NC; ++i) st16(lds + buf * STAGE + lo0 + RS * i * BK, rg[i]);
  };

  constexpr int IT = BM / WM / 16, JT = BN / WN / 16;   // 16x16 accumulators per wave: IT x JT
  const int wm = wid / WN, wn = wid % WN;
  const int fr = lane & 15, g = lane >> 4;
  // byte offsets of this lane's two chunks (2g, 2g + 1) in fragment rows: the swizzle term
  // (row >> 1) & 7 depends on fr only, because every fragment starts at a multiple of 16 rows
  const int f = (fr >> 1) & 7;
  const int aoff = (wm * (BM / WM) + fr) * BK, boff = (BM + wn * (BN / WN) + fr) * BK;
  const int c0 = ((2 * g) ^ f) << 4, c1 = ((2 * g + 1) ^ f) << 4;
  auto frag = [&](const char* base) {
    const uint4 p = ld16(base + c0), q = ld16(base + c1);
    return i32x8{(int)p.x, (int)p.y, (int)p.z, (int)p.w, (int)q.x, (int)q.y, (int)q.z, (int)q.w};
  };

  f32x4 acc[IT][JT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  lstore(0);
  if (nk > 1) gload(1);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* st = lds + (kt & 1) * STAGE;
    i32x8 b[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j) b[j] = frag(st + boff + 16 * j * BK);
    // the A fragment of row block i + 1 is read during the MFMAs of block i; the scheduling
    // barrier keeps the compiler from hoisting every A read to the top (8 fragments = 64
    // VGPRs on the 256-row tile, which would not fit beside 128 accumulator registers)
    i32x8 a = frag(st + aoff);
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      i32x8 an = a;
      if (i + 1 < IT) an = frag(st + aoff + 16 * (i + 1) * BK);
#pragma unroll
      for (int j = 0; j < JT; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b[j], acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0,
                                                                     0x7f7f7f7f);
      __builtin_amdgcn_sched_barrier(0);
      a = an;
    }
    if (kt + 1 < nk) {
      lstore((kt + 1) & 1);
      if (kt + 2 < nk) gload(kt + 2);
    }
    __syncthreads();
  }

  // acc[i][j][r] = C[(BM / WM) wm + 16 i + 4 g + r][(BN / WN) wn + 16 j + fr] (tile-local)
  const int rbase = m0 + (BM / WM) * wm + 4 * g;
#pragma unroll
  for (int j = 0; j < JT; ++j) {
    const int n = n0 + (BN / WN) * wn + 16 * j + fr;
    if (n >= N) continue;
    const float sn = wsc[n];
#pragma unroll
    for (int i = 0; i < IT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = rbase + 16 * i + r;
        if (m >= M) continue;
        const float v = acc[i][j][r] * xs[m] * sn;
        if (PARTIAL) part[((int64_t)blockIdx.y * M + m) * N + n] = v;
        else out[(int64_t)m * ldo + n] = (bf16)v;
      }
  }
}

// Host-side launch census (read through w8_launch_counts): relaxed atomics on the host only.
constexpr int kMaxS = 16, kCensusS = kMaxS + 1;
std::atomic<int64_t> g_a8_count[3][kCensusS];   // [BM: 64, 128, 256][splits]
std::atomic<int64_t> g_quant_count[2];          // [silu_mul]
constexpr int kBm[3] = {64, 128, 256};

int pick_tile(int64_t M) { return M <= 64 ? 0 : (M < 512 ? 1 : 2); }
int tile_bn(int) { return 128; }

// K slices: enough workgroups for 256 CUs (x 2 for the 256-thread tiles, which fit two to a
// CU) where the tiles alone are fewer; at least 4 K steps per slice; at most 16.
int pick_split(int64_t M, int64_t N, int64_t K) {
  const int t = pick_tile(M);
  const int64_t tiles = ((M + kBm[t] - 1) / kBm[t]) * ((N + tile_bn(t) - 1) / tile_bn(t));
  const int64_t want = (t == 2 ? 256 : 512) / std::max<int64_t>(tiles, 1);
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, K / BK / 4, (int64_t)kMaxS}));
}

bool aligned16(const at::Tensor& t) { return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0; }

// Every guard of quantize_rows_fp8; raises before anything is launched or written.
void check_quant(const at::Tensor& xq, const at::Tensor& xs, const at::Tensor& x, bool silu_mul) {
  const char* who = "quantize_rows_fp8";
  TORCH_CHECK(x.is_cuda() && xq.is_cuda() && xs.is_cuda(), who, ": GPU tensors expected");
  TORCH_CHECK(x.device() == xq.device() && x.device() == xs.device(), who, ": tensors on different devices");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, who, ": x must be bf16");
  TORCH_CHECK(xq.scalar_type() == at::kFloat8_e4m3fn, who, ": xq must be float8_e4m3fn");
  TORCH_CHECK(xs.scalar_type() == at::kFloat, who, ": xs must be float32");
  TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.stride(1) == 1 && (x.size(0) == 1 || x.stride(0) % 8 == 0), who,
              ": x must be [M, K] with unit inner stride and a row stride that is a multiple of 8");
  TORCH_CHECK(!silu_mul || x.size(1) % 2 == 0, who, ": silu_mul takes gu [M, 2F]");
  const int64_t K = silu_mul ? x.size(1) / 2 : x.size(1);
  TORCH_CHECK(K >= 8 && K % 8 == 0 && K <= kQuantMaxK, who, ": K must be a multiple of 8 and at most ", kQuantMaxK,
              ", got ", K);
  TORCH_CHECK(xq.dim() == 2 && xq.size(0) == x.size(0) && xq.size(1) == K && xq.is_contiguous(), who,
              ": xq must be contiguous [M, K]");
  TORCH_CHECK(xs.is_contiguous() && xs.numel() == x.size(0), who, ": xs must be contiguous with M elements");
  TORCH_CHECK(aligned16(x) && (reinterpret_cast<uintptr_t>(xq.data_ptr()) & 7) == 0, who,
              ": x must be 16-byte and xq 8-byte aligned");
  TORCH_CHECK(x.size(0) < (int64_t(1) << 24), who, ": dimension too large");
}

template <bool SILU>
void quant_launch(hipStream_t st, const at::Tensor& x, int M, int K, at::Tensor& xq, at::Tensor& xs) {
  const int need = (K / 8 + 255) / 256;
#define QL(n)                                                                                                        \
  quantize_rows_kernel<n, SILU><<<M, 256, 0, st>>>((const bf16*)x.data_ptr(), x.stride(0), K, (fp8_t*)xq.data_ptr(), \
                                                   xs.data_ptr<float>())
  if (need <= 1) QL(1);
  else if (need <= 2) QL(2);
  else if (need <= 4) QL(4);
  else if (need <= 8) QL(8);
  else QL(14);
#undef QL
}

struct A8Args {
  int M, N, K;
};

// Every guard of w8a8_gemm; raises before anything is launched or written.
A8Args check_a8(const at::Tensor& out, const at::Tensor& xq, const at::Tensor& xs, const at::Tensor& w,
                const at::Tensor& ws) {
  const char* who = "w8a8_gemm";
  TORCH_CHECK(xq.is_cuda() && xs.is_cuda() && w.is_cuda() && ws.is_cuda() && out.is_cuda(), who, ": GPU tensors expected");
  TORCH_CHECK(xq.device() == w.device() && xs.device() == w.device() && ws.device() == w.device() &&
                  out.device() == w.device(), who, ": tensors on different devices");
  TORCH_CHECK(xq.scalar_type() == at::kFloat8_e4m3fn, who, ": xq must be float8_e4m3fn codes");
  TORCH_CHECK(w.scalar_type() == at::kFloat8_e4m3fn, who, ": w must be float8_e4m3fn codes");
  TORCH_CHECK(xs.scalar_type() == at::kFloat && ws.scalar_type() == at::kFloat, who, ": xs and ws must be float32");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16, who, ": out must be bf16");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), who, ": w must be contiguous [N, K]");
  TORCH_CHECK(w.size(0) >= 128 && w.size(0) % 128 == 0 && w.size(1) >= BK && w.size(1) % BK == 0, who,
              ": N and K must be multiples of 128, got N = ", w.size(0), ", K = ", w.size(1));
  TORCH_CHECK(xq.dim() == 2 && xq.size(0) >= 1 && xq.size(1) == w.size(1) && xq.is_contiguous(), who,
              ": xq must be contiguous [M, K] with the K of w");
  TORCH_CHECK(xs.is_contiguous() && xs.numel() == xq.size(0), who, ": xs must be contiguous with M elements");
  TORCH_CHECK(ws.is_contiguous() && ws.numel() == w.size(0), who, ": ws must be contiguous with N = ", w.size(0),
              " elements, got ", ws.numel());
  TORCH_CHECK(out.dim() == 2 && out.size(0) == xq.size(0) && out.size(1) == w.size(0) && out.stride(1) == 1 &&
                  (out.size(0) == 1 || out.stride(0) % 4 == 0),
              who, ": out must be [M, N] with unit inner stride and a row stride that is a multiple of 4");
  TORCH_CHECK(aligned16(xq) && aligned16(w), who, ": xq and w must be 16-byte aligned");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(out.data_ptr()) & 7) == 0, who, ": out must be 8-byte aligned");
  TORCH_CHECK(xq.size(0) < (int64_t(1) << 24) && w.size(0) < (int64_t(1) << 24) && w.size(1) <= (int64_t(1) << 22), who,
              ": dimension too large");
  return A8Args{(int)xq.size(0), (int)w.size(0), (int)w.size(1)};
}

template <int T, int BM, int BN, int WM, int WN>
void a8_launch(int S, hipStream_t st, const at::Tensor& xq, const at::Tensor& xs, const at::Tensor& w,
               const at::Tensor& ws, A8Args a, at::Tensor& out, float* part) {
  const int MT = (a.M + BM - 1) / BM;
  const dim3 grid((unsigned)(MT * ((a.N + BN - 1) / BN)), (unsigned)S);
  g_a8_count[T][S].fetch_add(1, std::memory_order_relaxed);
  if (S == 1)
    w8a8_gemm_kernel<BM, BN, WM, WN, false><<<grid, 64 * WM * WN, 0, st>>>(
        (const fp8_t*)xq.data_ptr(), (const fp8_t*)w.data_ptr(), xs.data_ptr<float>(), ws.data_ptr<float>(), a.M, a.N,
        a.K, 1, (bf16*)out.data_ptr(), out.stride(0), nullptr, MT);
  else
    w8a8_gemm_kernel<BM, BN, WM, WN, true><<<grid, 64 * WM * WN, 0, st>>>(
        (const fp8_t*)xq.data_ptr(), (const fp8_t*)w.data_ptr(), xs.data_ptr<float>(), ws.data_ptr<float>(), a.M, a.N,
        a.K, S, nullptr, 0, part, MT);
}

}  // namespace

// The shape rule of the W8A8 GEMM: fp8 codes, contiguous [N, K], N % 128 == 0, K % 128 == 0
// (and K within the row quantiser's register budget).
bool w8a8_supported(const at::Tensor& w) {
  return w.dim() == 2 && w.scalar_type() == at::kFloat8_e4m3fn && w.is_contiguous() && w.size(0) >= 128 &&
         w.size(0) % 128 == 0 && w.size(1) >= BK && w.size(1) % BK == 0 && w.size(1) <= kQuantMaxK;
}

// Workspace bytes that suffice for w8a8_gemm at every row count 1..M with automatic splits.
// Within one tile count the automatic S is constant, so S * m * N peaks at the multiples of
// 64 rows and at M itself.
int64_t w8a8_gemm_workspace(int64_t M, int64_t N, int64_t K) {
  TORCH_CHECK(M >= 1 && N >= 128 && K >= BK, "w8a8_gemm_workspace: M >= 1, N >= 128, K >= 128");
  int64_t best = 0;
  auto take = [&](int64_t m) {
    const int S = pick_split(m, N, K);
    if (S > 1) best = std::max(best, (int64_t)S * m * N * 4);
  };
  take(M);
  for (int64_t m = 64; m < M && m <= 256 * 256; m += 64) take(m);   // 256 tiles and more never split
  return best;
}

void quantize_rows_fp8(at::Tensor xq, at::Tensor xs, at::Tensor x, bool silu_mul) {
  check_quant(xq, xs, x, silu_mul);
  const int M = (int)x.size(0), K = (int)xq.size(1);
  auto st = at::hip::getCurrentHIPStream();
  g_quant_count[silu_mul].fetch_add(1, std::memory_order_relaxed);
  if (silu_mul) quant_launch<true>(st, x, M, K, xq, xs);
  else quant_launch<false>(st, x, M, K, xq, xs);
}

void w8a8_gemm(at::Tensor out, at::Tensor xq, at::Tensor xs, at::Tensor w, at::Tensor ws, at::Tensor workspace,
               int64_t splits_force) {
  const A8Args a = check_a8(out, xq, xs, w, ws);
  TORCH_CHECK(splits_force >= 0, "w8a8_gemm: splits >= 0 (0: automatic)");
  const int S = splits_force > 0 ? (int)std::min<int64_t>({splits_force, (int64_t)a.K / BK, (int64_t)kMaxS})
                                 : pick_split(a.M, a.N, a.K);
  float* part = nullptr;
  if (S > 1) {
    TORCH_CHECK(workspace.is_cuda() && workspace.device() == w.device() && workspace.scalar_type() == at::kFloat &&
                    workspace.is_contiguous() && workspace.numel() >= (int64_t)S * a.M * a.N,
                "w8a8_gemm: workspace must be a contiguous float32 tensor of at least splits * M * N = ",
                (int64_t)S * a.M * a.N, " elements on the device of w");
    TORCH_CHECK(aligned16(workspace), "w8a8_gemm: workspace must be 16-byte aligned");
    part = workspace.data_ptr<float>();
  }
  auto st = at::hip::getCurrentHIPStream();
  switch (pick_tile(a.M)) {
    case 0: a8_launch<0, 64, 128, 1, 4>(S, st, xq, xs, w, ws, a, out, part); break;
    case 1: a8_launch<1, 128, 128, 2, 2>(S, st, xq, xs, w, ws, a, out, part); break;
    default: a8_launch<2, 256, 128, 4, 2>(S, st, xq, xs, w, ws, a, out, part); break;
  }
  if (S > 1) splitk_reduce_launch(part, S, a.M, a.N, (bf16*)out.data_ptr(), out.stride(0), st);
}

// The W8A8 route: quantise the rows of x (bf16 [M, K]), then the FP8 GEMM.
void linear_w8a8(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor ws, at::Tensor workspace,
                 int64_t splits_force) {
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1), "linear_w8a8: x must be [M, K] with the K of w");
  TORCH_CHECK(w8a8_supported(w), "linear_w8a8: w must be contiguous float8_e4m3fn [N, K] with N % 128 == 0, K % 128 "
              "== 0 and K <= ", kQuantMaxK);
  at::Tensor xq = at::empty({x.size(0), x.size(1)}, x.options().dtype(at::kFloat8_e4m3fn));
  at::Tensor xs = at::empty({x.size(0)}, x.options().dtype(at::kFloat));
  // both guards first: nothing is written unless the whole route is valid
  check_quant(xq, xs, x, false);
  check_a8(out, xq, xs, w, ws);
  quantize_rows_fp8(xq, xs, x, false);
  w8a8_gemm(out, xq, xs, w, ws, workspace, splits_force);
}

// The W8A8 part of the launch census (w8_launch_counts): {"a8_bm128_s2": n, "quant": n, ...}.
void w8a8_launch_counts(pybind11::dict& d, bool reset) {
  const char* qn[2] = {"quant", "quant_silu"};
  for (int q = 0; q < 2; ++q) {
    const int64_t n = reset ? g_quant_count[q].exchange(0) : g_quant_count[q].load();
    if (n) d[pybind11::str(qn[q])] = n;
  }
  for (int t = 0; t < 3; ++t)
    for (int s = 0; s < kCensusS; ++s) {
      const int64_t n = reset ? g_a8_count[t][s].exchange(0) : g_a8_count[t][s].load();
      if (n) d[pybind11::str("a8_bm" + std::to_string(kBm[t]) + "_s" + std::to_string(s))] = n;
    }
}
