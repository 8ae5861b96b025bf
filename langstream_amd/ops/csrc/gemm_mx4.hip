// MXFP4 projections (W4A8): FP8 (OCP e4m3fn) activation rows times OCP MXFP4 weights on the gfx950
// block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 with A = e4m3 and B = e2m1.
//
//   out[m, n] = bf16(xs[m] * sum_b 2^(s[n, b] - 127) * sum_{k in b} xq[m, k] * value(q[n, k]))
//
// xq [M, K] e4m3 codes and xs [M] f32 come from quantize_rows_fp8 (gemm_w8a8.hip).  A weight is
// the pair of ops/reference.py quantize_weight_mxfp4: codes uint8 [N, K / 2], byte j of a row =
// q[2j] | q[2j + 1] << 4 (e2m1: bit 3 sign, magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6), and scales
// uint8 [N, K / 32], E8M0, one per block b of 32 input columns.  The codes go from memory into
// the MFMA operand as they are (no expansion in registers) and the instruction applies the
// block scale inside the multiply; both are powers of two, so only the summation order differs
// from the reference.
//
// OPERAND ORDER (CDNA4 ISA, V_MFMA_SCALE_F32_16X16X128_F8F6F4; lane l, row / column l & 15,
//   g = l >> 4).  The two operand widths do NOT cover the same K elements per lane:
//   - an 8-bit operand is 8 VGPRs in two halves: VGPRs 0..3 hold K = 16 g .. 16 g + 15 and VGPRs
//     4..7 hold K = 64 + 16 g .. 64 + 16 g + 15 (byte j & 3 of VGPR j >> 2 within a half): the
//     instruction is two K = 64 halves, each split 16 per lane group;
//   - a 4-bit operand is 4 VGPRs holding the 32 CONSECUTIVE elements K = 32 g .. 32 g + 31,
//     element j in bits 4 (j & 7) .. + 3 of VGPR j >> 3: memory order for the nibble order above;
//   - the lane's B scale (byte opsel of a VGPR, here byte 0) multiplies the products of the lane's
//     own B elements, so with a 4-bit B an MX block IS a lane's group: byte g of the aligned dword
//     s[n, 4 kt .. 4 kt + 3], one v_lshrrev per fragment and K step, no repacked layout.
//   So A of lane (fr, g) is the 16-B chunks g and g + 4 of an x row's 128-B K step (NOT chunks 2 g
//   and 2 g + 1, which w8a8_gemm may use because there both operands are 8-bit and permuted
//   alike), and B is chunk g of a w row's 64-B K step.  The A scale is 2^0 (0x7f), so which K
//   elements an A scale would cover does not matter.  The lane holds D[4 g + r][l & 15], r = 0..3.
//   test_mx4_every_code_every_position pins all of this.
//
// mx4_gemm (rows > 16): tile BM x 128 x 128 codes with the row thresholds and wave grids of
//   w8a8_gemm (BM = 64: 4 waves 1 x 4; 128: 2 x 2; 256: 8 waves 4 x 2).  Two LDS stages; the
//   global loads of K step kt + 2 are issued after step kt + 1's registers went to LDS and are in
//   flight during the MFMAs of step kt + 1.  A stage holds BM x rows of 128 B, 128 w rows of
//   64 B and 128 scale dwords.
//   X ROWS: chunk c (16 B) of row r at chunk c ^ ((r >> 1) & 7), as in w8a8_gemm.
//   W ROWS: 64-B rows put every FOURTH row on the same banks (64 banks x 4 B = 256 B = 4 rows),
//   so chunk c of row r is stored at chunk c ^ ((r >> 2) & 3).  A ds_read_b128 phase is 16
//   lanes = 16 consecutive rows 16 a + i, one logical chunk g: the slot in the 256-B window is
//   4 (i & 3) + (g ^ (i >> 2)), a bijection of i, so the 16 lanes hit 16 distinct 16-B slots.
//   A store phase is 16 lanes = 4 consecutive rows (one value of r >> 2) x 4 chunks: slot
//   4 (r & 3) + (c ^ const), again 16 distinct slots.  No padding.
//   SCALES: thread t < 128 loads the dword of w row t; a fragment reads 16 consecutive dwords
//   (the 4 lanes of a row share an address: broadcast).
//   SPLIT-K: the rule of w8a8_gemm (S <= 16 slices of whole K steps, uneven allowed).  A slice
//   stores its RAW f32 accumulators into workspace slabs [S, M, N]; mx4_reduce_kernel sums the
//   slabs and multiplies by xs[m] once.  Slabs that were already multiplied by xs[m] (the scheme of
//   w8a8_gemm with splitk_reduce_launch) round every partial product, and where the slices cancel
//   to an exact zero they leave a residue of |partial| * xs * 2^-24, above the project's absolute
//   floor of 1e-6 for xs near 1; summing first gives the unsplit result whenever the partial sums
//   are exact.
//
// mx4_skinny (rows <= 16, the decode form): no LDS for weights.  A workgroup of 4 waves owns 16
//   weight rows and the K steps of its slice; wave v takes steps v, v + 4, ... of every chunk of
//   16 steps.  The B operand of a step is ONE non-temporal 16-B global load per lane (row
//   l & 15, bytes 64 kt + 16 g ..) landing in the operand registers, its scale one 4-B load.
//   The 4 loads of a wave's steps in a chunk are issued before the x rows of the chunk are
//   staged, so they are in flight across the staging and the barrier (depth 4: 4 KB per wave;
//   the compiler reports 72 VGPRs, so registers allow 7 waves per SIMD and the 32 KB of LDS set
//   the occupancy: 5 workgroups = 20 waves = 80 KB of weight bytes in flight per CU).  The <= 16 x rows of a chunk
//   (16 steps x 16 rows x 128 B = 32 KB, rows past M zero, x-row swizzle) are staged once per
//   workgroup.  The 4 waves combine their accumulators through LDS; above that, slabs and
//   mx4_reduce_kernel where N / 16 workgroups cannot fill the chip.
//
// Shape rule: N % 128 == 0, K % 128 == 0, K <= 28672 (the row quantiser's bound).
// Compiled with the default flags: the only f32 VALU work is the epilogue multiply.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <atomic>
#include <string>

#include "ops.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 128;   // codes per K step: 128 B of an x row, 64 B of a w row, 4 scale bytes
constexpr int BN = 128;   // weight rows per tile
constexpr int kQuantMaxK = 28672;
constexpr int kSkinnyM = 16;
constexpr int XCH = 16;   // K steps of x the skinny kernel stages at a time

__device__ __forceinline__ int x_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int w_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

// one block-scaled MFMA: A = 32 e4m3 codes (scale 2^0), B = 32 e2m1 codes in 16 B with the E8M0
// scale in byte 0 of sb
__device__ __forceinline__ f32x4 mfma_mx4(i32x8 a, uint4 b, f32x4 acc, uint32_t sb) {
  const i32x8 bb{(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, bb, acc, 0 /*A e4m3*/, 4 /*B e2m1*/, 0, 0x7f7f7f7f, 0,
                                                          (int)sb);
}

// the A operand of lane (fr, g): chunks g and g + 4 (swizzled: c0, c1) of an x row's K step
__device__ __forceinline__ i32x8 x_frag(const char* rowp, int c0, int c1) {
  const uint4 p = ld16(rowp + c0), q = ld16(rowp + c1);
  return i32x8{(int)p.x, (int)p.y, (int)p.z, (int)p.w, (int)q.x, (int)q.y, (int)q.z, (int)q.w};
}

// ------------------------------------------------------------------------------- tiled
template <int BM, int WM, int WN, bool PARTIAL>
__global__ void __launch_bounds__(64 * WM * WN) mx4_gemm_kernel(const fp8_t* __restrict__ xq, const uint8_t* __restrict__ w,
                                                                const uint8_t* __restrict__ sc, const float* __restrict__ xs,
                                                                int M, int N, int K, int S, bf16* __restrict__ out,
                                                                int64_t ldo, float* __restrict__ part, int MT) {
  constexpr int NT = 64 * WM * WN;
  constexpr int XB = BM * 128, WB = BN * 64;     // bytes of the x rows and of the w rows of a stage
  constexpr int STAGE = XB + WB + BN * 4;        // + the scale dwords
  constexpr int NCX = BM * 8 / NT, NCW = BN * 4 / NT;   // 16-B chunks per thread per K step
  static_assert((BM * 8) % NT == 0 && (BN * 4) % NT == 0 && NT >= BN, "chunks split evenly over the threads");
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = logical % MT, nt = logical / MT;
  const int m0 = mt * BM, n0 = nt * BN;
  // K steps [k0, k1) of slice blockIdx.y (S <= K / 128, host-checked: every slice has a step)
  const int nkt = K / BK;
  const int k0 = (int)((int64_t)blockIdx.y * nkt / S), k1 = (int)((int64_t)(blockIdx.y + 1) * nkt / S);
  const int nk = k1 - k0;

  // x chunk i of this thread: row (tid >> 3) + (NT / 8) i, chunk tid & 7; w chunk i: row
  // (tid >> 2) + (NT / 4) i, chunk tid & 3.  Both row steps are multiples of 16, so the swizzle
  // terms do not depend on i.  Rows past M stage zeros; N % 128 == 0, so every w row exists.
  constexpr int RSX = NT / 8, RSW = NT / 4;
  const int xr = tid >> 3, xc = tid & 7, wr = tid >> 2, wc = tid & 3;
  const int xlo = x_off(xr, xc), wlo = XB + w_off(wr, wc);
  const fp8_t* xt = xq + (int64_t)m0 * K + (int64_t)k0 * BK;
  const uint8_t* wt = w + (int64_t)n0 * (K / 2) + (int64_t)k0 * (BK / 2);
  const unsigned xgo = (unsigned)xr * (unsigned)K + xc * 16;
  const unsigned wgo = (unsigned)wr * (unsigned)(K / 2) + wc * 16;
  const uint8_t* st_ = sc + (int64_t)(n0 + (tid & (BN - 1))) * (K / 32) + (int64_t)k0 * 4;
  const int xrows = M - m0 - xr;   // row RSX i of this thread exists iff RSX i < xrows
  uint4 rx[NCX], rw[NCW];
  uint32_t rs = 0;
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NCX; ++i)
      rx[i] = RSX * i < xrows ? ld16(xt + (xgo + (unsigned)(RSX * i) * (unsigned)K + kt * BK)) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NCW; ++i) rw[i] = ld16(wt + (wgo + (unsigned)(RSW * i) * (unsigned)(K / 2) + kt * (BK / 2)));
    if (tid < BN) rs = *reinterpret_cast<const uint32_t*>(st_ + kt * 4);
  };
  auto lstore = [&](int buf) {
    char* s = lds + buf * STAGE;
#pragma unroll
    for (int i = 0; i < NCX; ++i) st16(s + xlo + RSX * i * 128, rx[i]);
#pragma unroll
    for (int i = 0; i < NCW; ++i) st16(s + wlo + RSW * i * 64, rw[i]);
    if (tid < BN) *reinterpret_cast<uint32_t*>(s + XB + WB + tid * 4) = rs;
  };

  constexpr int IT = BM / WM / 16, JT = BN / WN / 16;   // 16x16 accumulators per wave: IT x JT
  const int wm = wid / WN, wn = wid % WN;
  const int fr = lane & 15, g = lane >> 4;
  // every fragment starts at a multiple of 16 rows, so the swizzle terms depend on fr only
  const int fx = (fr >> 1) & 7;
  const int aoff = (wm * (BM / WM) + fr) * 128;
  const int c0 = (g ^ fx) << 4, c1 = ((g + 4) ^ fx) << 4;
  const int brow = wn * (BN / WN) + fr;
  const int boff = XB + brow * 64 + ((g ^ ((fr >> 2) & 3)) << 4), soff = XB + WB + brow * 4;

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
    uint4 b[JT];
    uint32_t sb[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      b[j] = ld16(st + boff + 16 * j * 64);
      sb[j] = *reinterpret_cast<const uint32_t*>(st + soff + 16 * j * 4) >> (8 * g);
    }
    // the A fragment of row block i + 1 is read during the MFMAs of block i (see w8a8_gemm)
    i32x8 a = x_frag(st + aoff, c0, c1);
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      i32x8 an = a;
      if (i + 1 < IT) an = x_frag(st + aoff + 16 * (i + 1) * 128, c0, c1);
#pragma unroll
      for (int j = 0; j < JT; ++j) acc[i][j] = mfma_mx4(a, b[j], acc[i][j], sb[j]);
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
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = rbase + 16 * i + r;
      if (m >= M) continue;
      const float sm = xs[m];
#pragma unroll
      for (int j = 0; j < JT; ++j) {
        const int n = n0 + (BN / WN) * wn + 16 * j + fr;
        if (PARTIAL) part[((int64_t)blockIdx.y * M + m) * N + n] = acc[i][j][r];
        else out[(int64_t)m * ldo + n] = (bf16)(acc[i][j][r] * sm);
      }
    }
}

// ------------------------------------------------------------------------------ skinny
template <bool PARTIAL>
__global__ void __launch_bounds__(256) mx4_skinny_kernel(const fp8_t* __restrict__ xq, const uint8_t* __restrict__ w,
                                                         const uint8_t* __restrict__ sc, const float* __restrict__ xs,
                                                         int M, int N, int K, int S, bf16* __restrict__ out, int64_t ldo,
                                                         float* __restrict__ part) {
  constexpr int STEP = 16 * 128;   // bytes of the 16 x rows of one K step
  __shared__ __attribute__((aligned(1024))) char lds[XCH * STEP];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nkt = K / BK;
  const int k0 = (int)((int64_t)blockIdx.y * nkt / S), k1 = (int)((int64_t)(blockIdx.y + 1) * nkt / S);
  const uint8_t* wrow = w + (int64_t)(n0 + fr) * (K / 2) + 16 * g;
  const uint8_t* srow = sc + (int64_t)(n0 + fr) * (K / 32);
  // staging: chunk q = tid + 256 i of a chunk of steps: step q >> 7, row (q >> 3) & 15, 16-B chunk q & 7
  const int sr = (tid >> 3) & 15, scn = tid & 7;
  const fp8_t* xrow = xq + (int64_t)sr * K + scn * 16;
  const int slo = x_off(sr, scn);
  const int fx = (fr >> 1) & 7;
  const int aoff = fr * 128, c0 = (g ^ fx) << 4, c1 = ((g + 4) ^ fx) << 4;

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kc = k0; kc < k1; kc += XCH) {
    const int nst = min(XCH, k1 - kc);
    uint4 b[XCH / 4];
    uint32_t sb[XCH / 4];
#pragma unroll
    for (int j = 0; j < XCH / 4; ++j) {
      const int kt = kc + wid + 4 * j;
      b[j] = make_uint4(0, 0, 0, 0);
      sb[j] = 0;
      if (wid + 4 * j < nst) {
        b[j] = ld16_nt(wrow + (int64_t)kt * 64);
        sb[j] = *reinterpret_cast<const uint32_t*>(srow + kt * 4);
      }
    }
#pragma unroll
    for (int i = 0; i < XCH * 128 / 256; ++i) {
      const int step = 2 * i + (tid >> 7);
      if (step < nst)
        st16(lds + step * STEP + slo, sr < M ? ld16(xrow + (int64_t)(kc + step) * BK) : make_uint4(0, 0, 0, 0));
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < XCH / 4; ++j)
      if (wid + 4 * j < nst)
        acc = mfma_mx4(x_frag(lds + (wid + 4 * j) * STEP + aoff, c0, c1), b[j], acc, sb[j] >> (8 * g));
    __syncthreads();   // every wave is done with the stage before the next chunk (or the combine) overwrites it
  }

  // the 4 waves split K: combine through LDS, wave 0 stores.  acc[r] = C[4 g + r][n0 + fr]
  f32x4* red = reinterpret_cast<f32x4*>(lds);
  red[tid] = acc;
  __syncthreads();
  if (wid != 0) return;
  const f32x4 t = (red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]);
  const int n = n0 + fr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 4 * g + r;
    if (m >= M) continue;
    if (PARTIAL) part[((int64_t)blockIdx.y * M + m) * N + n] = t[r];
    else out[(int64_t)m * ldo + n] = (bf16)(t[r] * xs[m]);
  }
}

// ------------------------------------------------------------------------------ split-K
// out[m, n] = bf16(xs[m] * sum_s part[s, m, n]): 4 columns per thread (N % 128 == 0, so a thread
// stays in one row), 16-B loads, one 8-B store.
__global__ void __launch_bounds__(256) mx4_reduce_kernel(const float* __restrict__ part, int S, int M, int N,
                                                         const float* __restrict__ xs, bf16* __restrict__ out,
                                                         int64_t ldo) {
  const int64_t idx = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t total = (int64_t)M * N;
  if (idx >= total) return;
  const int m = (int)(idx / N), n = (int)(idx - (int64_t)m * N);
  f32x4 a = *reinterpret_cast<const f32x4*>(part + idx);
#pragma unroll 4
  for (int s = 1; s < S; ++s) a += *reinterpret_cast<const f32x4*>(part + (int64_t)s * total + idx);
  a *= xs[m];
  *reinterpret_cast<bf16x4*>(out + (int64_t)m * ldo + n) = bf16x4{(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3]};
}

// Host-side launch census (the keys mx4_launch_counts adds to w8_launch_counts).
constexpr int kMaxS = 16, kCensusS = kMaxS + 1;
std::atomic<int64_t> g_mx4_count[4][kCensusS];   // [skinny, BM 64, 128, 256][splits]
constexpr int kBm[3] = {64, 128, 256};

int pick_tile(int64_t M) { return M <= 64 ? 0 : (M < 512 ? 1 : 2); }

// The K slices of the tiled form: pick_split of w8a8_gemm (enough workgroups for 256 CUs, x 2
// for the 256-thread tiles; at least 4 K steps per slice; at most 16).  The skinny form has
// N / 16 workgroups of 4 waves, five to a CU: slices until there are 1024, under the same bounds.
int pick_split(int64_t M, int64_t N, int64_t K) {
  int64_t want;
  if (M <= kSkinnyM) {
    want = 1024 / std::max<int64_t>(N / 16, 1);
  } else {
    const int t = pick_tile(M);
    const int64_t tiles = ((M + kBm[t] - 1) / kBm[t]) * (N / BN);
    want = (t == 2 ? 256 : 512) / std::max<int64_t>(tiles, 1);
  }
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, K / BK / 4, (int64_t)kMaxS}));
}

bool aligned16(const at::Tensor& t) { return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0; }

struct Mx4Args {
  int M, N, K;
};

bool codes_ok(const at::Tensor& w) {
  return w.dim() == 2 && w.scalar_type() == at::kByte && w.is_contiguous() && w.size(0) >= BN && w.size(0) % BN == 0 &&
         w.size(1) >= BK / 2 && w.size(1) % (BK / 2) == 0 && 2 * w.size(1) <= kQuantMaxK;
}

// Every guard of mx4_gemm; raises before anything is launched or written.
Mx4Args check_mx4(const at::Tensor& out, const at::Tensor& xq, const at::Tensor& xs, const at::Tensor& w,
                  const at::Tensor& s) {
  const char* who = "mx4_gemm";
  TORCH_CHECK(xq.is_cuda() && xs.is_cuda() && w.is_cuda() && s.is_cuda() && out.is_cuda(), who, ": GPU tensors expected");
  TORCH_CHECK(xq.device() == w.device() && xs.device() == w.device() && s.device() == w.device() &&
                  out.device() == w.device(), who, ": tensors on different devices");
  TORCH_CHECK(xq.scalar_type() == at::kFloat8_e4m3fn, who, ": xq must be float8_e4m3fn codes");
  TORCH_CHECK(w.scalar_type() == at::kByte && s.scalar_type() == at::kByte, who,
              ": w (packed e2m1 codes) and s (E8M0 block scales) must be uint8");
  TORCH_CHECK(xs.scalar_type() == at::kFloat, who, ": xs must be float32");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16, who, ": out must be bf16");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), who, ": w must be contiguous [N, K / 2]");
  TORCH_CHECK(codes_ok(w), who, ": N and K must be multiples of 128 and K at most ", kQuantMaxK, ", got N = ", w.size(0),
              ", K = ", 2 * w.size(1));
  const int64_t N = w.size(0), K = 2 * w.size(1);
  TORCH_CHECK(s.dim() == 2 && s.size(0) == N && s.size(1) == K / 32 && s.is_contiguous(), who,
              ": s must be contiguous [N, K / 32] = [", N, ", ", K / 32, "], got ", s.sizes());
  TORCH_CHECK(xq.dim() == 2 && xq.size(0) >= 1 && xq.size(1) == K && xq.is_contiguous(), who,
              ": xq must be contiguous [M, K] with the K of w");
  TORCH_CHECK(xs.is_contiguous() && xs.numel() == xq.size(0), who, ": xs must be contiguous with M elements");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == xq.size(0) && out.size(1) == N && out.stride(1) == 1 &&
                  (out.size(0) == 1 || out.stride(0) % 4 == 0),
              who, ": out must be [M, N] with unit inner stride and a row stride that is a multiple of 4");
  TORCH_CHECK(aligned16(xq) && aligned16(w), who, ": xq and w must be 16-byte aligned");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(s.data_ptr()) & 3) == 0, who, ": s must be 4-byte aligned");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(out.data_ptr()) & 7) == 0, who, ": out must be 8-byte aligned");
  TORCH_CHECK(xq.size(0) < (int64_t(1) << 24) && N < (int64_t(1) << 24), who, ": dimension too large");
  return Mx4Args{(int)xq.size(0), (int)N, (int)K};
}

// The K slices of a call (forced: clamped to the K steps and to 16) and the guard of the workspace
// their partials need.
int check_splits(const char* who, Mx4Args a, int64_t splits_force, const at::Tensor& workspace, const at::Tensor& w) {
  TORCH_CHECK(splits_force >= 0, who, ": splits >= 0 (0: automatic)");
  const int S = splits_force > 0 ? (int)std::min<int64_t>({splits_force, (int64_t)a.K / BK, (int64_t)kMaxS})
                                 : pick_split(a.M, a.N, a.K);
  if (S > 1) {
    TORCH_CHECK(workspace.is_cuda() && workspace.device() == w.device() && workspace.scalar_type() == at::kFloat &&
                    workspace.is_contiguous() && workspace.numel() >= (int64_t)S * a.M * a.N,
                who, ": workspace must be a contiguous float32 tensor of at least splits * M * N = ",
                (int64_t)S * a.M * a.N, " elements on the device of w");
    TORCH_CHECK(aligned16(workspace), who, ": workspace must be 16-byte aligned");
  }
  return S;
}

// The guards of linear_mxfp4 on x and w: the shape agreement, and what quantize_rows_fp8 asks of its
// input (it runs them again itself; here they run before anything is launched).
void check_rows(const at::Tensor& x, const at::Tensor& w, bool silu_mul) {
  const char* who = "linear_mxfp4";
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(0) >= 1 && x.size(1) == (silu_mul ? 4 : 2) * w.size(1), who,
              ": x must be [M, ", silu_mul ? "2 K" : "K", "] with the K of w");
  TORCH_CHECK(codes_ok(w), who, ": w must be contiguous uint8 [N, K / 2] with N % 128 == 0, K % 128 == 0 and K <= ",
              kQuantMaxK);
  TORCH_CHECK(x.is_cuda() && x.device() == w.device() && x.scalar_type() == at::kBFloat16, who,
              ": x must be bf16 on the device of w");
  TORCH_CHECK(x.stride(1) == 1 && (x.size(0) == 1 || x.stride(0) % 8 == 0) && aligned16(x), who,
              ": x must be 16-byte aligned with unit inner stride and a row stride that is a multiple of 8");
}

template <int T, int BM, int WM, int WN>
void mx4_launch(int S, hipStream_t st, const at::Tensor& xq, const at::Tensor& xs, const at::Tensor& w,
                const at::Tensor& s, Mx4Args a, at::Tensor& out, float* part) {
  const int MT = (a.M + BM - 1) / BM;
  const dim3 grid((unsigned)(MT * (a.N / BN)), (unsigned)S);
  g_mx4_count[1 + T][S].fetch_add(1, std::memory_order_relaxed);
  if (S == 1)
    mx4_gemm_kernel<BM, WM, WN, false><<<grid, 64 * WM * WN, 0, st>>>(
        (const fp8_t*)xq.data_ptr(), w.data_ptr<uint8_t>(), s.data_ptr<uint8_t>(), xs.data_ptr<float>(), a.M, a.N, a.K, 1,
        (bf16*)out.data_ptr(), out.stride(0), nullptr, MT);
  else
    mx4_gemm_kernel<BM, WM, WN, true><<<grid, 64 * WM * WN, 0, st>>>(
        (const fp8_t*)xq.data_ptr(), w.data_ptr<uint8_t>(), s.data_ptr<uint8_t>(), xs.data_ptr<float>(), a.M, a.N, a.K, S,
        nullptr, 0, part, MT);
}

void skinny_launch(int S, hipStream_t st, const at::Tensor& xq, const at::Tensor& xs, const at::Tensor& w,
                   const at::Tensor& s, Mx4Args a, at::Tensor& out, float* part) {
  const dim3 grid((unsigned)(a.N / 16), (unsigned)S);
  g_mx4_count[0][S].fetch_add(1, std::memory_order_relaxed);
  if (S == 1)
    mx4_skinny_kernel<false><<<grid, 256, 0, st>>>((const fp8_t*)xq.data_ptr(), w.data_ptr<uint8_t>(),
                                                   s.data_ptr<uint8_t>(), xs.data_ptr<float>(), a.M, a.N, a.K, 1,
                                                   (bf16*)out.data_ptr(), out.stride(0), nullptr);
  else
    mx4_skinny_kernel<true><<<grid, 256, 0, st>>>((const fp8_t*)xq.data_ptr(), w.data_ptr<uint8_t>(),
                                                  s.data_ptr<uint8_t>(), xs.data_ptr<float>(), a.M, a.N, a.K, S, nullptr, 0,
                                                  part);
}

}  // namespace

// The shape rule of the MXFP4 kernels: packed e2m1 codes, contiguous uint8 [N, K / 2], N % 128 == 0,
// K % 128 == 0, K within the row quantiser's register budget.
bool mx4_supported(const at::Tensor& w) { return codes_ok(w); }

// Workspace bytes that suffice for mx4_gemm at every row count 1..M with automatic splits.  Within
// one form and tile count the automatic S is constant, so S * m * N peaks at 16 rows (skinny), at
// the multiples of 64 rows and at M itself.
int64_t mx4_gemm_workspace(int64_t M, int64_t N, int64_t K) {
  TORCH_CHECK(M >= 1 && N >= BN && K >= BK, "mx4_gemm_workspace: M >= 1, N >= 128, K >= 128");
  int64_t best = 0;
  auto take = [&](int64_t m) {
    const int S = pick_split(m, N, K);
    if (S > 1) best = std::max(best, (int64_t)S * m * N * 4);
  };
  take(M);
  if (M > kSkinnyM) take(kSkinnyM);
  for (int64_t m = 64; m < M && m <= 256 * 256; m += 64) take(m);   // 256 tiles and more never split
  return best;
}

void mx4_gemm(at::Tensor out, at::Tensor xq, at::Tensor xs, at::Tensor w, at::Tensor s, at::Tensor workspace,
              int64_t splits_force) {
  const Mx4Args a = check_mx4(out, xq, xs, w, s);
  const int S = check_splits("mx4_gemm", a, splits_force, workspace, w);
  float* part = S > 1 ? workspace.data_ptr<float>() : nullptr;
  auto st = at::hip::getCurrentHIPStream();
  if (a.M <= kSkinnyM) {
    skinny_launch(S, st, xq, xs, w, s, a, out, part);
  } else {
    switch (pick_tile(a.M)) {
      case 0: mx4_launch<0, 64, 1, 4>(S, st, xq, xs, w, s, a, out, part); break;
      case 1: mx4_launch<1, 128, 2, 2>(S, st, xq, xs, w, s, a, out, part); break;
      default: mx4_launch<2, 256, 4, 2>(S, st, xq, xs, w, s, a, out, part); break;
    }
  }
  if (S > 1)
    mx4_reduce_kernel<<<(unsigned)(((int64_t)a.M * a.N / 4 + 255) / 256), 256, 0, st>>>(
        part, S, a.M, a.N, xs.data_ptr<float>(), (bf16*)out.data_ptr(), out.stride(0));
}

// The MXFP4 route: quantise the rows of x (bf16 [M, K]; silu_mul: gu [M, 2K], the rows are
// bf16(silu(g) * u)), then the block-scaled GEMM.
void linear_mxfp4(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor s, at::Tensor workspace, int64_t splits_force,
                  bool silu_mul) {
  check_rows(x, w, silu_mul);
  at::Tensor xq = at::empty({x.size(0), 2 * w.size(1)}, x.options().dtype(at::kFloat8_e4m3fn));
  at::Tensor xs = at::empty({x.size(0)}, x.options().dtype(at::kFloat));
  // both guards first: nothing is launched or written unless the whole route is valid
  check_splits("linear_mxfp4", check_mx4(out, xq, xs, w, s), splits_force, workspace, w);
  quantize_rows_fp8(xq, xs, x, silu_mul);
  mx4_gemm(out, xq, xs, w, s, workspace, splits_force);
}

// Adds {"mx4_skinny_s2": n, "mx4_bm128_s1": n, ...} to the census of w8_launch_counts.
void mx4_launch_counts(pybind11::dict& d, bool reset) {
  for (int t = 0; t < 4; ++t)
    for (int s = 0; s < kCensusS; ++s) {
      const int64_t n = reset ? g_mx4_count[t][s].exchange(0) : g_mx4_count[t][s].load();
      if (!n) continue;
      const std::string key = t == 0 ? "mx4_skinny" : "mx4_bm" + std::to_string(kBm[t - 1]);
      d[pybind11::str(key + "_s" + std::to_string(s))] = n;
    }
}
