// W8A16 projections: out[M, N] = bf16((x[M, K] . code[N, K]^T) * s[N]) with bf16 activations,
// OCP e4m3fn weight codes (torch.float8_e4m3fn, one byte each) and one f32 scale per output
// row.  A code decodes to bf16 exactly (3 mantissa bits), so the products run on the bf16
// MFMA / dot instructions and the accumulation is f32; the weights cross HBM, L2 and LDS as
// bytes -- half the traffic of the bf16 kernels, which is the whole cost of a small-batch
// decode step.
//
// w8_gemm: tiled MFMA GEMM for any M >= 1.  Tile BM x 64 x 64 (BM = 64 for M <= 64, else
//   128), 256 threads, one wave per (BM/2) x 32 sub-tile of 16x16x32 accumulators.  Per K
//   step a thread moves BM/32 16-B chunks of x and ONE 16-B chunk of w (16 codes) global ->
//   registers -> LDS, double-buffered with the next step's loads in flight during the MFMAs
//   (the structure of gemm_skinny.hip).  W sits in LDS as codes (80-B rows: 64 codes + pad);
//   each lane reads its 8 codes of an MFMA operand with one 8-B LDS read and expands them in
//   registers (fp8_unpack8).  Few tiles cannot fill the chip, so the launcher cuts K into
//   S in {1, 2, 4, 8} slices (gridDim.y); slices store f32 partials into workspace slabs
//   [S, M, N] that splitk_reduce_launch sums.
//   SCALE: s[n] multiplies the f32 accumulator once, in the epilogue -- the final sum at
//   S = 1, each slice's partial before it is stored at S > 1 (the reduction then only adds).
// w8_gemv: register-streaming kernel for M <= 4 (the structure of gemm_gemv.hip): a block
//   owns RB rows of w, K is cut into 1024-code chunks (64 lanes x 16 B), chunk c belongs to
//   wave c % 4; every weight load is a non-temporal 16-B load issued before the first dot,
//   x stays in registers, the dots run on v_dot2c_f32_bf16 after the in-register decode.
//   Shape rule: K % 1024 == 0, K <= 28672.  Other shapes at M <= 4 run on w8_gemm.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <atomic>
#include <string>

#include "ops.h"

namespace {

constexpr int BN = 64, BK = 64;
constexpr int LDX = BK + 8;   // x LDS row, bf16 elements (144 B)
constexpr int LDW = BK + 16;  // w LDS row, bytes (80 B: 16-B stores and 8-B reads stay aligned)

template <int BM, bool PARTIAL>
__global__ void __launch_bounds__(256) w8_gemm_kernel(const bf16* __restrict__ x, int64_t ldx,
                                                      const fp8_t* __restrict__ w, const float* __restrict__ sc,
                                                      int M, int N, int K, int S, bf16* __restrict__ out,
                                                      int64_t ldo, float* __restrict__ part, int MT) {
  constexpr int XS = BM * LDX * 2, WS = BN * LDW;  // bytes per stage
  constexpr int XC = BM * 8 / 256;                 // 16-B x chunks per thread per K step
  __shared__ __attribute__((aligned(16))) char lds[2 * (XS + WS)];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = logical % MT, nt = logical / MT;
  const int m0 = mt * BM;
  // K steps [k0, k1) of slice blockIdx.y (S <= K / 64, host-checked: every slice has a step)
  const int nkt = K / BK;
  const int k0 = (int)((int64_t)blockIdx.y * nkt / S), k1 = (int)((int64_t)(blockIdx.y + 1) * nkt / S);
  const int nk = k1 - k0;
  const int64_t kbeg = (int64_t)k0 * BK;

  const bf16* xp[XC];
  bool xok[XC];
#pragma unroll
  for (int i = 0; i < XC; ++i) {
    const int q = tid + 256 * i, row = q >> 3, kc = q & 7;
    xok[i] = m0 + row < M;
    xp[i] = x + (int64_t)(xok[i] ? m0 + row : 0) * ldx + kbeg + kc * 8;
  }
  const fp8_t* wp = w + (int64_t)(nt * BN + (tid >> 2)) * K + kbeg + (tid & 3) * 16;
  uint4 rx[XC], rw;
  auto gload = [&](int kt) {
    const int ko = kt * BK;
#pragma unroll
    for (int i = 0; i < XC; ++i) rx[i] = xok[i] ? ld16(xp[i] + ko) : make_uint4(0, 0, 0, 0);
    rw = ld16(wp + ko);
  };
  auto lstore = [&](int buf) {
    char* lx = lds + buf * (XS + WS);
    char* lw = lx + XS;
#pragma unroll
    for (int i = 0; i < XC; ++i) {
      const int q = tid + 256 * i;
      st16(lx + ((q >> 3) * LDX + (q & 7) * 8) * 2, rx[i]);
    }
    st16(lw + (tid >> 2) * LDW + (tid & 3) * 16, rw);
  };

  constexpr int IT = BM / 32;  // 16-row accumulator tiles per wave
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  f32x4 acc[IT][2];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  lstore(0);
  if (nk > 1) gload(1);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* lx = lds + (kt & 1) * (XS + WS);
    const char* lw = lx + XS;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[IT], b[2];
#pragma unroll
      for (int i = 0; i < IT; ++i)
        a[i] = __builtin_bit_cast(bf16x8, ld16(lx + (((BM / 2) * wm + 16 * i + fr) * LDX + 32 * ks + fk) * 2));
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j] = fp8_unpack8(*reinterpret_cast<const uint2*>(lw + (32 * wn + 16 * j + fr) * LDW + 32 * ks + fk));
#pragma unroll
      for (int i = 0; i < IT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      lstore((kt + 1) & 1);
      if (kt + 2 < nk) gload(kt + 2);
    }
    __syncthreads();
  }

  // acc[i][j][r] = C[(BM/2) wm + 16 i + 4 (lane >> 4) + r][32 wn + 16 j + fr] (tile-local)
  const int rbase = (BM / 2) * wm + 4 * (lane >> 4);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = nt * BN + 32 * wn + 16 * j + fr;
    const float sn = sc[n];
#pragma unroll
    for (int i = 0; i < IT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + rbase + 16 * i + r;
        if (m >= M) continue;
        const float v = acc[i][j][r] * sn;
        if (PARTIAL) part[((int64_t)blockIdx.y * M + m) * N + n] = v;
        else out[(int64_t)m * ldo + n] = (bf16)v;
      }
  }
}

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// 8-element bf16 dot on v_dot2c_f32_bf16 (pairs taken with shufflevector, as gemm_gemv.hip)
__device__ __forceinline__ float dot8(bf16x8 av, bf16x8 bv, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(av, av, 0, 1), __builtin_shufflevector(bv, bv, 0, 1),
                                        acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(av, av, 2, 3), __builtin_shufflevector(bv, bv, 2, 3),
                                        acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(av, av, 4, 5), __builtin_shufflevector(bv, bv, 4, 5),
                                        acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(av, av, 6, 7), __builtin_shufflevector(bv, bv, 6, 7),
                                        acc, false);
  return acc;
}

// TR: rows of x handled (rows >= T are clamped to T - 1 and not stored); KCH: 1024-code
// chunks per wave (ceil(K / 4096)); RB: w rows per block.
template <int TR, int KCH, int RB>
__global__ void __launch_bounds__(256) w8_gemv_kernel(const bf16* __restrict__ x, int64_t ldx, int T,
                                                      const fp8_t* __restrict__ W, const float* __restrict__ sc,
                                                      int N, int K, bf16* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nchunk = K >> 10;  // K % 1024 == 0 (host-checked)
  const int base = blockIdx.x * RB;
  u32x4 wr[RB][KCH];
  u32x4 xr[TR][KCH][2];
  // branch-free tail: a chunk past K reloads the last one and is zeroed by a select
#pragma unroll
  for (int m = 0; m < TR; ++m) {
    const bf16* xm = x + (int64_t)min(m, T - 1) * ldx + lane * 16;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const bf16* p = xm + (min(c * 4 + wv, nchunk - 1) << 10);
      xr[m][c][0] = *reinterpret_cast<const u32x4*>(p);
      xr[m][c][1] = *reinterpret_cast<const u32x4*>(p + 8);
    }
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const fp8_t* wrow = W + (int64_t)(base + r) * K + lane * 16;
#pragma unroll
    for (int c = 0; c < KCH; ++c)
      wr[r][c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow + (min(c * 4 + wv, nchunk - 1) << 10)));
  }
  // where x + w fit in ~160 VGPRs every w load is issued before the first dot (the empty asm
  // "redefines" the fragments after the loads); larger K streams through a rolling window
  if constexpr (RB * KCH * 4 + TR * KCH * 8 <= 160) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int c = 0; c < KCH; ++c) asm volatile("" : "+v"(wr[r][c]));
  }
#pragma unroll
  for (int m = 0; m < TR; ++m)
#pragma unroll
    for (int c = 0; c < KCH; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) xr[m][c][h] = c * 4 + wv < nchunk ? xr[m][c][h] : u32x4{0, 0, 0, 0};
  float acc[RB][TR];
#pragma unroll
  for (int r = 0; r < RB; ++r) {
#pragma unroll
    for (int m = 0; m < TR; ++m) acc[r][m] = 0.f;
#pragma unroll
    for (int c = 0; c < KCH; ++c) {
      const uint4 cw = __builtin_bit_cast(uint4, wr[r][c]);
      const bf16x8 lo = fp8_unpack8(make_uint2(cw.x, cw.y)), hi = fp8_unpack8(make_uint2(cw.z, cw.w));
#pragma unroll
      for (int m = 0; m < TR; ++m) {
        acc[r][m] = dot8(lo, __builtin_bit_cast(bf16x8, xr[m][c][0]), acc[r][m]);
        acc[r][m] = dot8(hi, __builtin_bit_cast(bf16x8, xr[m][c][1]), acc[r][m]);
      }
    }
  }
  // reduce over the 64 lanes, then over the 4 waves through LDS
  __shared__ float red[4][RB * TR];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int m = 0; m < TR; ++m) acc[r][m] += __shfl_xor(acc[r][m], o, 64);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int m = 0; m < TR; ++m) red[wv][r * TR + m] = acc[r][m];
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < RB * TR) {
    const int r = t / TR, m = t % TR;
    if (m < T)
      out[(int64_t)m * ldo + base + r] = (bf16)((red[0][t] + red[1][t] + red[2][t] + red[3][t]) * sc[base + r]);
  }
}

// Host-side launch census, one counter per kernel variant: the tests read it to prove which
// route a shape took (w8_launch_counts).  Relaxed atomics on the host only.
constexpr int kCensusS = 17;
std::atomic<int64_t> g_gemv_count;
std::atomic<int64_t> g_gemm_count[2][kCensusS];   // [BM == 128][splits]

int pick_bm(int64_t M) { return M <= 64 ? 64 : 128; }

// K slices: enough workgroups for 256 CUs x 2 where the tiles alone are fewer, at least 4 K
// steps per slice, a power of two up to 8.
int pick_split(int64_t M, int64_t N, int64_t K) {
  const int bm = pick_bm(M);
  const int64_t tiles = ((M + bm - 1) / bm) * (N / BN);
  const int64_t want = 512 / std::max<int64_t>(tiles, 1), cap = std::min<int64_t>(8, K / BK / 4);
  int s = 1;
  while (s * 2 <= want && s * 2 <= cap) s *= 2;
  return s;
}

struct W8Args {
  int M, N, K;
};

// Every guard of the two entry points; raises before anything is launched or written.
W8Args check_w8(const char* who, const at::Tensor& out, const at::Tensor& x, const at::Tensor& w,
                const at::Tensor& s) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && s.is_cuda() && out.is_cuda(), who, ": GPU tensors expected");
  TORCH_CHECK(x.device() == w.device() && x.device() == s.device() && x.device() == out.device(), who,
              ": tensors on different devices");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, who, ": x must be bf16");
  TORCH_CHECK(w.scalar_type() == at::kFloat8_e4m3fn, who, ": w must be float8_e4m3fn codes");
  TORCH_CHECK(s.scalar_type() == at::kFloat, who, ": s must be float32");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16, who, ": out must be bf16");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), who, ": w must be contiguous [N, K]");
  TORCH_CHECK(s.is_contiguous() && s.numel() == w.size(0), who, ": s must be contiguous with N = ", w.size(0),
              " elements, got ", s.numel());
  TORCH_CHECK(x.dim() == 2 && x.size(1) == w.size(1) && x.stride(1) == 1 && (x.size(0) == 1 || x.stride(0) % 8 == 0),
              who, ": x must be [M, K] with unit inner stride and a row stride that is a multiple of 8");
  TORCH_CHECK(x.size(0) >= 1, who, ": M >= 1");
  TORCH_CHECK(w.size(0) % BN == 0 && w.size(1) % BK == 0, who, ": N and K must be multiples of 64, got N = ",
              w.size(0), ", K = ", w.size(1));
  TORCH_CHECK(out.dim() == 2 && out.size(0) == x.size(0) && out.size(1) == w.size(0) && out.stride(1) == 1 &&
                  (out.size(0) == 1 || out.stride(0) % 4 == 0),
              who, ": out must be [M, N] with unit inner stride and a row stride that is a multiple of 4");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(w.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(s.data_ptr()) & 15) == 0,
              who, ": x, w and s must be 16-byte aligned");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(out.data_ptr()) & 7) == 0, who, ": out must be 8-byte aligned");
  TORCH_CHECK(x.size(0) < (int64_t(1) << 24) && w.size(0) < (int64_t(1) << 24) && w.size(1) < (int64_t(1) << 24), who,
              ": dimension too large");
  return W8Args{(int)x.size(0), (int)w.size(0), (int)w.size(1)};
}

bool gemv_shape(int64_t N, int64_t K) { return K % 1024 == 0 && K <= 28672 && N % 8 == 0; }

template <int BM>
void gemm_launch(int S, hipStream_t st, const at::Tensor& x, const at::Tensor& w, const at::Tensor& s, W8Args a,
                 at::Tensor& out, float* part) {
  const int MT = (a.M + BM - 1) / BM;
  const dim3 grid((unsigned)(MT * (a.N / BN)), (unsigned)S);
  g_gemm_count[BM == 128][std::min(S, kCensusS - 1)].fetch_add(1, std::memory_order_relaxed);
  if (S == 1)
    w8_gemm_kernel<BM, false><<<grid, 256, 0, st>>>((const bf16*)x.data_ptr(), x.stride(0), (const fp8_t*)w.data_ptr(),
                                                    s.data_ptr<float>(), a.M, a.N, a.K, 1, (bf16*)out.data_ptr(),
                                                    out.stride(0), nullptr, MT);
  else
    w8_gemm_kernel<BM, true><<<grid, 256, 0, st>>>((const bf16*)x.data_ptr(), x.stride(0), (const fp8_t*)w.data_ptr(),
                                                   s.data_ptr<float>(), a.M, a.N, a.K, S, nullptr, 0, part, MT);
}

template <int TR, int KCH>
void gemv_launch_rb(hipStream_t st, const at::Tensor& x, const at::Tensor& w, const at::Tensor& s, W8Args a,
                    at::Tensor& out) {
  // RB w rows share one x fetch and one reduction; 8 while the fragments fit in registers
  constexpr int RB = KCH <= 2 ? 8 : 4;
  w8_gemv_kernel<TR, KCH, RB><<<a.N / RB, 256, 0, st>>>((const bf16*)x.data_ptr(), x.stride(0), a.M,
                                                        (const fp8_t*)w.data_ptr(), s.data_ptr<float>(), a.N, a.K,
                                                        (bf16*)out.data_ptr(), out.stride(0));
}

template <int TR>
void gemv_launch_k(hipStream_t st, const at::Tensor& x, const at::Tensor& w, const at::Tensor& s, W8Args a,
                   at::Tensor& out) {
  switch ((a.K + 4095) / 4096) {
    case 1: return gemv_launch_rb<TR, 1>(st, x, w, s, a, out);
    case 2: return gemv_launch_rb<TR, 2>(st, x, w, s, a, out);
    case 3: return gemv_launch_rb<TR, 3>(st, x, w, s, a, out);
    case 4: return gemv_launch_rb<TR, 4>(st, x, w, s, a, out);
    case 5: return gemv_launch_rb<TR, 5>(st, x, w, s, a, out);
    case 6: return gemv_launch_rb<TR, 6>(st, x, w, s, a, out);
    case 7: return gemv_launch_rb<TR, 7>(st, x, w, s, a, out);
    default: TORCH_CHECK(false, "w8_gemv: K = ", a.K, " > 28672 is not supported");
  }
}

}  // namespace

// The shape rule of the W8 kernels: fp8 codes, contiguous [N, K], N % 64 == 0, K % 64 == 0.
bool w8_supported(const at::Tensor& w) {
  return w.dim() == 2 && w.scalar_type() == at::kFloat8_e4m3fn && w.is_contiguous() && w.size(0) % BN == 0 &&
         w.size(1) % BK == 0;
}

// Whether w8_gemv takes this weight (M <= 4 is the caller's side of the rule).
bool w8_gemv_supported(const at::Tensor& w) { return w8_supported(w) && gemv_shape(w.size(0), w.size(1)); }

// Workspace bytes that suffice for w8_gemm at every row count 1..M with automatic splits
// (callers that capture graphs allocate it once; M may be any upper bound).
int64_t w8_gemm_workspace(int64_t M, int64_t N, int64_t K) {
  TORCH_CHECK(M >= 1 && N >= BN && K >= BK, "w8_gemm_workspace: M >= 1, N >= 64, K >= 64");
  int64_t best = 0;
  auto take = [&](int64_t m) {
    const int S = pick_split(m, N, K);
    if (S > 1) best = std::max(best, (int64_t)S * m * N * 4);
  };
  take(std::min<int64_t>(M, 64));
  for (int64_t m = 128; ; m += 128) {
    take(std::min(m, M));
    if (m >= M || (m / 128) * (N / BN) >= 512) break;   // more tiles than that never split
  }
  return best;
}

void w8_gemm(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor s, at::Tensor workspace, int64_t splits_force) {
  const W8Args a = check_w8("w8_gemm", out, x, w, s);
  TORCH_CHECK(splits_force >= 0, "w8_gemm: splits >= 0 (0: automatic)");
  const int S = splits_force > 0 ? (int)std::min<int64_t>(splits_force, a.K / BK) : pick_split(a.M, a.N, a.K);
  float* part = nullptr;
  if (S > 1) {
    TORCH_CHECK(workspace.is_cuda() && workspace.device() == x.device() && workspace.scalar_type() == at::kFloat &&
                    workspace.is_contiguous() && workspace.numel() >= (int64_t)S * a.M * a.N,
                "w8_gemm: workspace must be a contiguous float32 tensor of at least splits * M * N = ",
                (int64_t)S * a.M * a.N, " elements on the device of x");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(workspace.data_ptr()) & 15) == 0, "w8_gemm: workspace must be 16-byte aligned");
    part = workspace.data_ptr<float>();
  }
  auto st = at::hip::getCurrentHIPStream();
  if (pick_bm(a.M) == 64) gemm_launch<64>(S, st, x, w, s, a, out, part);
  else gemm_launch<128>(S, st, x, w, s, a, out, part);
  if (S > 1) splitk_reduce_launch(part, S, a.M, a.N, (bf16*)out.data_ptr(), out.stride(0), st);
}

void w8_gemv(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor s) {
  const W8Args a = check_w8("w8_gemv", out, x, w, s);
  TORCH_CHECK(a.M <= 4, "w8_gemv: 1 <= M <= 4, got ", a.M);
  TORCH_CHECK(gemv_shape(a.N, a.K), "w8_gemv: K must be a multiple of 1024 and at most 28672, got K = ", a.K);
  auto st = at::hip::getCurrentHIPStream();
  g_gemv_count.fetch_add(1, std::memory_order_relaxed);
  switch (a.M) {
    case 1: return gemv_launch_k<1>(st, x, w, s, a, out);
    case 2: return gemv_launch_k<2>(st, x, w, s, a, out);
    default: return gemv_launch_k<4>(st, x, w, s, a, out);
  }
}

// The route every caller takes: w8_gemv for M <= 4 where its shape rule holds, else w8_gemm.
void linear_w8(at::Tensor out, at::Tensor x, at::Tensor w, at::Tensor s, at::Tensor workspace, int64_t splits_force) {
  if (x.dim() == 2 && x.size(0) <= 4 && splits_force == 0 && w.dim() == 2 && gemv_shape(w.size(0), w.size(1)))
    w8_gemv(out, x, w, s);
  else
    w8_gemm(out, x, w, s, workspace, splits_force);
}

// The launch census since the last reset: {"gemv": n, "gemm_bm64_s4": n, ...}.
pybind11::dict w8_launch_counts(bool reset) {
  pybind11::dict d;
  const int64_t g = reset ? g_gemv_count.exchange(0) : g_gemv_count.load();
  if (g) d[pybind11::str("gemv")] = g;
  for (int b = 0; b < 2; ++b)
    for (int s = 0; s < kCensusS; ++s) {
      const int64_t n = reset ? g_gemm_count[b][s].exchange(0) : g_gemm_count[b][s].load();
      if (n == 0) continue;
      d[pybind11::str("gemm_bm" + std::to_string(b ? 128 : 64) + "_s" + std::to_string(s))] = n;
    }
  return d;
}
