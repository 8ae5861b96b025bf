"""Operands for the W8A16 (fp8 weight) kernel tests (a plain module shared by
test_weights_fp8_cpu.py and test_weights_fp8_gpu.py; torch only, everything is built on the CPU).

EXACT set: x in {-2, -1, 1, 2}, weight codes with values in {0, +-0.5, +-1, +-1.5, +-2, +-3,
+-4, +-6} and at most 64 non-zeros per row, row scales in {0.5, 1, 2}.  Every product is a
multiple of 0.5 of magnitude <= 12, a row sums at most 64 of them, so every partial sum of any
subset of the K products, in any order and under any K split, is a multiple of 0.5 below
768 -- exact in f32 -- and the scaled sum a multiple of 0.25 below 1536, exact in f32 too:
the kernel's output must EQUAL bf16(reference).

The non-zeros are placed as gemm_probe.probe_columns names them: column 0, K - 1, every
multiple of the kernel's K step (64, which includes every split boundary and every 1024-code
chunk of the GEMV) and the column before it are non-zero in some row, so zeroing one x element
there changes an output (probes_seen checks that on the oracle).

ROUNDED set: the same x and codes with arbitrary positive scales; compared with the project's
rounded rule |got - ref| <= 2^-7 |ref| + 1e-6 (gemm_probe.RTOL / FLOOR).
"""
from __future__ import annotations

import functools

import torch

import gemm_probe as gp
from langstream_amd.ops import reference as ref

FP8 = torch.float8_e4m3fn
X_VALS = (-2.0, -1.0, 1.0, 2.0)
CODE_VALS = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
SCALES = (0.5, 1.0, 2.0)
NZ = 64
STEP = 64          # K step of w8_gemm; the GEMV's 1024-code chunks are multiples of it


def _choice(vals, shape, g):
    v = torch.tensor(vals, dtype=torch.float32)
    return v[torch.randint(0, len(vals), shape, generator=g)]


@functools.lru_cache(maxsize=64)
def make_codes(N, K, seed=0):
    """float8_e4m3fn [N, K]: min(64, K) non-zeros per row, every probe column non-zero in some row."""
    g = torch.Generator().manual_seed(seed + 13 * K + 7 * N)
    nz = min(NZ, K)
    cols = gp.probe_columns(K, STEP)
    rep = max(1, min(3, (N * nz) // (2 * len(cols))))
    score = torch.rand(N, K, generator=g)
    per_row = [0] * N
    stride = 37 if N % 37 else 41
    for i, k in enumerate(cols):
        for j in range(rep):
            r = ((i * rep + j) * stride) % N
            score[r, k] = -1.0
            per_row[r] += 1
    assert max(per_row) <= nz, (N, K, max(per_row))
    idx = score.topk(nz, dim=1, largest=False).indices
    w = torch.zeros(N, K)
    w.scatter_(1, idx, _choice(CODE_VALS, (N, nz), g) * _choice((-1.0, 1.0), (N, nz), g))
    assert bool((w[:, cols] != 0).any(0).all())
    codes = w.to(FP8)
    assert torch.equal(codes.float(), w)          # every value is an e4m3 number
    return codes


@functools.lru_cache(maxsize=64)
def make_x(M, K, seed=0):
    return _choice(X_VALS, (M, K), torch.Generator().manual_seed(1000 + seed + K)).to(torch.bfloat16)


@functools.lru_cache(maxsize=64)
def exact_scales(N, seed=0):
    return _choice(SCALES, (N,), torch.Generator().manual_seed(77 + seed + N)).contiguous()


@functools.lru_cache(maxsize=64)
def rounded_scales(N, seed=0):
    """amax / 448-style scales: arbitrary positive f32 over three decades."""
    g = torch.Generator().manual_seed(99 + seed + N)
    return (torch.rand(N, generator=g) * 3.0 + 0.05).mul(10.0 ** torch.randint(-3, 0, (N,), generator=g).float()) \
        .to(torch.float32).contiguous()


@functools.lru_cache(maxsize=64)
def oracle(M, N, K, rounded=False):
    """float64 reference of the case, computed once and shared."""
    s = rounded_scales(N) if rounded else exact_scales(N)
    return ref.linear_w8(make_x(M, K), make_codes(N, K), s, dtype=torch.float64)


def probes_seen(M, N, K):
    """Zeroing x[m, k] at every probe column k changes the oracle's row m (m = 0 and M - 1)."""
    x, codes, s = make_x(M, K), make_codes(N, K), exact_scales(N)
    base = oracle(M, N, K)
    wd = codes.double() * s.double()[:, None]
    for m in sorted({0, M - 1}):
        for k in gp.probe_columns(K, STEP):
            delta = x[m, k].double() * wd[:, k]       # what the row loses without x[m, k]
            if not bool(((base[m] - delta) != base[m]).any()):
                return False
    return True


def all_codes_case():
    """K = 256, M = 256, N = 128: x the identity, w[n, k] the code (n + k) mod 256 with the two
    NaN codes replaced by 0 -> out[m, n] = value of code (n + m) mod 256 times s[n], exactly."""
    n = torch.arange(128)[:, None]
    k = torch.arange(256)[None, :]
    byte = ((n + k) % 256).to(torch.uint8)
    byte = torch.where((byte & 0x7F) == 0x7F, torch.zeros_like(byte), byte)
    codes = byte.contiguous().view(FP8)
    x = torch.eye(256, dtype=torch.bfloat16)
    s = exact_scales(128)
    expect = (codes.float().t() * s[None, :]).double()     # [m = k, n]
    return x, codes, s, expect
