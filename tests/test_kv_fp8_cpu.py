"""FP8 (e4m3) paged KV cache on the CPU: the reference quantiser (the format every HIP
writer must reproduce bit for bit), the reference write / gather path, and the CPU
LLMEngine with ``kv_cache_dtype="fp8"``."""
import pytest
import torch

from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaModel, PRESETS
from langstream_amd.ops import reference as ref

FP8 = torch.float8_e4m3fn


def _codes(t):
    return t.view(torch.uint8)


def _q(vals, scale=1.0):
    return _codes(ref.quantize_kv(torch.tensor(vals, dtype=torch.float32).to(torch.bfloat16), scale)).tolist()


def test_quantizer_saturates_without_nan():
    # 448 = 0x7E is the largest finite e4m3fn value; torch's own cast gives NaN (0x7F) past 464
    assert _q([448.0, 449.0, 464.0, 480.0, 1e4, 3e38, float("inf")]) == [0x7E] * 7
    assert _q([-448.0, -464.0, -480.0, -1e4, -3e38, float("-inf")]) == [0xFE] * 6
    # below the clamp the last binade still rounds to nearest: 416 | 432 (tie -> even 448) | 448
    assert _q([416.0, 424.0, 432.0, 440.0]) == [0x7D, 0x7D, 0x7E, 0x7E]
    # every finite or infinite bf16 pattern gives a non-NaN code
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    c = _codes(ref.quantize_kv(bits[~bits.isnan()]))
    assert not ((c & 0x7F) == 0x7F).any()
    assert ref.quantize_kv(bits[~bits.isnan()], 4.0).float().abs().max() == 448.0


def test_quantizer_rounds_to_nearest_even():
    # 1.0 = 0x38, spacing 1/8.  The tie 1.0625 goes DOWN to the even mantissa 000, the tie
    # 1.1875 goes UP to the even mantissa 010; just off a tie goes to the nearer value.
    assert _q([1.0, 1.0625, 1.125, 1.1875, 1.25]) == [0x38, 0x38, 0x39, 0x3A, 0x3A]
    assert _q([1.0703125, 1.1796875]) == [0x39, 0x39]
    assert _q([-1.0625, -1.1875]) == [0xB8, 0xBA]
    # the same pair one binade up and at the top of a binade (mantissa carry into the exponent)
    assert _q([2.125, 2.375, 1.9375]) == [0x40, 0x42, 0x40]


def test_quantizer_preserves_subnormals():
    # e4m3 subnormals k * 2^-9, k = 1..7 (codes 1..7); the smallest normal 2^-6 is code 8
    sub = [k * 2.0 ** -9 for k in range(1, 8)]
    assert _q(sub) == list(range(1, 8))
    assert _q([-v for v in sub]) == [0x80 + k for k in range(1, 8)]
    assert _q([2.0 ** -6]) == [8]
    # ties between subnormals: 0.5 ulp -> 0 (even), 1.5 ulp -> 2, 2.5 ulp -> 2; below 0.5 ulp -> 0
    assert _q([2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -11, 0.0]) == [0, 2, 2, 0, 0]
    assert _q([-0.0, -(2.0 ** -11)]) == [0x80, 0x80]
    # the values come back exactly
    back = ref.quantize_kv(torch.tensor(sub)).float()
    assert torch.equal(back, torch.tensor(sub))


def test_quantizer_scale_is_a_multiply_by_the_f32_reciprocal():
    x = (torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 3).to(torch.bfloat16)
    for s in (0.25, 4.0, 0.3, 1.7):
        inv = torch.tensor(1.0) / torch.tensor(s)    # f32, rounded once
        exp = (x.float() * inv).clamp(-448, 448).to(FP8)
        assert torch.equal(_codes(ref.quantize_kv(x, s)), _codes(exp))
    assert torch.equal(_codes(ref.quantize_kv(x, 0.25)), _codes(ref.quantize_kv((x.float() * 4).to(torch.bfloat16))))


@pytest.mark.parametrize("D", [64, 128])
def test_write_and_gather_round_trip(D):
    torch.manual_seed(D)
    T, Hq, Hkv, BS = 150, 8, 2, ops.KV_BLOCK
    ks, vs = 0.25, 4.0
    qkv = (torch.randn(T, (Hq + 2 * Hkv) * D) * 2).to(torch.bfloat16)
    pos = torch.arange(T, dtype=torch.int32) + 7
    cs = ref.rope_cos_sin(4096, D, 500000.0)
    nb = 4
    kc, vc = ops.new_kv_cache(nb, Hkv, D, "cpu", FP8)
    assert kc.dtype == FP8 and vc.dtype == FP8 and kc.shape == (nb, Hkv, BS, D) and vc.shape == (nb, Hkv, 8, D, 8)
    assert kc.element_size() == 1
    slots = torch.randperm(nb * BS)[:T].to(torch.int64)
    slots[3] = -1
    ops.rope_and_cache(qkv, pos, cs, slots, kc, vc, Hq, Hkv, k_scale=ks, v_scale=vs)
    rows = qkv.view(T, Hq + 2 * Hkv, D)      # rotated in place, bf16
    kq = _codes(ref.quantize_kv(rows[:, Hq: Hq + Hkv], ks))
    vq = _codes(ref.quantize_kv(rows[:, Hq + Hkv:], vs))
    written = 0
    for t in range(T):
        s = int(slots[t])
        if s < 0:
            continue
        blk, off = divmod(s, BS)
        assert torch.equal(_codes(kc)[blk, :, off], kq[t])
        assert torch.equal(_codes(vc)[blk, :, off // 8, :, off % 8], vq[t])
        written += 1
    assert int((_codes(kc) != 0).any(-1).sum()) == written * Hkv     # the slot -1 row is not cached
    # gather: one sequence whose block table lists the blocks in reverse
    bt = torch.tensor([3, 2, 1, 0], dtype=torch.int32)
    n = 200
    K, V = ref.gather_kv(kc, vc, bt, n)
    assert K.dtype == FP8 and K.shape == (n, Hkv, D) and V.shape == (n, Hkv, D)
    Kf, Vf = ref.dequant_kv(K, V, ks, vs)
    for j in (0, 63, 64, 199):
        blk, off = int(bt[j // BS]), j % BS
        assert torch.equal(Kf[j], kc[blk, :, off].float() * ks)
        assert torch.equal(Vf[j], vc[blk, :, off // 8, :, off % 8].float() * vs)
    # power-of-two scales: the dequantised values are the quantiser's grid, |x - x^| <= 2^-4 |x| (+ subnormal step)
    s0 = int(slots[0])
    blk, off = divmod(s0, BS)
    x = rows[0, Hq: Hq + Hkv].float()
    assert ((kc[blk, :, off].float() * ks - x).abs() <= x.abs() / 16 + ks * 2.0 ** -10).all()


@pytest.fixture(scope="module")
def small():
    return LlamaModel(PRESETS["llama-small"], device="cpu", dtype=torch.bfloat16, seed=5)


PROMPTS = [list(range(3 + 11 * i, 3 + 11 * i + n)) for i, n in enumerate((5, 33, 70, 130))]


def test_engine_fp8_generates_and_halves_block_bytes(small):
    kw = dict(num_blocks=32, max_model_len=512, max_batch=8)
    sp = SamplingParams(max_tokens=5, temperature=0.0, ignore_eos=True)
    e8 = LLMEngine(small, None, kv_cache_dtype="fp8", **kw)
    reqs = e8.generate(PROMPTS, sp)
    assert all(len(r.output_ids) == 5 for r in reqs)
    e16 = LLMEngine(small, None, **kw)
    assert e16.kv_cache_dtype == "bf16" and e8.kv_cache_dtype == "fp8"
    assert e8.kv_bytes_per_block * 2 == e16.kv_bytes_per_block
    cfg = small.cfg
    assert e16.kv_bytes_per_block == 2 * cfg.num_layers * small.hkv * 64 * cfg.head_dim * 2
    assert e8.stats["kv_cache_dtype"] == "fp8" and e8.stats["kv_bytes_per_block"] == e8.kv_bytes_per_block
    assert e16.stats["kv_cache_dtype"] == "bf16"
    assert all(k.dtype == FP8 and v.dtype == FP8 for k, v in e8.kv_caches)
    assert all(k.dtype == torch.bfloat16 for k, _ in e16.kv_caches)
    assert any(bool((_codes(k) != 0).any()) for k, _ in e8.kv_caches)
    with pytest.raises(ValueError):
        LLMEngine(small, None, kv_cache_dtype="int4", **kw)
    assert LLMEngine(small, None, kv_cache_dtype="auto", **kw).kv_cache_dtype == "bf16"


def test_engine_fp8_with_prefix_cache(small):
    head = list(range(100, 100 + 130))
    prompts = [head + list(range(500 + 20 * i, 500 + 20 * i + 9 + i)) for i in range(4)]
    sp = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True)
    kw = dict(num_blocks=64, max_model_len=512, max_batch=2, kv_cache_dtype="fp8", kv_k_scale=0.5, kv_v_scale=2.0)
    on = LLMEngine(small, None, prefix_cache=True, **kw)
    out_on = [r.output_ids for r in on.generate(prompts, sp)]
    off = LLMEngine(small, None, prefix_cache=False, **kw)
    tops = {}
    sp_ref = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True, logprobs=2)
    reqs = [off.submit(p, sp_ref, callback=lambda ev, i=i: tops.setdefault(i, []).append(dict(ev.top)))
            for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        off.step()
    off._flush()
    out_off = [r.output_ids for r in reqs]
    assert all(len(o) == 4 for o in out_on)
    assert on.prefix.stats["hits"] >= 1 and on.stats["prefix_hit_tokens"] >= 128
    assert off.stats["prefill_tokens"] - on.stats["prefill_tokens"] == on.stats["prefix_hit_tokens"]
    # copied blocks hold the codes the first prompt wrote: the same greedy tokens with and
    # without reuse (bf16 model: they may part only at a near-tie of the top two, < 0.1 nats)
    for i, (x, y) in enumerate(zip(out_on, out_off)):
        for t, (a, b) in enumerate(zip(x, y)):
            if a != b:
                alt = tops[i][t]
                assert a in alt and b in alt and abs(alt[a] - alt[b]) < 0.1, (i, t, a, b, alt)
                break


def _first_tops(e, prompts):
    events = {}
    reqs = [e.submit(p, SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True, logprobs=5),
                     callback=lambda ev, i=i: events.setdefault(i, ev)) for i, p in enumerate(prompts)]
    while not all(r.finished for r in reqs):
        e.step()
    e._flush()
    return [events[i] for i in range(len(prompts))]


def test_first_token_logprob_close_to_bf16_cache(small):
    """First-token top-1 log-prob, fp8 cache against a bf16 cache on the same model."""
    kw = dict(num_blocks=32, max_model_len=512, max_batch=8)
    t16 = _first_tops(LLMEngine(small, None, **kw), PROMPTS)
    t8 = _first_tops(LLMEngine(small, None, kv_cache_dtype="fp8", **kw), PROMPTS)
    gaps = [abs(a.top[0][1] - b.top[0][1]) for a, b in zip(t8, t16)]
    print("fp8 vs bf16 first-token top-1 log-prob gaps:", gaps)
    # measured on the CPU reference over PROMPTS: 0.0471, 0.0154, 0.0156, 0.0155 nats (largest
    # 0.0471); the bound is twice the largest
    assert max(gaps) <= 0.0943
