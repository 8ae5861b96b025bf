"""MXFP4 projection weights without a GPU: the OCP quantiser and the reference projection of
ops/reference.py, the ``weights_dtype="mxfp4"`` model (state dict, refusals by name) and the
``weights-dtype: mxfp4`` configuration key."""
import dataclasses

import pytest
import torch

from langstream_amd.models.llama import LlamaModel, PRESETS, TPInfo
from langstream_amd.ops import reference as ref

E2M1 = torch.tensor(ref.E2M1_VALUES + tuple(-v for v in ref.E2M1_VALUES))


def _codes(packed):
    return torch.stack([packed & 15, packed >> 4], 2).view(packed.shape[0], -1)


def test_quantiser_reproduces_every_e2m1_block_exactly():
    """e2m1 values times 2^e with 4 or 6 present come back exactly; amax 6 * 2^e gets byte e + 127."""
    g = torch.Generator().manual_seed(0)
    es = torch.tensor([-127, -126, -20, -1, 0, 1, 7, 60, 125])
    q = torch.randint(0, 16, (len(es), 64), generator=g)
    q[:, 0], q[:, 32], q[:, 33] = 7, 6, 15        # amax 6 in block 0, 4 (and -6) in block 1
    w = torch.ldexp(E2M1[q], es[:, None])
    codes, scales = ref.quantize_weight_mxfp4(w)
    assert torch.equal(scales, (es + 127).to(torch.uint8)[:, None].expand(9, 2))
    assert torch.equal(ref.dequantize_weight_mxfp4(codes, scales), w)
    assert torch.equal(_codes(codes)[:, (0, 32, 33)], torch.tensor([[7, 6, 15]]).expand(9, 3).to(torch.uint8))
    assert torch.equal(codes.view(torch.float4_e2m1fn_x2).view(torch.uint8), codes)
    pair = torch.zeros(1, 32)
    pair[0, 0], pair[0, 1] = 1.0, -6.0                                   # codes 2 and 15
    assert int(ref.quantize_weight_mxfp4(pair)[0][0, 0]) == 2 | 15 << 4


def test_quantiser_zero_block_ties_and_saturation():
    w = torch.zeros(2, 64)
    # amax 4 -> e = 0: midpoints go to the even code; 7.5 saturates to 6
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -2.5, -5.0])
    w[0, 32] = 4.0
    w[0, 33:33 + len(ties)] = ties
    w[1, :3] = torch.tensor([7.5, -7.0, 5.5])
    codes, scales = ref.quantize_weight_mxfp4(w)
    assert scales.tolist() == [[127, 127], [127, 127]]
    q = _codes(codes)
    assert not bool(q[0, :32].any()) and not bool(q[1, 32:].any())           # zero blocks: zero codes, no -0
    assert q[0, 33:33 + len(ties)].tolist() == [0, 2, 2, 4, 4, 6, 6, 0, 10, 12, 14]
    assert q[1, :3].tolist() == [7, 15, 7]
    with pytest.raises(ValueError, match="255"):
        ref.dequantize_weight_mxfp4(codes, torch.full_like(scales, 255))
    with pytest.raises(ValueError, match="multiple"):
        ref.quantize_weight_mxfp4(torch.zeros(2, 48))


@pytest.mark.parametrize("silu_mul", [False, True])
def test_linear_mxfp4_reference_formula(silu_mul):
    """f32 against a plain float64 product over the dequantised operands, within K roundings."""
    g = torch.Generator().manual_seed(1)
    M, N, K = 7, 128, 256
    x = torch.randn(M, 2 * K if silu_mul else K, generator=g).to(torch.bfloat16)
    codes, scales = ref.quantize_weight_mxfp4(torch.randn(N, K, generator=g) * 0.05)
    xq, xs = ref.quantize_rows_fp8(x, silu_mul)
    wd = ref.dequantize_weight_mxfp4(codes, scales, torch.float64)
    want = (xq.double() * xs.double()[:, None]) @ wd.t()
    got = ref.linear_mxfp4(x, codes, scales, dtype=torch.float32, silu_mul=silu_mul)
    assert got.dtype == torch.float32
    bound = K * 2.0 ** -23 * ((xq.double().abs() * xs.double()[:, None]) @ wd.abs().t())
    assert bool(((got.double() - want).abs() <= bound).all())
    assert torch.equal(ref.linear_mxfp4(x, codes, scales, silu_mul=silu_mul), got.to(torch.bfloat16))
    assert torch.equal(ref.linear_mxfp4(x, codes, scales, dtype=torch.float64, silu_mul=silu_mul), want)


def test_model_state_dict_round_trip_and_refusals():
    cfg = PRESETS["llama-tiny"]
    m = LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype="mxfp4")
    l0 = m.layers[0]
    N, K2 = l0.down_w.shape
    assert l0.down_w.dtype == l0.down_s.dtype == torch.uint8 and l0.down_s.shape == (N, 2 * K2 // 32)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    other = LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype="mxfp4", seed=5)
    other.load_state_dict(sd)
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())
    wide = LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=7)
    other.load_state_dict(wide.state_dict())
    c, s = ref.quantize_weight_mxfp4(wide.layers[1].o_w)
    assert torch.equal(other.layers[1].o_w, c) and torch.equal(other.layers[1].o_s, s)

    def load(model, **changes):
        model.load_state_dict({**sd, **changes})

    with pytest.raises(ValueError, match=r"layers\.0\.qkv_s.*255"):
        load(other, **{"layers.0.qkv_s": torch.full_like(sd["layers.0.qkv_s"], 255)})
    for wd in ("bf16", "fp8"):
        with pytest.raises(ValueError, match="layers.0.qkv_w holds MXFP4 codes"):
            load(LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype=wd))
    with pytest.raises(ValueError, match="layers.0.qkv_w holds int4 codes"):
        other.load_state_dict(LlamaModel(cfg, device="cpu", dtype=torch.float32, weights_dtype="int4").state_dict())
    with pytest.raises(ValueError, match="activations_dtype='fp8' with weights_dtype='mxfp4'"):
        LlamaModel(cfg, device="cpu", weights_dtype="mxfp4", activations_dtype="fp8")
    with pytest.raises(ValueError, match="mixture-of-experts.*mxfp4"):
        LlamaModel(PRESETS["qwen3-moe-tiny"], device="cpu", weights_dtype="mxfp4")
    with pytest.raises(ValueError, match="mxfp4.*tensor parallelism"):
        LlamaModel(cfg, device="cpu", weights_dtype="mxfp4", tp=TPInfo(rank=0, world=2))
    with pytest.raises(ValueError, match=r"layers\.0\.gate_up_w.*multiples of 128"):
        LlamaModel(dataclasses.replace(cfg, intermediate_size=cfg.intermediate_size + 32), device="cpu",
                   weights_dtype="mxfp4")


@pytest.mark.parametrize("source", ["key", "environment"])
def test_weights_dtype_mxfp4_flows_from_configuration(monkeypatch, source):
    from langstream_amd.services import ServiceRegistry
    monkeypatch.setenv("LS_WEIGHTS_DTYPE", "mxfp4" if source == "environment" else "bf16")
    reg = ServiceRegistry({"device": "cpu", "num-blocks": 16, "use-graphs": "false", "max-model-len": 256,
                           "chat-model": "llama-tiny", **({"weights-dtype": "mxfp4"} if source == "key" else {})})
    try:
        e = reg.llm_engine("llama-tiny")
        assert e.stats["weights_dtype"] == "mxfp4" and e.model.layers[0].qkv_s.dtype == torch.uint8
        assert e.stats["weight_bytes"] == e.model.weight_bytes
    finally:
        reg.shutdown()
