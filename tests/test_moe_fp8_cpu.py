"""FP8 expert weights above the kernel, on the CPU: the model's quantiser, state dicts in both forms,
ops.moe_mlp with scales, and the experts-dtype configuration key."""
import pytest
import torch

from langstream_amd import ops
from langstream_amd.models.llama import EXPERT_NAMES, LlamaModel, PRESETS
from langstream_amd.ops import reference as ref

MOE = PRESETS["qwen3-moe-tiny"]


def _model(seed=0, **kw):
    return LlamaModel(MOE, device="cpu", dtype=torch.float32, seed=seed, **kw)


def _same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def test_model_quantises_its_experts_with_the_one_rule():
    wide, m8 = _model(), _model(experts_dtype="fp8")
    for lw, l8 in zip(wide.layers, m8.layers):
        for n in EXPERT_NAMES:
            w = getattr(lw, n + "_w")
            codes, s = ref.quantize_weight_fp8(w.reshape(-1, w.shape[-1]))
            assert torch.equal(getattr(l8, n + "_w").view(torch.uint8), codes.view(torch.uint8).view(w.shape))
            assert torch.equal(getattr(l8, n + "_s"), s.view(w.shape[:2]))
        assert torch.equal(lw.qkv_w, l8.qkv_w) and torch.equal(lw.router_w, l8.router_w)   # everything else as it was
    assert m8.weight_bytes < wide.weight_bytes and "layers.0.experts_down_s" in m8.state_dict()


@pytest.mark.parametrize("form", ["wide", "codes"])
def test_state_dict_round_trip(form):
    m8, other = _model(experts_dtype="fp8"), _model(seed=1, experts_dtype="fp8")
    assert not _same(other.state_dict(), m8.state_dict())
    other.load_state_dict(_model().state_dict() if form == "wide" else m8.state_dict())
    assert _same(other.state_dict(), m8.state_dict())
    sd = m8.state_dict()
    with pytest.raises(ValueError, match="layers.0.experts_gate_up_w holds float8_e4m3fn codes but the model's experts_dtype"):
        _model().load_state_dict(sd)
    with pytest.raises(ValueError, match="layers.0.experts_gate_up_s is missing"):
        other.load_state_dict({k: v for k, v in sd.items() if k != "layers.0.experts_gate_up_s"})


def test_cpu_moe_mlp_with_scales_is_the_reference_on_the_dequantised_weights():
    l8 = _model(experts_dtype="fp8").layers[0]
    x = torch.randn(9, MOE.hidden_size, generator=torch.Generator().manual_seed(0))
    a = (x, l8.router_w, l8.experts_gate_up_w, l8.experts_down_w, 2, True)
    s = dict(gate_up_s=l8.experts_gate_up_s, down_s=l8.experts_down_s)
    got = ops.moe_mlp(*a, **s)
    assert torch.equal(got, ref.moe_mlp(*a, **s))
    deq = [w.double() * sc.double()[..., None] for w, sc in ((a[2], s["gate_up_s"]), (a[3], s["down_s"]))]
    assert torch.equal(got, ref.moe_mlp(x, a[1], *deq, 2, True))
    with pytest.raises(ValueError, match="float8_e4m3fn codes but"):
        ops.moe_mlp(*a)
    with pytest.raises(ValueError, match="together"):
        ops.moe_mlp(*a, gate_up_s=s["gate_up_s"])
    with pytest.raises(ValueError, match="down_s must be float32"):
        ops.moe_mlp(*a, gate_up_s=s["gate_up_s"], down_s=s["down_s"][:, :-1])


def test_experts_dtype_flows_from_configuration_and_environment(monkeypatch):
    from langstream_amd.services import ServiceRegistry
    base = {"device": "cpu", "num-blocks": 16, "use-graphs": "false", "max-model-len": 256, "chat-model": "qwen3-moe-tiny"}

    def engine(**extra):
        reg = ServiceRegistry({**base, **extra})
        try:
            e = reg.llm_engine("qwen3-moe-tiny")
            return e.stats["experts_dtype"], e.model.layers[0].experts_down_w.dtype
        finally:
            reg.shutdown()

    monkeypatch.delenv("LS_EXPERTS_DTYPE", raising=False)
    assert engine() == ("bf16", torch.float32)
    assert engine(**{"experts-dtype": "fp8"}) == ("fp8", ref.FP8_DTYPE)
    monkeypatch.setenv("LS_EXPERTS_DTYPE", "fp8")
    assert engine() == ("fp8", ref.FP8_DTYPE)
    assert engine(**{"experts-dtype": "bf16"}) == ("bf16", torch.float32)   # the key wins over the environment
    with pytest.raises(ValueError, match="dense model"):
        ServiceRegistry({**base, "chat-model": "llama-tiny"}).llm_engine("llama-tiny")
