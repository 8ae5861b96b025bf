"""Int4 expert weights above the kernel, on the CPU: ops.reference.moe_mlp with zero points, the model's
quantiser, state dicts in both forms, the load refusals, and the experts-dtype configuration key."""
import pytest
import torch

from langstream_amd import ops
from langstream_amd.models.llama import EXPERT_NAMES, LlamaModel, PRESETS, int4_group
from langstream_amd.ops import reference as ref

MOE = PRESETS["qwen3-moe-tiny"]


def _model(seed=0, **kw):
    return LlamaModel(MOE, device="cpu", dtype=torch.float32, seed=seed, **kw)


def _same(a: dict, b: dict) -> bool:
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


def test_reference_with_zero_points_is_the_reference_on_the_dequantised_weights():
    l4 = _model(experts_dtype="int4").layers[0]
    x = torch.randn(9, MOE.hidden_size, generator=torch.Generator().manual_seed(0))
    a = (x, l4.router_w, l4.experts_gate_up_w, l4.experts_down_w, 2, True)
    q = dict(gate_up_s=l4.experts_gate_up_s, down_s=l4.experts_down_s, gate_up_z=l4.experts_gate_up_z,
             down_z=l4.experts_down_z)
    got = ops.moe_mlp(*a, **q)
    assert torch.equal(got, ref.moe_mlp(*a, **q))
    deq = [torch.stack([ref.dequantize_weight_int4(w[e], s[e], z[e], torch.float64) for e in range(w.shape[0])])
           for w, s, z in ((a[2], q["gate_up_s"], q["gate_up_z"]), (a[3], q["down_s"], q["down_z"]))]
    assert torch.equal(got, ref.moe_mlp(x, a[1], *deq, 2, True))
    for drop, match in ((("gate_up_s", "down_s"), "need the scales"), (("down_z",), "together"),
                        (tuple(q), "uint8 int4 codes but no scales")):
        with pytest.raises(ValueError, match=match):
            ops.moe_mlp(*a, **{k: v for k, v in q.items() if k not in drop})
    with pytest.raises(ValueError, match="down_z must be uint8"):
        ops.moe_mlp(*a, **{**q, "down_z": q["down_z"][:, :-1]})
    with pytest.raises(ValueError, match="gate_up_s must be float32"):
        ops.moe_mlp(*a, **{**q, "gate_up_s": q["gate_up_s"].double()})


@pytest.mark.parametrize("form", ["wide", "codes"])
def test_state_dict_round_trip_and_load_refusals(form):
    wide, m4, other = _model(), _model(experts_dtype="int4"), _model(seed=1, experts_dtype="int4")
    for lw, l4 in zip(wide.layers, m4.layers):   # the constructor's rule: quantize_weight_int4 over the E N rows
        for n in EXPERT_NAMES:
            w = getattr(lw, n + "_w")
            E, N, K = w.shape
            c, s, z = ref.quantize_weight_int4(w.reshape(E * N, K), int4_group(n, N, K))
            assert torch.equal(getattr(l4, n + "_w"), c.view(E, N, K // 2))
            assert torch.equal(getattr(l4, n + "_s"), s.view(E, N, -1)) and torch.equal(getattr(l4, n + "_z"), z.view(E, N, -1))
        assert torch.equal(lw.qkv_w, l4.qkv_w) and torch.equal(lw.router_w, l4.router_w)   # everything else as it was
    assert m4.weight_bytes < _model(experts_dtype="fp8").weight_bytes
    sd = m4.state_dict()
    assert not _same(other.state_dict(), sd)
    other.load_state_dict(wide.state_dict() if form == "wide" else sd)
    assert _same(other.state_dict(), sd)
    key = "layers.0.experts_gate_up"
    for model in (_model(), _model(experts_dtype="fp8")):
        with pytest.raises(ValueError, match=key + "_w holds int4 codes but the model's experts_dtype"):
            model.load_state_dict(sd)
    with pytest.raises(ValueError, match=key + "_w holds float8_e4m3fn codes but the model's experts_dtype is 'int4'"):
        other.load_state_dict(_model(experts_dtype="fp8").state_dict())
    for suffix in ("_s", "_z"):
        with pytest.raises(ValueError, match=key + suffix + " is missing"):
            other.load_state_dict({k: v for k, v in sd.items() if k != key + suffix})


def test_experts_dtype_int4_flows_from_configuration_and_environment(monkeypatch):
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
    assert engine(**{"experts-dtype": "int4"}) == ("int4", torch.uint8)
    monkeypatch.setenv("LS_EXPERTS_DTYPE", "int4")
    assert engine() == ("int4", torch.uint8)
    assert engine(**{"experts-dtype": "bf16"}) == ("bf16", torch.float32)   # the key wins over the environment
    with pytest.raises(ValueError, match="expected bf16, fp8 or int4"):
        engine(**{"experts-dtype": "int8"})


@pytest.mark.parametrize("kw,match", [
    (dict(weights_dtype="fp8"), "fp8 or int4"), (dict(weights_dtype="int4"), "experts_dtype"),
    (dict(weights_dtype="mxfp4"), "mixture-of-experts.*mxfp4"), (dict(weights_dtype="fp8", activations_dtype="fp8"), "fp8 or int4"),
    (dict(cfg=PRESETS["llama-tiny"]), "dense model")])
def test_what_stays_refused_with_int4_experts(kw, match):
    kw = dict(kw)
    with pytest.raises(ValueError, match=match):
        LlamaModel(kw.pop("cfg", MOE), device="cpu", dtype=torch.float32, experts_dtype="int4", **kw)
