"""Mixture-of-experts models on the CPU: a tiny Qwen3-MoE and a tiny Mixtral from the installed
``transformers``, written as checkpoint directories with the hub's per-expert tensor names, read
back through models.loader and compared with the library's logits in f32.  Nothing is fetched."""
from __future__ import annotations

import json
import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import pytest  # noqa: E402
import torch  # noqa: E402

from langstream_amd.models.llama import PRESETS, LlamaModel, TPInfo  # noqa: E402
from langstream_amd.models.loader import llama_config_from_hf, load_packed  # noqa: E402
from test_qk_norm_cpu import BOUND, IDS, SHAPE, _hf_logits, _our_logits  # noqa: E402

HUB = {"qwen3_moe": ("mlp", "gate_proj", "up_proj", "down_proj"), "mixtral": ("block_sparse_moe", "w1", "w3", "w2")}


def _save(path, family: str, **extra):
    """A tiny random f32 model of the family, saved under the hub's tensor names (one tensor per
    expert and projection), whatever layout the installed transformers keeps in memory."""
    import transformers as tf
    from safetensors.torch import save_file
    torch.manual_seed(0)
    rope = {"rope_theta": 1e6, "rope_type": "default"}
    if family == "qwen3_moe":
        cfg = tf.Qwen3MoeConfig(**SHAPE, head_dim=64, rope_parameters=rope, num_experts=8, num_experts_per_tok=2,
                                moe_intermediate_size=128, decoder_sparse_step=1, mlp_only_layers=[], **extra)
        model = tf.Qwen3MoeForCausalLM(cfg)
    else:
        cfg = tf.MixtralConfig(**{**SHAPE, "intermediate_size": 192}, rope_parameters=rope, num_local_experts=4,
                               num_experts_per_tok=2, **extra)
        model = tf.MixtralForCausalLM(cfg)
    model = model.float().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(".gate.weight"):
                p.normal_(0.0, 1.0)   # a router that decides: the library's init leaves all experts near 1 / E
    block, gate, up, down = HUB[family]
    sd = {}
    for n, t in model.state_dict().items():
        n = n.replace(".mlp.", f".{block}.")
        if n.endswith(".experts.gate_up_proj"):
            for e, (g, u) in enumerate(zip(*t.chunk(2, dim=1))):
                sd[n.replace("gate_up_proj", f"{e}.{gate}.weight")] = g.contiguous()
                sd[n.replace("gate_up_proj", f"{e}.{up}.weight")] = u.contiguous()
        elif n.endswith(".experts.down_proj"):
            for e, d in enumerate(t):
                sd[n.replace("down_proj", f"{e}.{down}.weight")] = d.contiguous()
        else:
            sd[n] = t.contiguous()
    cfg.save_pretrained(str(path))
    save_file(sd, os.path.join(str(path), "model.safetensors"))
    return model


@pytest.mark.parametrize("family,norm", [("qwen3_moe", True), ("qwen3_moe", False), ("mixtral", True)])
def test_moe_logits_match_transformers(tmp_path, family, norm):
    hf = _save(tmp_path, family, **({"norm_topk_prob": norm} if family == "qwen3_moe" else {}))
    cfg = llama_config_from_hf(str(tmp_path))
    assert (cfg.num_experts, cfg.experts_per_token, cfg.moe_intermediate_size, cfg.norm_topk_prob, cfg.qk_norm) == (
        (8, 2, 128, norm, True) if family == "qwen3_moe" else (4, 2, 192, True, False))
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32)
    sd = load_packed(str(tmp_path))
    assert sd["layers.1.experts_gate_up_w"].shape == (cfg.num_experts, 2 * cfg.moe_intermediate_size, 256)
    model.load_state_dict(sd)
    assert cfg.num_params == sum(v.numel() for v in model.state_dict().values())
    assert model.weight_bytes == 4 * cfg.num_params
    ours = _our_logits(model, IDS)
    err = (ours - _hf_logits(hf, IDS)).abs().max().item()
    model.layers[0].router_w.copy_(model.layers[0].router_w.flip(0))   # other experts: the routes matter
    moved = (_our_logits(model, IDS) - ours).abs().max().item()
    print(f"{family} norm_topk={norm}: max |logits - transformers| {err:.3g}; a permuted router moves ours by {moved:.3g}")
    assert err <= BOUND
    assert moved > 100 * BOUND


@pytest.mark.parametrize("key,value,match", [
    ("decoder_sparse_step", 2, "decoder_sparse_step"), ("mlp_only_layers", [0], "mlp_only_layers"),
    ("shared_expert_intermediate_size", 64, "shared_expert_intermediate_size"),
    ("quantization_config", {"quant_method": "fp8"}, "quantization_config"), ("num_experts", None, "num_experts")])
def test_refused_config_keys(tmp_path, key, value, match):
    base = dict(SHAPE, model_type="qwen3_moe", head_dim=64, num_experts=8, num_experts_per_tok=2,
                moe_intermediate_size=128, norm_topk_prob=True)
    with open(tmp_path / "config.json", "w") as f:
        json.dump({**base, key: value}, f)
    with pytest.raises(ValueError, match=match):
        llama_config_from_hf(str(tmp_path))


@pytest.mark.parametrize("kw,match", [(dict(weights_dtype="fp8"), "fp8 or int4"), (dict(weights_dtype="int4"), "fp8 or int4"),
                                      (dict(tp=TPInfo(0, 2, None)), "tensor parallelism")])
def test_refused_model_options(kw, match):
    with pytest.raises(ValueError, match=match):
        LlamaModel(PRESETS["qwen3-moe-tiny"], device="cpu", dtype=torch.float32, **kw)
