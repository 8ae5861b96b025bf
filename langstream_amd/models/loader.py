"""Checkpoint loading: HuggingFace -> packed layouts, tensor-parallel sharding, safetensors IO.

The reference loads models inside the remote providers or through DJL
(``AbstractHuggingFaceEmbeddingService.java:42-224``); here weights are packed once into
the GEMM-friendly layouts of ``models/llama.py`` / ``models/bert.py`` and each TP rank
keeps only its shard (a 70B model at TP=8 is ~17.5 GB per MI355X, leaving >250 GB of
HBM for the KV cache).

Only non-executing loaders are used: safetensors, or ``torch.load(weights_only=True)``.
Loading is streamed tensor by tensor (``safe_open``) so host memory stays bounded.
"""
from __future__ import annotations

import glob
import json
import logging
import os
from typing import Dict, Iterable, Optional, Tuple

import torch

from .llama import LlamaConfig, W8_NAMES

log = logging.getLogger(__name__)
FP8 = torch.float8_e4m3fn

# ---------------------------------------------------------------- safetensors IO


def iter_checkpoint(path: str) -> Iterable[Tuple[str, torch.Tensor]]:
    """Yield (name, tensor) from a file or a directory of ``*.safetensors`` (or
    ``*.bin``/``*.pt`` via ``torch.load(weights_only=True)``)."""
    files = [path] if os.path.isfile(path) else sorted(
        glob.glob(os.path.join(path, "*.safetensors")) or glob.glob(os.path.join(path, "*.bin"))
        or glob.glob(os.path.join(path, "*.pt")))
    if not files:
        raise FileNotFoundError(f"no checkpoint files under {path}")
    for f in files:
        if f.endswith(".safetensors"):
            from safetensors import safe_open
            with safe_open(f, framework="pt", device="cpu") as fh:
                for k in fh.keys():
                    yield k, fh.get_tensor(k)
        else:
            sd = torch.load(f, map_location="cpu", weights_only=True)
            yield from sd.items()


def save_packed(sd: Dict[str, torch.Tensor], path: str, metadata: Optional[dict] = None) -> None:
    from safetensors.torch import save_file
    save_file({k: v.detach().contiguous().cpu() for k, v in sd.items()}, path,
              metadata={k: json.dumps(v) for k, v in (metadata or {}).items()})


def load_packed(path: str, device="cpu") -> Dict[str, torch.Tensor]:
    """Load a packed state dict (our names); converts HF checkpoints on the fly."""
    sd = dict(iter_checkpoint(path))
    if any(k.startswith("model.layers.") or k == "model.embed_tokens.weight" for k in sd):
        cfg = llama_config_from_hf(path) if os.path.isdir(path) else None
        sd = convert_hf_llama(sd, cfg)
    elif any(k.startswith(("bert.", "encoder.layer.", "embeddings.")) for k in sd):
        sd = convert_hf_bert(sd)
    return {k: v.to(device) for k, v in sd.items()}


# ---------------------------------------------------------------- Llama


HF_MODEL_TYPES = ("llama", "mistral", "qwen2", "qwen3")   # Llama-architecture families the engine serves


def hf_model_type(model_dir: str) -> str:
    """``model_type`` of a Hugging Face directory's ``config.json`` ("llama" when absent)."""
    with open(os.path.join(model_dir, "config.json")) as f:
        return json.load(f).get("model_type", "llama")


def _checkpoint_names(model_dir: str) -> set:
    """Tensor names of a directory's ``*.safetensors`` (headers only, no tensor is read)."""
    names: set = set()
    for f in sorted(glob.glob(os.path.join(model_dir, "*.safetensors"))):
        from safetensors import safe_open
        with safe_open(f, framework="pt", device="cpu") as fh:
            names.update(fh.keys())
    return names


def _rope_from_hf(c: dict) -> Tuple[float, Optional[dict]]:
    """(base, scaling) from ``rope_parameters`` (transformers 5: base and scaling fields in
    one object) or, without it, the top-level ``rope_theta`` / ``rope_scaling``.  Scaling is
    None or the llama3 fields; any other type raises."""
    rp = c.get("rope_parameters")
    if isinstance(rp, dict):
        theta, sc = rp.get("rope_theta", c.get("rope_theta")), rp
    else:
        theta, sc = c.get("rope_theta"), c.get("rope_scaling")
    kind = (sc.get("rope_type", sc.get("type")) if sc else None) or "default"
    if kind not in ("default", "llama3"):
        raise ValueError(f"unsupported RoPE scaling type {kind!r} (supported: default, llama3)")
    scaling = None
    if kind == "llama3":
        scaling = {"rope_type": "llama3", "factor": float(sc["factor"]),
                   "low_freq_factor": float(sc.get("low_freq_factor", 1.0)),
                   "high_freq_factor": float(sc.get("high_freq_factor", 4.0)),
                   "original_max_position_embeddings": int(sc.get("original_max_position_embeddings", 8192))}
    return float(theta if theta is not None else 10000.0), scaling


LAYER_TYPES = ("full_attention", "sliding_attention")


def _check_quantization_config(c: dict, names: set) -> None:
    """``quantization_config`` is read only to refuse what is known not to fit the W8A16 path
    (per-tensor or per-channel e4m3 weights, bf16 activations, bf16 lm_head); what the
    checkpoint holds is decided by tensor names and dtypes in ``convert_hf_llama``.  The
    field names follow the compressed-tensors and fbgemm_fp8 layouts."""
    q = c.get("quantization_config")
    if any(n.startswith("lm_head.weight_scale") for n in names):
        raise ValueError("quantization_config: the checkpoint quantises lm_head (lm_head.weight_scale); only "
                         "the layer projections may be fp8 (lm_head belongs in ignore / modules_to_not_convert)")
    if not isinstance(q, dict):
        return
    if q.get("weight_block_size"):
        raise ValueError(f"quantization_config.weight_block_size = {q['weight_block_size']!r}: block-wise "
                         f"weight scales are not supported (per-tensor or per-channel only)")
    if q.get("kv_cache_scheme") is not None:
        raise ValueError("quantization_config.kv_cache_scheme is set: checkpoint KV-cache scales are not "
                         "supported (the engine's own kv-cache-dtype option is)")
    for gname, g in (q.get("config_groups") or {}).items():
        w = (g or {}).get("weights") or {}
        where = f"quantization_config.config_groups.{gname}.weights"
        if w.get("num_bits", 8) != 8:
            raise ValueError(f"{where}.num_bits = {w['num_bits']!r}: only 8-bit weights are supported")
        if w.get("type", "float") != "float":
            raise ValueError(f"{where}.type = {w['type']!r}: only float (e4m3) weights are supported")
        if w.get("strategy", "tensor") not in ("tensor", "channel"):
            raise ValueError(f"{where}.strategy = {w['strategy']!r}: only tensor and channel are supported")


def _window_layers_from_hf(c: dict, mtype: str) -> Optional[tuple]:
    """The windowed layer indices of a checkpoint with an active sliding window, None for
    every layer: ``layer_types`` where the config has it, else the family's rule (Mistral:
    every layer; Qwen2 and Qwen3: the layers ``i >= max_window_layers``)."""
    n = int(c["num_hidden_layers"])
    lt = c.get("layer_types")
    if isinstance(lt, (list, tuple)) and lt:
        if len(lt) != n:
            raise ValueError(f"layer_types has {len(lt)} entries for {n} layers")
        layers = tuple(i for i, t in enumerate(lt) if t == "sliding_attention")
    elif mtype in ("qwen2", "qwen3"):
        layers = tuple(range(min(int(c.get("max_window_layers", 28)), n), n))
    else:
        return None
    return None if len(layers) == n else layers


def llama_config_from_hf(model_dir: str, sliding_window: bool = False) -> LlamaConfig:
    """The shape of a Hugging Face ``llama`` / ``mistral`` / ``qwen2`` / ``qwen3`` directory.  Anything
    the engine would compute differently from the checkpoint's own model is refused here
    (other model types, other RoPE scalings, other layer types) or in ``convert_hf_llama``
    (other tensors).

    ``qkv_bias`` is set for ``qwen2`` and for any checkpoint with ``q_proj.bias`` (a ``qwen3``
    one with ``attention_bias``); ``qk_norm`` for ``qwen3`` and for any checkpoint with
    ``self_attn.q_norm.weight``.

    A checkpoint with an active sliding window (Mistral's ``sliding_window``, Qwen2 / Qwen3 with
    ``use_sliding_window``) shorter than ``max_position_embeddings`` is served in one of two
    ways.  ``sliding_window=False`` (the default): as a full-attention model up to the
    window, ``max_position`` clamped to it.  ``True``: over its whole position range, with
    the window in the attention kernels of the layers that have one
    (``LlamaConfig.sliding_window`` / ``window_layers``)."""
    with open(os.path.join(model_dir, "config.json")) as f:
        c = json.load(f)
    mtype = c.get("model_type", "llama")
    if mtype not in HF_MODEL_TYPES:
        raise ValueError(f"unsupported model_type {mtype!r} (supported: {', '.join(HF_MODEL_TYPES)})")
    theta, scaling = _rope_from_hf(c)
    names = _checkpoint_names(model_dir)
    _check_quantization_config(c, names)
    qkv_bias = mtype == "qwen2" or any(n.endswith("self_attn.q_proj.bias") for n in names)
    qk_norm = mtype == "qwen3" or any(n.endswith("self_attn.q_norm.weight") for n in names)
    max_pos = c.get("max_position_embeddings", 8192)
    for t in c.get("layer_types") or ():
        if t not in LAYER_TYPES:
            raise ValueError(f"unsupported layer type {t!r} in layer_types (supported: {', '.join(LAYER_TYPES)})")
    # an active sliding window: full attention equals windowed attention up to the window,
    # so positions past it are not served
    window = c.get("sliding_window")
    if mtype in ("qwen2", "qwen3") and not c.get("use_sliding_window", False):
        window = None
    if mtype == "llama":
        window = None
    win, win_layers = 0, None
    if window and sliding_window and int(window) < max_pos:
        win_layers = _window_layers_from_hf(c, mtype)
        if win_layers is None or len(win_layers) > 0:
            win = int(window)
        else:
            win_layers = None   # no layer is windowed: a full-attention model
    elif window:
        max_pos = min(max_pos, int(window))
    eos = c.get("eos_token_id", 2)
    eos = list(eos) if isinstance(eos, (list, tuple)) else [eos]
    gen = os.path.join(model_dir, "generation_config.json")
    if os.path.exists(gen):
        with open(gen) as f:
            ge = json.load(f).get("eos_token_id")
        for e in (ge if isinstance(ge, list) else [ge]):
            if e is not None and e not in eos:
                eos.append(e)
    eos = [e for e in eos if e is not None]
    bos = c.get("bos_token_id")
    return LlamaConfig(
        name=c.get("_name_or_path") or mtype, vocab_size=c["vocab_size"], hidden_size=c["hidden_size"],
        intermediate_size=c["intermediate_size"], num_layers=c["num_hidden_layers"],
        num_heads=c["num_attention_heads"],
        num_kv_heads=c.get("num_key_value_heads") or c["num_attention_heads"],
        head_dim=c.get("head_dim") or c["hidden_size"] // c["num_attention_heads"],
        rope_theta=theta, rope_scaling=scaling,
        rms_eps=c.get("rms_norm_eps", 1e-5), max_position=max_pos,
        tie_embeddings=bool(c.get("tie_word_embeddings", False)), bos_token_id=1 if bos is None else bos,
        eos_token_ids=tuple(eos), qkv_bias=qkv_bias, qk_norm=qk_norm, sliding_window=win,
        window_layers=win_layers)


def convert_hf_llama(hf: Dict[str, torch.Tensor], cfg: Optional[LlamaConfig] = None) -> Dict[str, torch.Tensor]:
    """HF ``LlamaForCausalLM`` / ``MistralForCausalLM`` / ``Qwen2ForCausalLM`` /
    ``Qwen3ForCausalLM`` names -> packed names (fused qkv / gate_up, ``q/k/v_proj.bias`` fused
    into ``qkv_b``, ``self_attn.q_norm.weight`` / ``k_norm.weight`` as ``q_norm`` / ``k_norm``,
    both or neither).  A checkpoint is loaded whole or refused: a tensor that is not consumed
    (``o_proj.bias``, ``mlp.*.bias``, ...) raises ValueError naming it; ``rotary_emb.inv_freq``
    is the only name skipped."""
    used = set()
    kinds = set()        # {"fp8", "wide"} over every projection: one kind per checkpoint
    dropped = []         # activation-scale tensors consumed and not used

    def take(name):
        used.add(name)
        return hf[name]

    def proj(name):
        """(weight, f32 [N] scale or None) of one ``..._proj``: a float8_e4m3fn weight comes with a
        sibling ``weight_scale`` (scalar, [1], [N] or [N, 1]; per-tensor scales are broadcast)."""
        w = take(name + ".weight")
        for extra in ("input_scale", "input_scale_ub"):
            if name + "." + extra in hf:
                dropped.append(name + "." + extra)
                used.add(name + "." + extra)
        if w.dtype != FP8:
            kinds.add("wide")
            return w, None
        kinds.add("fp8")
        sn = name + ".weight_scale"
        if sn not in hf:
            raise ValueError(f"checkpoint tensor {name + '.weight'!r} is float8_e4m3fn but {sn!r} is missing")
        sc = take(sn).to(torch.float32).reshape(-1)
        if sc.numel() == 1:
            sc = sc.expand(w.shape[0])
        if sc.numel() != w.shape[0]:
            raise ValueError(f"checkpoint tensor {sn!r} has {sc.numel()} elements for {w.shape[0]} output rows "
                             f"(per-tensor or per-channel scales only)")
        if not bool((sc > 0).all()) or not bool(torch.isfinite(sc).all()):
            raise ValueError(f"checkpoint tensor {sn!r} must be positive and finite")
        return w, sc.contiguous()

    def fuse(key, names):
        ws, ss = zip(*[proj(n) for n in names])
        if any(x is None for x in ss) != all(x is None for x in ss):
            raise ValueError(f"checkpoint mixes fp8 and wider projections in {key} ({', '.join(names)})")
        out[f"{key}_w"] = ws[0] if len(ws) == 1 else _cat_rows(ws)
        if ss[0] is not None:
            out[f"{key}_s"] = ss[0] if len(ss) == 1 else torch.cat(ss, 0)

    out = {"embed": take("model.embed_tokens.weight"), "final_norm": take("model.norm.weight")}
    out["lm_head"] = take("lm_head.weight") if "lm_head.weight" in hf else hf["model.embed_tokens.weight"]
    for n in ("embed", "lm_head"):
        if out[n].dtype == FP8:
            raise ValueError(f"checkpoint tensor for {n} is float8_e4m3fn: only the layer projections may be fp8")
    i = 0
    while f"model.layers.{i}.self_attn.q_proj.weight" in hf:
        p = f"model.layers.{i}."
        qkv = [p + f"self_attn.{n}_proj" for n in "qkv"]
        fuse(f"layers.{i}.qkv", qkv)
        if any(n + ".bias" in hf for n in qkv):
            out[f"layers.{i}.qkv_b"] = torch.cat([take(n + ".bias") for n in qkv], 0)
        qn, kn = p + "self_attn.q_norm.weight", p + "self_attn.k_norm.weight"
        if qn in hf or kn in hf:
            for n in (qn, kn):
                if n not in hf:
                    raise ValueError(f"checkpoint tensor {n!r} is missing: q_norm and k_norm come together")
            out[f"layers.{i}.q_norm"] = take(qn)
            out[f"layers.{i}.k_norm"] = take(kn)
        fuse(f"layers.{i}.o", [p + "self_attn.o_proj"])
        fuse(f"layers.{i}.gate_up", [p + "mlp.gate_proj", p + "mlp.up_proj"])
        fuse(f"layers.{i}.down", [p + "mlp.down_proj"])
        out[f"layers.{i}.in_norm"] = take(p + "input_layernorm.weight")
        out[f"layers.{i}.post_norm"] = take(p + "post_attention_layernorm.weight")
        i += 1
    if cfg is not None:
        assert i == cfg.num_layers, f"checkpoint has {i} layers, config {cfg.num_layers}"
    if len(kinds) > 1:
        raise ValueError("checkpoint mixes fp8 (float8_e4m3fn) and wider projection weights; the projections "
                         "of a checkpoint are all fp8 or all bf16 / f16 / f32")
    if dropped:
        log.info("fp8 checkpoint: %d activation-scale tensors (input_scale / input_scale_ub) dropped; "
                 "activations stay bf16 (first: %s)", len(dropped), dropped[0])
    left = sorted(n for n in hf if n not in used and not n.endswith("rotary_emb.inv_freq"))
    if left:
        raise ValueError(f"checkpoint tensor {left[0]!r} is not supported"
                         + (f" (and {len(left) - 1} more)" if len(left) > 1 else ""))
    return out


def _cat_rows(ts) -> torch.Tensor:
    """torch.cat along dim 0 that also takes float8 tensors (as bytes)."""
    if ts[0].dtype == FP8:
        return torch.cat([t.contiguous().view(torch.uint8) for t in ts], 0).view(FP8)
    return torch.cat(list(ts), 0)


def checkpoint_weights_dtype(sd: Dict[str, torch.Tensor]) -> str:
    """"fp8" when the layer projections of a packed state dict are float8_e4m3fn codes, else "bf16"."""
    keys = tuple(f".{n}_w" for n in W8_NAMES)
    return "fp8" if any(k.endswith(keys) and v.dtype == FP8 for k, v in sd.items()) else "bf16"


def shard_llama(sd: Dict[str, torch.Tensor], cfg: LlamaConfig, rank: int, world: int) -> Dict[str, torch.Tensor]:
    """Full packed state dict -> this TP rank's shard: column-parallel qkv / gate_up
    (by heads / by FFN columns), row-parallel o / down, vocab-parallel embed / lm_head
    (padded to a multiple of ``world``), replicated norms (the per-head ``q_norm`` / ``k_norm``
    included: every rank's heads share the one weight).  The row scales of fp8 weights follow
    the rows: ``qkv_s`` / ``gate_up_s`` are sliced like ``qkv_w`` / ``gate_up_w``; ``o_s`` /
    ``down_s`` are replicated (those weights are cut along K, every rank keeps all rows)."""
    if world == 1:
        return dict(sd)
    from .llama import tp_kv_heads
    D = cfg.head_dim
    hq, hkv, f = cfg.num_heads // world, tp_kv_heads(cfg.num_kv_heads, world), cfg.intermediate_size // world
    # first KV head of this rank (replicated heads when world > num_kv_heads)
    kv0 = rank * hkv if cfg.num_kv_heads >= world else rank // (world // cfg.num_kv_heads)
    Hq, Hkv, F = cfg.num_heads * D, cfg.num_kv_heads * D, cfg.intermediate_size
    vpr = (cfg.vocab_size + world - 1) // world
    out = {}
    for k, v in sd.items():
        if k.endswith((".qkv_w", ".qkv_b", ".qkv_s")):   # bias and scales are sliced like the rows they belong to
            q, kk, vv = v[:Hq], v[Hq: Hq + Hkv], v[Hq + Hkv:]
            out[k] = _cat_rows([q[rank * hq * D:(rank + 1) * hq * D], kk[kv0 * D:(kv0 + hkv) * D],
                                vv[kv0 * D:(kv0 + hkv) * D]])
        elif k.endswith(".o_w"):
            out[k] = v[:, rank * hq * D:(rank + 1) * hq * D]
        elif k.endswith((".gate_up_w", ".gate_up_s")):
            g, u = v[:F], v[F:]
            out[k] = _cat_rows([g[rank * f:(rank + 1) * f], u[rank * f:(rank + 1) * f]])
        elif k.endswith(".down_w"):
            out[k] = v[:, rank * f:(rank + 1) * f]
        elif k in ("embed", "lm_head"):
            part = v[rank * vpr:(rank + 1) * vpr]
            if part.shape[0] < vpr:
                part = torch.cat([part, part.new_zeros(vpr - part.shape[0], v.shape[1])], 0)
            out[k] = part
        else:
            out[k] = v
    return {k: v.contiguous() for k, v in out.items()}


# ---------------------------------------------------------------- BERT


def convert_hf_bert(hf: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """HF ``BertModel`` names (with or without the ``bert.`` prefix) -> packed names."""
    def g(name):
        for p in ("", "bert.", "model."):
            if p + name in hf:
                return hf[p + name]
        raise KeyError(name)

    out = {"wte": g("embeddings.word_embeddings.weight"), "wpe": g("embeddings.position_embeddings.weight"),
           "wtt": g("embeddings.token_type_embeddings.weight"), "emb_g": g("embeddings.LayerNorm.weight"),
           "emb_b": g("embeddings.LayerNorm.bias")}
    i = 0
    while True:
        p = f"encoder.layer.{i}."
        try:
            q = g(p + "attention.self.query.weight")
        except KeyError:
            break
        out[f"layers.{i}.qkv_w"] = torch.cat([q, g(p + "attention.self.key.weight"),
                                              g(p + "attention.self.value.weight")], 0)
        out[f"layers.{i}.qkv_b"] = torch.cat([g(p + "attention.self.query.bias"), g(p + "attention.self.key.bias"),
                                              g(p + "attention.self.value.bias")], 0)
        out[f"layers.{i}.o_w"] = g(p + "attention.output.dense.weight")
        out[f"layers.{i}.o_b"] = g(p + "attention.output.dense.bias")
        out[f"layers.{i}.ln1_g"] = g(p + "attention.output.LayerNorm.weight")
        out[f"layers.{i}.ln1_b"] = g(p + "attention.output.LayerNorm.bias")
        out[f"layers.{i}.ff1_w"] = g(p + "intermediate.dense.weight")
        out[f"layers.{i}.ff1_b"] = g(p + "intermediate.dense.bias")
        out[f"layers.{i}.ff2_w"] = g(p + "output.dense.weight")
        out[f"layers.{i}.ff2_b"] = g(p + "output.dense.bias")
        out[f"layers.{i}.ln2_g"] = g(p + "output.LayerNorm.weight")
        out[f"layers.{i}.ln2_b"] = g(p + "output.LayerNorm.bias")
        i += 1
    return out
