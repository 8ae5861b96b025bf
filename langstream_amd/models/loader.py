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
        sd = convert_hf_llama(sd, cfg, hf_quantization_config(path) if os.path.isdir(path) else None)
    elif any(k.startswith(("bert.", "encoder.layer.", "embeddings.")) for k in sd):
        sd = convert_hf_bert(sd)
    return {k: v.to(device) for k, v in sd.items()}


# ---------------------------------------------------------------- Llama


# Llama-architecture families the engine serves; the last two have a mixture-of-experts MLP
HF_MODEL_TYPES = ("llama", "mistral", "qwen2", "qwen3", "qwen3_moe", "mixtral")
MOE_MODEL_TYPES = ("qwen3_moe", "mixtral")


def hf_model_type(model_dir: str) -> str:
    """``model_type`` of a Hugging Face directory's ``config.json`` ("llama" when absent)."""
    with open(os.path.join(model_dir, "config.json")) as f:
        return json.load(f).get("model_type", "llama")


def hf_quantization_config(model_dir: str) -> Optional[dict]:
    """``quantization_config`` of a Hugging Face directory's ``config.json`` (None when absent)."""
    with open(os.path.join(model_dir, "config.json")) as f:
        q = json.load(f).get("quantization_config")
    return q if isinstance(q, dict) else None


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
    elif mtype in ("qwen2", "qwen3", "qwen3_moe"):
        layers = tuple(range(min(int(c.get("max_window_layers", 28)), n), n))
    else:
        return None
    return None if len(layers) == n else layers


def _moe_from_hf(c: dict, mtype: str) -> dict:
    """The mixture-of-experts fields of a ``qwen3_moe`` / ``mixtral`` config ({} for a dense
    family).  Every layer must be sparse and nothing but routed experts may feed the MLP
    output; a config that says otherwise is refused by the name of its key."""
    if mtype not in MOE_MODEL_TYPES:
        return {}
    # the expert count goes by either name, whatever the family (the library writes both forms)
    ekey = "num_experts" if c.get("num_experts") else "num_local_experts"
    for key in (ekey, "num_experts_per_tok"):
        if not c.get(key):
            raise ValueError(f"model_type {mtype!r}: config.json has no "
                             f"{'num_experts / num_local_experts' if key == ekey else key}")
    if c.get("decoder_sparse_step", 1) != 1:
        raise ValueError(f"decoder_sparse_step = {c['decoder_sparse_step']!r}: only models whose every layer is a "
                         f"mixture of experts are supported (decoder_sparse_step = 1)")
    if c.get("mlp_only_layers"):
        raise ValueError(f"mlp_only_layers = {c['mlp_only_layers']!r}: dense layers inside a mixture-of-experts "
                         f"model are not supported")
    for key in ("shared_expert_intermediate_size", "n_shared_experts", "num_shared_experts"):
        if c.get(key):
            raise ValueError(f"{key} = {c[key]!r}: shared experts are not supported")
    if c.get("quantization_config"):
        raise ValueError("quantization_config: a quantised mixture-of-experts checkpoint is not supported "
                         "(bf16 / f16 / f32 experts only)")
    F = c.get("moe_intermediate_size") if mtype == "qwen3_moe" else c.get("intermediate_size")
    if not F:
        raise ValueError(f"model_type {mtype!r}: config.json has no "
                         f"{'moe_intermediate_size' if mtype == 'qwen3_moe' else 'intermediate_size'}")
    return dict(num_experts=int(c[ekey]), experts_per_token=int(c["num_experts_per_tok"]),
                moe_intermediate_size=int(F),
                norm_topk_prob=True if mtype == "mixtral" else bool(c.get("norm_topk_prob", False)))


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
    moe = _moe_from_hf(c, mtype)
    names = _checkpoint_names(model_dir)
    _check_quantization_config(c, names)
    qkv_bias = mtype == "qwen2" or any(n.endswith("self_attn.q_proj.bias") for n in names)
    qk_norm = mtype in ("qwen3", "qwen3_moe") or any(n.endswith("self_attn.q_norm.weight") for n in names)
    max_pos = c.get("max_position_embeddings", 8192)
    for t in c.get("layer_types") or ():
        if t not in LAYER_TYPES:
            raise ValueError(f"unsupported layer type {t!r} in layer_types (supported: {', '.join(LAYER_TYPES)})")
    # an active sliding window: full attention equals windowed attention up to the window,
    # so positions past it are not served
    window = c.get("sliding_window")
    if mtype in ("qwen2", "qwen3", "qwen3_moe") and not c.get("use_sliding_window", False):
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
        intermediate_size=c.get("intermediate_size") or moe["moe_intermediate_size"], num_layers=c["num_hidden_layers"],
        num_heads=c["num_attention_heads"],
        num_kv_heads=c.get("num_key_value_heads") or c["num_attention_heads"],
        head_dim=c.get("head_dim") or c["hidden_size"] // c["num_attention_heads"],
        rope_theta=theta, rope_scaling=scaling,
        rms_eps=c.get("rms_norm_eps", 1e-5), max_position=max_pos,
        tie_embeddings=bool(c.get("tie_word_embeddings", False)), bos_token_id=1 if bos is None else bos,
        eos_token_ids=tuple(eos), qkv_bias=qkv_bias, qk_norm=qk_norm, sliding_window=win,
        window_layers=win_layers, **moe)


AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)   # nibble i of an AWQ word holds column 8 * col + AWQ_ORDER[i]


def _unpack_nibbles(t: torch.Tensor, order=None) -> torch.Tensor:
    """int32 [R, C] -> uint8 [R, 8 C]: nibble i (lowest first) of word c is column 8 c + i, or
    with ``order`` column 8 c + order[i]."""
    nib = ((t.to(torch.int32).unsqueeze(-1) >> (4 * torch.arange(8, dtype=torch.int32))) & 15).to(torch.uint8)
    if order is not None:
        placed = torch.empty_like(nib)
        placed[..., list(order)] = nib
        nib = placed
    return nib.reshape(t.shape[0], 8 * t.shape[1])


def _int4_scheme(q: Optional[dict]) -> Tuple[str, int, int]:
    """(method, group_size, zero offset) of the ``quantization_config`` of a checkpoint with
    ``qweight`` tensors: GPTQ (4 bits, no ``desc_act``; ``checkpoint_format`` "gptq" stores
    zero - 1, "gptq_v2" the zero point) or AWQ (4 bits, version "gemm", with zero points).
    Everything else is refused by the name of the field."""
    if not isinstance(q, dict):
        raise ValueError("the checkpoint holds qweight tensors but config.json has no quantization_config "
                         "(gptq or awq expected)")
    method = str(q.get("quant_method", "")).lower()
    if method not in ("gptq", "awq"):
        raise ValueError(f"quantization_config.quant_method = {q.get('quant_method')!r}: qweight tensors are "
                         f"supported for gptq and awq only")
    if q.get("bits") != 4:
        raise ValueError(f"quantization_config.bits = {q.get('bits')!r}: only 4-bit {method} weights are supported")
    off = 0
    if method == "gptq":
        if q.get("desc_act", False):
            raise ValueError("quantization_config.desc_act = true: activation-ordered GPTQ groups are not "
                             "supported (g_idx must be k // group_size)")
        fmt = q.get("checkpoint_format") or "gptq"
        if fmt not in ("gptq", "gptq_v2"):
            raise ValueError(f"quantization_config.checkpoint_format = {fmt!r}: expected gptq or gptq_v2")
        off = 1 if fmt == "gptq" else 0
    else:
        if str(q.get("version", "gemm")).lower() != "gemm":
            raise ValueError(f"quantization_config.version = {q.get('version')!r}: only the AWQ gemm layout is "
                             f"supported")
        if not q.get("zero_point", True):
            raise ValueError("quantization_config.zero_point = false: symmetric AWQ checkpoints are not supported")
    return method, int(q.get("group_size", 128)), off


def _int4_proj(hf, take, name: str, scheme) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One AWQ / GPTQ ``..._proj`` -> (codes uint8 [N, K / 2], scale f32 [N, K / G], zero uint8
    [N, K / G]) in the layout of ops.reference.pack_weight_int4."""
    from ..ops import reference as ref
    method, gs, off = scheme
    for part in ("qzeros", "scales"):
        if f"{name}.{part}" not in hf:
            raise ValueError(f"checkpoint tensor {name + '.qweight'!r} comes without {name + '.' + part!r}")
    qw, qz, sc = take(name + ".qweight"), take(name + ".qzeros"), take(name + ".scales")
    if qw.dtype != torch.int32 or qz.dtype != torch.int32 or qw.dim() != 2 or qz.dim() != 2 or sc.dim() != 2:
        raise ValueError(f"checkpoint tensors {name}.qweight / .qzeros must be 2-D int32 and .scales 2-D")
    if method == "gptq":
        q = _unpack_nibbles(qw.t().contiguous())                     # [K / 8, N] -> [N, K]
        zero = _unpack_nibbles(qz).to(torch.int32) + off             # [K / G, N]
    else:
        q = _unpack_nibbles(qw, AWQ_ORDER).t().contiguous()          # [K, N / 8] -> [N, K]
        zero = _unpack_nibbles(qz, AWQ_ORDER).to(torch.int32)
    N, K = q.shape
    G = K if gs == -1 else gs
    if G <= 0 or G % 64 or K % G:
        raise ValueError(f"quantization_config.group_size = {gs} for {name} with K = {K}: the group size must be "
                         f"a multiple of 64 that divides K (or -1: one group per row)")
    if tuple(sc.shape) != (K // G, N) or tuple(zero.shape) != (K // G, N):
        raise ValueError(f"checkpoint tensors {name}.scales {tuple(sc.shape)} / .qzeros do not have K / G = "
                         f"{K // G} rows and N = {N} columns")
    if int(zero.max()) > 15:
        raise ValueError(f"checkpoint tensor {name + '.qzeros'!r} holds a zero point of 16 (stored 15 in the "
                         f"gptq format): outside 0..15, not supported")
    if name + ".g_idx" in hf:
        if not torch.equal(take(name + ".g_idx").to(torch.int64), torch.arange(K) // G):
            raise ValueError(f"checkpoint tensor {name + '.g_idx'!r} is not k // group_size: activation-ordered "
                             f"groups are not supported")
    scale = sc.t().to(torch.float32).contiguous()
    if not bool((scale > 0).all()) or not bool(torch.isfinite(scale).all()):
        raise ValueError(f"checkpoint tensor {name + '.scales'!r} must be positive and finite")
    return ref.pack_weight_int4(q), scale, zero.t().to(torch.uint8).contiguous()


def convert_hf_llama(hf: Dict[str, torch.Tensor], cfg: Optional[LlamaConfig] = None,
                     quantization: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """HF ``LlamaForCausalLM`` / ``MistralForCausalLM`` / ``Qwen2ForCausalLM`` /
    ``Qwen3ForCausalLM`` names -> packed names (fused qkv / gate_up, ``q/k/v_proj.bias`` fused
    into ``qkv_b``, ``self_attn.q_norm.weight`` / ``k_norm.weight`` as ``q_norm`` / ``k_norm``,
    both or neither).  A checkpoint is loaded whole or refused: a tensor that is not consumed
    (``o_proj.bias``, ``mlp.*.bias``, ...) raises ValueError naming it; ``rotary_emb.inv_freq``
    is the only name skipped.

    AWQ and GPTQ checkpoints (``..._proj.qweight`` / ``.qzeros`` / ``.scales``; ``quantization``
    is the ``quantization_config`` of their ``config.json``, see ``_int4_scheme``) become int4
    triples ``{key}_w`` / ``_s`` / ``_z`` in the layout of ``ops.reference.pack_weight_int4``."""
    used = set()
    scheme = _int4_scheme(quantization) if any(n.endswith(".qweight") for n in hf) else None
    if "lm_head.qweight" in hf:
        raise ValueError("checkpoint tensor 'lm_head.qweight': a quantised lm_head is not supported; only the "
                         "layer projections may be int4")
    kinds = set()        # {"fp8", "wide"} over every projection: one kind per checkpoint
    dropped = []         # activation-scale tensors consumed and not used

    def take(name):
        used.add(name)
        return hf[name]

    def proj(name):
        """(weight, f32 [N] scale or None) of one ``..._proj``: a float8_e4m3fn weight comes with a
        sibling ``weight_scale`` (scalar, [1], [N] or [N, 1]; per-tensor scales are broadcast)."""
        if name + ".qweight" in hf:
            kinds.add("int4")
            return _int4_proj(hf, take, name, scheme)
        w = take(name + ".weight")
        for extra in ("input_scale", "input_scale_ub"):
            if name + "." + extra in hf:
                dropped.append(name + "." + extra)
                used.add(name + "." + extra)
        if w.dtype != FP8:
            kinds.add("wide")
            return w, None, None
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
        return w, sc.contiguous(), None

    def fuse(key, names):
        ws, ss, zs = zip(*[proj(n) for n in names])
        if any(x is None for x in zs) != all(x is None for x in zs):
            raise ValueError(f"checkpoint mixes int4 and wider projections in {key} ({', '.join(names)})")
        if zs[0] is not None:
            out[f"{key}_w"], out[f"{key}_s"], out[f"{key}_z"] = (torch.cat(t, 0) for t in (ws, ss, zs))
            return
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
    while any(f"model.layers.{i}.self_attn.q_proj.{w}" in hf for w in ("weight", "qweight")):
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
        if not _moe_layer(hf, take, out, i):
            fuse(f"layers.{i}.gate_up", [p + "mlp.gate_proj", p + "mlp.up_proj"])
            fuse(f"layers.{i}.down", [p + "mlp.down_proj"])
        out[f"layers.{i}.in_norm"] = take(p + "input_layernorm.weight")
        out[f"layers.{i}.post_norm"] = take(p + "post_attention_layernorm.weight")
        i += 1
    if cfg is not None:
        assert i == cfg.num_layers, f"checkpoint has {i} layers, config {cfg.num_layers}"
    if "int4" in kinds and len(kinds) > 1:
        raise ValueError("checkpoint mixes int4 (qweight) and other projection weights; the projections of a "
                         "checkpoint are all int4, all fp8 or all bf16 / f16 / f32")
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


# per-expert hub names of the two MoE families: (block, gate, up, down)
_MOE_NAMES = (("mlp", "gate_proj", "up_proj", "down_proj"), ("block_sparse_moe", "w1", "w3", "w2"))


def _moe_layer(hf, take, out, i: int) -> bool:
    """The mixture-of-experts MLP of layer i, if the checkpoint has one: the router
    (``{block}.gate.weight``) and the experts, per expert under the hub names
    (Qwen3-MoE ``mlp.experts.{e}.gate_proj / up_proj / down_proj.weight``, Mixtral
    ``block_sparse_moe.experts.{e}.w1 / w3 / w2.weight``) or already stacked
    (``{block}.experts.gate_up_proj`` [E, 2F, H] and ``.down_proj`` [E, H, F]), become
    ``router_w`` [E, H], ``experts_gate_up_w`` [E, 2F, H] (gate rows, then up rows) and
    ``experts_down_w`` [E, H, F].  Quantised experts and shared experts are refused by name."""
    p = f"model.layers.{i}."
    for block, gate, up, down in _MOE_NAMES:
        b = p + block + "."
        if b + "gate.weight" not in hf:
            continue
        for n in hf:
            if n.startswith(b) and ("shared_expert" in n or n.endswith((".qweight", ".weight_scale", ".scales"))):
                raise ValueError(f"checkpoint tensor {n!r}: shared experts and quantised experts are not supported")
        router = take(b + "gate.weight")
        if b + "experts.gate_up_proj" in hf:
            gu, dn = take(b + "experts.gate_up_proj"), take(b + "experts.down_proj")
        else:
            E = router.shape[0]
            for e in range(E):
                for part in (gate, up, down):
                    if f"{b}experts.{e}.{part}.weight" not in hf:
                        raise ValueError(f"checkpoint tensor {b}experts.{e}.{part}.weight is missing "
                                         f"({b}gate.weight routes over {E} experts)")
            gu = torch.stack([torch.cat([take(f"{b}experts.{e}.{gate}.weight"), take(f"{b}experts.{e}.{up}.weight")], 0)
                              for e in range(E)])
            dn = torch.stack([take(f"{b}experts.{e}.{down}.weight") for e in range(E)])
        E, H = router.shape
        for n, t in ((b + "experts gate_up", gu), (b + "experts down", dn)):
            if t.dtype == FP8 or not t.is_floating_point():
                raise ValueError(f"checkpoint tensors {n} are {t.dtype}: quantised experts are not supported")
        if gu.dim() != 3 or dn.dim() != 3 or gu.shape[0] != E or dn.shape[0] != E or gu.shape[2] != H or \
                dn.shape[1] != H or gu.shape[1] != 2 * dn.shape[2]:
            raise ValueError(f"checkpoint tensors under {b}experts have shapes {tuple(gu.shape)} / {tuple(dn.shape)}, "
                             f"expected [E, 2F, H] / [E, H, F] with E = {E}, H = {H}")
        out[f"layers.{i}.router_w"] = router
        out[f"layers.{i}.experts_gate_up_w"] = gu.contiguous()
        out[f"layers.{i}.experts_down_w"] = dn.contiguous()
        return True
    return False


def _cat_rows(ts) -> torch.Tensor:
    """torch.cat along dim 0 that also takes float8 tensors (as bytes)."""
    if ts[0].dtype == FP8:
        return torch.cat([t.contiguous().view(torch.uint8) for t in ts], 0).view(FP8)
    return torch.cat(list(ts), 0)


def checkpoint_weights_dtype(sd: Dict[str, torch.Tensor]) -> str:
    """"fp8" when the layer projections of a packed state dict are float8_e4m3fn codes, "int4"
    when they are packed 4-bit codes with zero points (``{name}_z``), "mxfp4" when they are uint8
    codes without zero points (packed e2m1 with E8M0 block scales ``{name}_s``), else "bf16"."""
    if any(k.endswith(tuple(f".{n}_z" for n in W8_NAMES)) for k in sd):
        return "int4"
    keys = tuple(f".{n}_w" for n in W8_NAMES)
    if any(k.endswith(keys) and v.dtype == torch.uint8 for k, v in sd.items()):
        return "mxfp4"
    return "fp8" if any(k.endswith(keys) and v.dtype == FP8 for k, v in sd.items()) else "bf16"


def shard_llama(sd: Dict[str, torch.Tensor], cfg: LlamaConfig, rank: int, world: int) -> Dict[str, torch.Tensor]:
    """Full packed state dict -> this TP rank's shard: column-parallel qkv / gate_up
    (by heads / by FFN columns), row-parallel o / down, vocab-parallel embed / lm_head
    (padded to a multiple of ``world``), replicated norms (the per-head ``q_norm`` / ``k_norm``
    included: every rank's heads share the one weight).  The row scales of fp8 weights follow
    the rows: ``qkv_s`` / ``gate_up_s`` are sliced like ``qkv_w`` / ``gate_up_w``; ``o_s`` /
    ``down_s`` are replicated (those weights are cut along K, every rank keeps all rows).

    int4 weights (``{name}_z`` present): the column shards cut codes, scales and zero points by
    rows; the row shards ``o`` / ``down`` cut all three along K -- bytes of two codes, columns
    of one group -- and are refused unless K / world is a multiple of the group size."""
    if world == 1:
        return dict(sd)

    def k_cut(k, v, lo, hi):
        """Columns [lo, hi) of K of an ``o`` / ``down`` tensor (int4: codes, scales or zero points)."""
        base = k[:-2]
        if base + "_z" not in sd:
            return v[:, lo:hi] if k.endswith("_w") else v     # bf16 / fp8: the row scales are replicated
        K, NG = 2 * sd[base + "_w"].shape[1], sd[base + "_s"].shape[1]
        G = K // NG
        if lo % G or hi % G:
            raise ValueError(f"{base}_w: K / TP = {hi - lo} is not a multiple of the int4 group size {G}; this "
                             f"TP degree cannot shard the checkpoint")
        return v[:, lo // 2:hi // 2] if k.endswith("_w") else v[:, lo // G:hi // G]

    from .llama import tp_kv_heads
    D = cfg.head_dim
    hq, hkv, f = cfg.num_heads // world, tp_kv_heads(cfg.num_kv_heads, world), cfg.intermediate_size // world
    # first KV head of this rank (replicated heads when world > num_kv_heads)
    kv0 = rank * hkv if cfg.num_kv_heads >= world else rank // (world // cfg.num_kv_heads)
    Hq, Hkv, F = cfg.num_heads * D, cfg.num_kv_heads * D, cfg.intermediate_size
    vpr = (cfg.vocab_size + world - 1) // world
    out = {}
    for k, v in sd.items():
        if k.endswith((".qkv_w", ".qkv_b", ".qkv_s", ".qkv_z")):   # bias and scales are sliced like the rows they belong to
            q, kk, vv = v[:Hq], v[Hq: Hq + Hkv], v[Hq + Hkv:]
            out[k] = _cat_rows([q[rank * hq * D:(rank + 1) * hq * D], kk[kv0 * D:(kv0 + hkv) * D],
                                vv[kv0 * D:(kv0 + hkv) * D]])
        elif k.endswith((".o_w", ".o_s", ".o_z")):
            out[k] = k_cut(k, v, rank * hq * D, (rank + 1) * hq * D)
        elif k.endswith((".gate_up_w", ".gate_up_s", ".gate_up_z")):
            g, u = v[:F], v[F:]
            out[k] = _cat_rows([g[rank * f:(rank + 1) * f], u[rank * f:(rank + 1) * f]])
        elif k.endswith((".down_w", ".down_s", ".down_z")):
            out[k] = k_cut(k, v, rank * f, (rank + 1) * f)
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
