"""Llama-family decoder (Llama-3 8B / 70B and small test configs) on the HIP kernels.

This is the local replacement for the reference's remote chat/text completion
services (``ChatCompletionsStep.java:132-155`` ->
``OpenAICompletionService.java:122-311``).  Design, MI355X-first:

* weights packed for the GEMM shapes hipBLASLt likes: fused ``qkv`` [(Hq+2Hkv)*D, H],
  fused ``gate_up`` [2F, H]; bf16; sized per TP rank (column-parallel qkv/gate_up,
  row-parallel o/down, vocab-parallel embedding and LM head).
* one fused HIP kernel per elementwise stage: fused_add_rmsnorm (residual add + norm),
  rope_and_cache (RoPE + paged-KV write, V stored transposed), silu_and_mul.
* attention: MFMA paged prefill (varlen, causal, chunked-prefix) and paged decode
  (split-KV) kernels reading the engine's KV cache directly.
* TP: one process per GPU, RCCL all-reduce after o_proj and down_proj (2 per layer) and
  an all-gather of the vocab-sharded logits.  The all-reduce is on the torch.distributed
  process group so decode steps stay capturable in a HIP graph.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F

from .. import ops
from ..ops import reference as ref


@dataclass
class LlamaConfig:
    name: str = "llama"
    vocab_size: int = 128256
    hidden_size: int = 4096
    intermediate_size: int = 14336
    num_layers: int = 32
    num_heads: int = 32
    num_kv_heads: int = 8
    head_dim: int = 128
    rope_theta: float = 500000.0
    rope_scaling: Optional[dict] = None
    rms_eps: float = 1e-5
    max_position: int = 8192
    tie_embeddings: bool = False
    bos_token_id: int = 128000
    eos_token_ids: tuple = (128001, 128009)
    qkv_bias: bool = False   # a bias on the fused QKV projection (Qwen2), added before RoPE
    # a per-head RMSNorm (eps rms_eps) of every q and k head after the projection and before
    # RoPE (Qwen3): one [head_dim] weight for all q heads and one for all k heads, per layer
    qk_norm: bool = False
    # sliding-window attention (Mistral, Qwen2): a windowed layer's query at position p sees the
    # keys p - W < j <= p.  0: full attention.  window_layers: the windowed layer indices,
    # None with a window: every layer
    sliding_window: int = 0
    window_layers: Optional[tuple] = None

    def layer_window(self, i: int) -> int:
        """The attention window of layer i (0: full attention)."""
        if self.sliding_window <= 0:
            return 0
        if self.window_layers is None or i in self.window_layers:
            return int(self.sliding_window)
        return 0

    @property
    def num_params(self) -> int:
        H, Fi, V, L = self.hidden_size, self.intermediate_size, self.vocab_size, self.num_layers
        qkv = H * (self.num_heads + 2 * self.num_kv_heads) * self.head_dim
        o = self.num_heads * self.head_dim * H
        mlp = 3 * H * Fi
        if self.qkv_bias:
            qkv += (self.num_heads + 2 * self.num_kv_heads) * self.head_dim
        if self.qk_norm:
            qkv += 2 * self.head_dim
        return L * (qkv + o + mlp + 2 * H) + V * H * (1 if self.tie_embeddings else 2) + H

    def flops_per_token(self, ctx: int = 0) -> float:
        """Forward FLOPs per token (2 * matmul params + attention)."""
        H, Fi, L = self.hidden_size, self.intermediate_size, self.num_layers
        lin = 2 * L * (H * (self.num_heads + 2 * self.num_kv_heads) * self.head_dim
                       + self.num_heads * self.head_dim * H + 3 * H * Fi) + 2 * self.vocab_size * H
        attn = 4 * L * self.num_heads * self.head_dim * ctx
        return float(lin + attn)


PRESETS = {
    "llama-3-8b": LlamaConfig(name="llama-3-8b"),
    "llama-3.1-8b": LlamaConfig(name="llama-3.1-8b", max_position=131072,
                                rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                              "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}),
    "llama-3-70b": LlamaConfig(name="llama-3-70b", hidden_size=8192, intermediate_size=28672, num_layers=80,
                               num_heads=64, num_kv_heads=8),
    # small configs for tests / CPU plumbing (same code path, tiny shapes)
    "llama-tiny": LlamaConfig(name="llama-tiny", vocab_size=512, hidden_size=256, intermediate_size=512,
                              num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64, max_position=2048,
                              bos_token_id=1, eos_token_ids=(2,)),
    "llama-small": LlamaConfig(name="llama-small", vocab_size=32000, hidden_size=1024, intermediate_size=2816,
                               num_layers=4, num_heads=8, num_kv_heads=2, head_dim=128, max_position=4096,
                               bos_token_id=1, eos_token_ids=(2,)),
    # the same two shapes as Qwen2: a bias on the QKV projection, RoPE base 1e6, eps 1e-6
    "qwen2-tiny": LlamaConfig(name="qwen2-tiny", vocab_size=512, hidden_size=256, intermediate_size=512,
                              num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64, max_position=2048,
                              bos_token_id=1, eos_token_ids=(2,), qkv_bias=True, rope_theta=1e6, rms_eps=1e-6),
    "qwen2-small": LlamaConfig(name="qwen2-small", vocab_size=32000, hidden_size=1024, intermediate_size=2816,
                               num_layers=4, num_heads=8, num_kv_heads=2, head_dim=128, max_position=4096,
                               bos_token_id=1, eos_token_ids=(2,), qkv_bias=True, rope_theta=1e6, rms_eps=1e-6),
    # Qwen3: no bias, a per-head RMSNorm of q and k.  qwen3-tiny is qwen2-tiny's shape;
    # qwen3-small has the layer shape of Qwen3-0.6B, in which Hq * D = 2048 is not the hidden size
    "qwen3-tiny": LlamaConfig(name="qwen3-tiny", vocab_size=512, hidden_size=256, intermediate_size=512,
                              num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64, max_position=2048,
                              bos_token_id=1, eos_token_ids=(2,), qk_norm=True, rope_theta=1e6, rms_eps=1e-6),
    "qwen3-small": LlamaConfig(name="qwen3-small", vocab_size=32000, hidden_size=1024, intermediate_size=3072,
                               num_layers=4, num_heads=16, num_kv_heads=8, head_dim=128, max_position=4096,
                               bos_token_id=1, eos_token_ids=(2,), qk_norm=True, rope_theta=1e6, rms_eps=1e-6,
                               tie_embeddings=True),
    "qwen3-0.6b": LlamaConfig(name="qwen3-0.6b", vocab_size=151936, hidden_size=1024, intermediate_size=3072,
                              num_layers=28, num_heads=16, num_kv_heads=8, head_dim=128, max_position=40960,
                              bos_token_id=151643, eos_token_ids=(151645, 151643), qk_norm=True, rope_theta=1e6,
                              rms_eps=1e-6, tie_embeddings=True),
    "qwen3-8b": LlamaConfig(name="qwen3-8b", vocab_size=151936, hidden_size=4096, intermediate_size=12288,
                            num_layers=36, num_heads=32, num_kv_heads=8, head_dim=128, max_position=40960,
                            bos_token_id=151643, eos_token_ids=(151645, 151643), qk_norm=True, rope_theta=1e6,
                            rms_eps=1e-6),
}


@dataclass
class TPInfo:
    rank: int = 0
    world: int = 1
    group: Optional[object] = None
    force_pg: bool = False   # run the native TP path (collectives, vocab-parallel sampling) even at world 1

    def all_reduce(self, t: torch.Tensor) -> torch.Tensor:
        if self.world > 1:
            dist.all_reduce(t, group=self.group)
        return t

    def all_gather_last(self, t: torch.Tensor) -> torch.Tensor:
        if self.world == 1:
            return t
        parts = [torch.empty_like(t) for _ in range(self.world)]
        dist.all_gather(parts, t.contiguous(), group=self.group)
        return torch.cat(parts, dim=-1)


@dataclass
class AttnMeta:
    """Per-step attention metadata (device tensors).

    A step packs ``num_decode`` decode tokens (rows [0, num_decode), one per running
    sequence) followed by prefill chunks (rows [num_decode, T)); either part may be
    empty.  Decode rows use the paged decode kernel, prefill rows the paged prefill
    kernel (``q_start`` is the ABSOLUTE first row of each prefill sequence)."""
    positions: torch.Tensor                      # [T] int32
    slots: torch.Tensor                          # [T] int64
    num_decode: int = 0
    # decode part
    d_block_tables: Optional[torch.Tensor] = None  # [nd, max_blocks] int32
    d_ctx_lens: Optional[torch.Tensor] = None      # [nd] int32
    nsplit: int = 1
    blocks_per_split: int = 1 << 30
    workspace: Optional[torch.Tensor] = None
    # prefill part
    num_prefill_tokens: int = 0
    p_block_tables: Optional[torch.Tensor] = None  # [np, max_blocks] int32
    q_start: Optional[torch.Tensor] = None         # [np] int32 (absolute rows)
    q_len: Optional[torch.Tensor] = None           # [np] int32
    ctx_len: Optional[torch.Tensor] = None         # [np] int32
    tiles: Optional[torch.Tensor] = None           # [ntiles, 2] int32


_PGEMM = {"0": 0, "all": 2}.get(os.environ.get("LS_PGEMM", "1"), 1)
_PGEMM_MIN_T = int(os.environ.get("LS_PGEMM_MIN_T", "8192"))   # below: hipBLASLt + silu_and_mul is faster


def _pgemm(x: torch.Tensor, w: torch.Tensor, silu: bool) -> bool:
    """The Python forward's own rule (not runner.hip's): bf16 rows on the GPU go to the
    256x256-tile MFMA GEMM from LS_PGEMM_MIN_T rows (default 8192 here, 1024 in the
    runner).  LS_PGEMM unset, "1" or any other word: gate_up only; "all": the plain
    projections too; "0": none."""
    return (_PGEMM > (0 if silu else 1) and x.is_cuda and x.shape[0] >= _PGEMM_MIN_T and x.dtype == torch.bfloat16
            and x.stride(-1) == 1 and ops.hip().gemm_prefill_supported(w, silu))


def _linear(x: torch.Tensor, w: torch.Tensor, s: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x . w^T; with row scales ``s`` the weight is fp8 codes and the W8A16 projection runs
    (ops.linear_w8: the HIP kernels on the GPU, ops.reference.linear_w8 on the CPU)."""
    if s is not None:
        return ops.linear_w8(x, w, s)
    return ops.gemm_prefill(x, w) if _pgemm(x, w, False) else F.linear(x, w)


WEIGHTS_DTYPES = ("bf16", "fp8")
W8_NAMES = ("qkv", "o", "gate_up", "down")   # the projections an fp8 model stores as codes + row scales


def tp_kv_heads(num_kv_heads: int, world: int) -> int:
    """KV heads per TP rank.  With more ranks than KV heads every KV head is REPLICATED on
    world / num_kv_heads consecutive ranks (each rank keeps the one KV head its query
    heads attend to), so e.g. an 8-KV-head model still shards over TP=16."""
    if num_kv_heads % world == 0:
        return num_kv_heads // world
    if world % num_kv_heads == 0:
        return 1
    raise ValueError(f"TP degree {world} must divide or be a multiple of the {num_kv_heads} KV heads")


class LlamaLayer:
    def __init__(self, cfg: LlamaConfig, tp: TPInfo, device, dtype, fp8: bool = False):
        H, D = cfg.hidden_size, cfg.head_dim
        assert cfg.num_heads % tp.world == 0, "TP must divide the query heads"
        assert cfg.intermediate_size % tp.world == 0
        self.hq = cfg.num_heads // tp.world
        self.hkv = tp_kv_heads(cfg.num_kv_heads, tp.world)
        self.f = cfg.intermediate_size // tp.world
        std = 0.02
        mk = lambda *s: (torch.randn(*s, device=device, dtype=torch.float32) * std).to(dtype)  # noqa: E731
        self.qkv_w = mk((self.hq + 2 * self.hkv) * D, H)
        self.o_w = mk(H, self.hq * D) / math.sqrt(2 * cfg.num_layers)
        self.gate_up_w = mk(2 * self.f, H)
        self.down_w = mk(H, self.f) / math.sqrt(2 * cfg.num_layers)
        # fp8 weights: codes + one f32 scale per output row, quantised here, layer by layer,
        # so the model never exists in full at the wider type
        self.qkv_s = self.o_s = self.gate_up_s = self.down_s = None
        if fp8:
            for n in W8_NAMES:
                codes, sc = ref.quantize_weight_fp8(getattr(self, n + "_w"))
                setattr(self, n + "_w", codes)
                setattr(self, n + "_s", sc)
        self.in_norm = torch.ones(H, device=device, dtype=dtype)
        self.post_norm = torch.ones(H, device=device, dtype=dtype)
        # packed like the rows of qkv_w: q heads, k heads, v heads
        self.qkv_b = torch.zeros((self.hq + 2 * self.hkv) * D, device=device, dtype=dtype) if cfg.qkv_bias else None

        # one weight for all q heads and one for all k heads (replicated on every TP rank)
        self.q_norm = torch.ones(D, device=device, dtype=dtype) if cfg.qk_norm else None
        self.k_norm = torch.ones(D, device=device, dtype=dtype) if cfg.qk_norm else None

    def tensors(self):
        t = [self.qkv_w, self.o_w, self.gate_up_w, self.down_w, self.in_norm, self.post_norm]
        if self.qkv_s is not None:
            t += [self.qkv_s, self.o_s, self.gate_up_s, self.down_s]
        if self.qkv_b is not None:
            t.append(self.qkv_b)
        if self.q_norm is not None:
            t += [self.q_norm, self.k_norm]
        return t


class LlamaModel:
    """Random-init (or state-dict-loaded) Llama weights + forward over the paged KV cache."""

    def __init__(self, cfg: LlamaConfig, device="cuda", dtype=torch.bfloat16, tp: Optional[TPInfo] = None,
                 seed: int = 0, weights_dtype: str = "bf16"):
        if weights_dtype not in WEIGHTS_DTYPES:
            raise ValueError(f"weights_dtype must be one of {WEIGHTS_DTYPES}, got {weights_dtype!r}")
        # "fp8": the four projections of every layer are float8_e4m3fn codes with one f32 scale
        # per output row (W8A16: activations, embed, lm_head and the norms keep `dtype`)
        self.weights_dtype = weights_dtype
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        self.tp = tp or TPInfo()
        g = torch.random.fork_rng(devices=[self.device] if self.device.type == "cuda" else [])
        with g:
            torch.manual_seed(seed + 1000 * self.tp.rank)
            H = cfg.hidden_size
            assert cfg.vocab_size % self.tp.world == 0 or True
            self.vocab_per_rank = (cfg.vocab_size + self.tp.world - 1) // self.tp.world
            self.vocab_start = self.tp.rank * self.vocab_per_rank
            self.embed = (torch.randn(self.vocab_per_rank, H, device=self.device) * 0.02).to(dtype)
            self.layers = [LlamaLayer(cfg, self.tp, self.device, dtype, fp8=weights_dtype == "fp8")
                           for _ in range(cfg.num_layers)]
            self.final_norm = torch.ones(H, device=self.device, dtype=dtype)
            self.lm_head = self.embed if cfg.tie_embeddings else (
                torch.randn(self.vocab_per_rank, H, device=self.device) * 0.02).to(dtype)
        self.hq = cfg.num_heads // self.tp.world
        self.hkv = tp_kv_heads(cfg.num_kv_heads, self.tp.world)
        self.cos_sin = ref.rope_cos_sin(cfg.max_position, cfg.head_dim, cfg.rope_theta, cfg.rope_scaling,
                                        device=self.device)
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        # scales of an fp8 KV cache (the engine that owns the caches sets them; bf16 caches ignore them)
        self.kv_k_scale = 1.0
        self.kv_v_scale = 1.0
        if weights_dtype == "fp8" and self.device.type == "cuda":
            # a projection the W8 kernels do not take is refused here, by name, never rerouted
            for i, l in enumerate(self.layers):
                for n in W8_NAMES:
                    w = getattr(l, n + "_w")
                    if w.shape[0] % 64 or w.shape[1] % 64:
                        raise ValueError(f"layers.{i}.{n}_w {tuple(w.shape)}: fp8 weights need both dimensions "
                                         f"to be multiples of 64")

    @property
    def weight_bytes(self) -> int:
        """Bytes of this rank's weights (tied lm_head counted once)."""
        ts = [self.embed, self.final_norm] + ([] if self.lm_head is self.embed else [self.lm_head])
        for l in self.layers:
            ts += l.tensors()
        return int(sum(t.numel() * t.element_size() for t in ts))

    # ------------------------------------------------------------------ weights io
    def _layer_names(self) -> tuple:
        names = ("qkv_w", "o_w", "gate_up_w", "down_w", "in_norm", "post_norm")
        if self.cfg.qkv_bias:
            names += ("qkv_b",)
        if self.cfg.qk_norm:
            names += ("q_norm", "k_norm")
        if self.weights_dtype == "fp8":
            names += tuple(n + "_s" for n in W8_NAMES)
        return names

    def state_dict(self) -> dict:
        sd = {"embed": self.embed, "final_norm": self.final_norm, "lm_head": self.lm_head}
        for i, l in enumerate(self.layers):
            for n in self._layer_names():
                sd[f"layers.{i}.{n}"] = getattr(l, n)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Load packed weights (our layout).  HF checkpoints are converted by
        ``models.loader.convert_hf_llama``."""
        self.embed.copy_(sd["embed"])
        self.final_norm.copy_(sd["final_norm"])
        if not self.cfg.tie_embeddings:
            self.lm_head.copy_(sd["lm_head"])
        fp8 = self.weights_dtype == "fp8"
        for i, l in enumerate(self.layers):
            for n in self._layer_names():
                key = f"layers.{i}.{n}"
                if fp8 and n.endswith("_s"):
                    continue   # loaded with its weight below
                src = sd[key]
                if n.endswith("_w") and n[:-2] in W8_NAMES:
                    if not fp8 and ref.is_fp8(src):
                        raise ValueError(f"{key} holds float8_e4m3fn codes but the model's weights_dtype is "
                                         f"'bf16'; build the model with weights_dtype='fp8'")
                    if fp8:
                        skey = f"layers.{i}.{n[:-2]}_s"
                        if ref.is_fp8(src):
                            if skey not in sd:
                                raise ValueError(f"{key} holds float8_e4m3fn codes but {skey} is missing")
                            sc = sd[skey].to(torch.float32).reshape(-1)
                            if sc.numel() == 1:
                                sc = sc.expand(src.shape[0])
                            if sc.numel() != src.shape[0]:
                                raise ValueError(f"{skey} has {sc.numel()} elements for {src.shape[0]} rows")
                            codes = src
                        else:   # a wider tensor: quantise it with the one rule
                            codes, sc = ref.quantize_weight_fp8(src.to(self.device))
                        getattr(l, n).view(torch.uint8).copy_(codes.contiguous().view(torch.uint8))
                        getattr(l, n[:-2] + "_s").copy_(sc)
                        continue
                getattr(l, n).copy_(src)

    # ------------------------------------------------------------------ forward
    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        if self.tp.world == 1:
            return F.embedding(ids.long(), self.embed)
        local = ids.long() - self.vocab_start
        mask = (local < 0) | (local >= self.vocab_per_rank)
        h = F.embedding(local.clamp(0, self.vocab_per_rank - 1), self.embed)
        h = h.masked_fill(mask[:, None], 0)
        return self.tp.all_reduce(h)

    def forward(self, ids: torch.Tensor, meta: AttnMeta, kv_caches: list) -> torch.Tensor:
        """Returns hidden states [T, H] after the final norm (all rows)."""
        cfg = self.cfg
        eps = cfg.rms_eps
        h = self.embed_tokens(ids)
        residual = h
        x = ops.rmsnorm(h, self.layers[0].in_norm, eps)
        D = cfg.head_dim
        ks, vs = self.kv_k_scale, self.kv_v_scale
        for li, layer in enumerate(self.layers):
            kc, vc = kv_caches[li]
            qkv = _linear(x, layer.qkv_w, layer.qkv_s)
            ops.rope_and_cache(qkv, meta.positions, self.cos_sin, meta.slots, kc, vc, self.hq, self.hkv,
                               k_scale=ks, v_scale=vs, bias=layer.qkv_b, q_norm=layer.q_norm, k_norm=layer.k_norm,
                               norm_eps=eps)
            q = qkv[:, : self.hq * D]
            nd = meta.num_decode
            win = cfg.layer_window(li)
            if meta.num_prefill_tokens == 0:
                attn = ops.paged_decode_attention(q, kc, vc, meta.d_block_tables, meta.d_ctx_lens, self.scale,
                                                  nsplit=meta.nsplit, blocks_per_split=meta.blocks_per_split,
                                                  workspace=meta.workspace, k_scale=ks, v_scale=vs, window=win)
            else:
                attn = torch.empty(q.shape[0], self.hq * D, dtype=q.dtype, device=q.device)
                if nd:
                    ops.paged_decode_attention(q[:nd], kc, vc, meta.d_block_tables, meta.d_ctx_lens, self.scale,
                                               out=attn[:nd], nsplit=meta.nsplit,
                                               blocks_per_split=meta.blocks_per_split, workspace=meta.workspace,
                                               k_scale=ks, v_scale=vs, window=win)
                ops.paged_prefill_attention(q, kc, vc, meta.p_block_tables, meta.q_start, meta.q_len, meta.ctx_len,
                                            meta.tiles, self.hq, self.scale, out=attn, k_scale=ks, v_scale=vs,
                                            window=win)
            o = _linear(attn, layer.o_w, layer.o_s)
            self.tp.all_reduce(o)
            ops.fused_add_rmsnorm(o, residual, layer.post_norm, eps)
            if layer.gate_up_s is not None:
                a = ops.silu_and_mul(_linear(o, layer.gate_up_w, layer.gate_up_s))
            elif _pgemm(o, layer.gate_up_w, True):
                a = ops.gemm_prefill(o, layer.gate_up_w, silu=True)
            else:
                a = ops.silu_and_mul(F.linear(o, layer.gate_up_w))
            d = _linear(a, layer.down_w, layer.down_s)
            self.tp.all_reduce(d)
            nxt = self.layers[li + 1].in_norm if li + 1 < len(self.layers) else self.final_norm
            ops.fused_add_rmsnorm(d, residual, nxt, eps)
            x = d
        return x

    def _native_runner(self, kv_caches: list):
        """The C++ step executor (``ops/csrc/runner.hip``), built once per KV-cache set.
        It issues the whole forward with the GIL released: a Python-driven forward
        re-acquires the GIL after every op and stalls behind busy agent threads."""
        key = id(kv_caches)
        r = getattr(self, "_runner", None)
        if r is not None and r[0] == key:
            return r[1]
        L = self.layers
        pg = None
        if self.tp.world > 1 or self.tp.force_pg:
            pg = self.tp.group if self.tp.group is not None else dist.group.WORLD
        runner = ops.hip().LlamaRunner(
            self.embed, [l.qkv_w for l in L], [l.o_w for l in L], [l.gate_up_w for l in L],
            [l.down_w for l in L], [l.in_norm for l in L], [l.post_norm for l in L], self.final_norm,
            self.lm_head, [kv[0] for kv in kv_caches], [kv[1] for kv in kv_caches], self.cos_sin, self.hq,
            self.hkv, self.cfg.head_dim, self.cfg.rms_eps, self.scale, self.cfg.vocab_size, self.vocab_start, pg,
            self.kv_k_scale, self.kv_v_scale, [l.qkv_b for l in L] if self.cfg.qkv_bias else None,
            [self.cfg.layer_window(i) for i in range(len(L))],
            [l.q_norm for l in L] if self.cfg.qk_norm else None,
            [l.k_norm for l in L] if self.cfg.qk_norm else None,
            *([[getattr(l, n + "_s") for l in L] for n in W8_NAMES] if self.weights_dtype == "fp8" else []))
        self._runner = (key, runner, kv_caches)
        return runner

    def forward_logits(self, ids: torch.Tensor, meta: AttnMeta, kv_caches: list,
                       rows: Optional[torch.Tensor] = None, local: bool = False) -> torch.Tensor:
        """Forward + LM head for ``rows`` (all rows if None) -> f32 [N, V].  On the GPU
        the native executor runs it; elsewhere the Python path (same math).  local: see
        ``logits`` (the Python path only; the native executor samples vocab-parallel itself)."""
        if self.device.type == "cuda" and ops.hip_available():
            ws = meta.workspace
            bps = meta.blocks_per_split
            if meta.num_decode:
                bps = min(bps, meta.d_block_tables.shape[1])
                if meta.nsplit > 1:
                    need = meta.num_decode * self.hq * meta.nsplit * (self.cfg.head_dim + 2)
                    assert ws is not None and ws.numel() >= need, "decode workspace too small"
            return self._native_runner(kv_caches).forward(
                ids, meta.positions, meta.slots, meta.num_decode, meta.d_block_tables, meta.d_ctx_lens,
                meta.nsplit, bps, ws, meta.num_prefill_tokens, meta.p_block_tables, meta.q_start, meta.q_len,
                meta.ctx_len, meta.tiles, rows)
        hidden = self.forward(ids, meta, kv_caches)
        if rows is not None:
            hidden = hidden.index_select(0, rows)
        return self.logits(hidden, local=local)

    def local_vocab(self) -> int:
        """Valid vocabulary entries of this rank's LM-head slice."""
        return max(0, min(self.vocab_per_rank, self.cfg.vocab_size - self.vocab_start))

    def logits(self, hidden: torch.Tensor, local: bool = False) -> torch.Tensor:
        """[N, H] -> f32 [N, V] (vocab-parallel matmul + all-gather under TP).  local=True
        under TP: this rank's [N, local_vocab()] slice (ops.sample_vocab_parallel)."""
        if hidden.is_cuda and hidden.dtype != torch.float32:
            # f32 output from the GEMM itself (same as the native runner's LM head)
            lg = torch.mm(hidden, self.lm_head.t(), out_dtype=torch.float32)
        else:
            lg = F.linear(hidden, self.lm_head).float()
        if self.tp.world > 1:
            if local:
                return lg[:, : self.local_vocab()]
            lg = self.tp.all_gather_last(lg)
        return lg[:, : self.cfg.vocab_size]
