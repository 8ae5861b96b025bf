"""Sliding-window attention from a Hugging Face directory to the engine (no GPU needed).

Tiny random Mistral (every layer windowed) and Qwen2 (``use_sliding_window``, layer 1 windowed)
models with a window of 8 are built from config objects with the installed ``transformers``,
saved, loaded with ``llama_config_from_hf(..., sliding_window=True)`` and compared with the
library's own forward over 37 and more positions: well past the window, where the default
loader (``max_position`` clamped to the window) does not serve.  Nothing is fetched."""
from __future__ import annotations

import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import json  # noqa: E402

import pytest  # noqa: E402
import torch  # noqa: E402

from langstream_amd import ops  # noqa: E402
from langstream_amd.models.llama import AttnMeta, LlamaConfig, LlamaModel  # noqa: E402
from langstream_amd.models.loader import llama_config_from_hf, load_packed  # noqa: E402
from langstream_amd.ops import reference as ref  # noqa: E402

SHAPE = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, max_position_embeddings=2048, tie_word_embeddings=False)
IDS = [int(t) for t in torch.randint(3, 512, (37,), generator=torch.Generator().manual_seed(3))]
W = 8


def _save(kind: str, path):
    import transformers as tf
    torch.manual_seed(0)
    if kind == "mistral":
        model = tf.MistralForCausalLM(tf.MistralConfig(**SHAPE, sliding_window=W))
    else:
        model = tf.Qwen2ForCausalLM(tf.Qwen2Config(**SHAPE, sliding_window=W, use_sliding_window=True,
                                                   max_window_layers=1))
    model = model.float().eval()
    model.save_pretrained(str(path))
    return model


@pytest.fixture(scope="module")
def mistral_dir(tmp_path_factory):
    path = tmp_path_factory.mktemp("mistral_w8")
    return _save("mistral", path), path


@pytest.fixture(scope="module")
def qwen2_dir(tmp_path_factory):
    path = tmp_path_factory.mktemp("qwen2_w8")
    return _save("qwen2", path), path


def _load(path, **kw) -> LlamaModel:
    cfg = llama_config_from_hf(str(path), **kw)
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32)
    model.load_state_dict(load_packed(str(path)))
    return model


def _our_logits(model: LlamaModel, ids) -> torch.Tensor:
    T = len(ids)
    meta = AttnMeta(positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T, dtype=torch.int64),
                    num_decode=0, num_prefill_tokens=T, p_block_tables=torch.arange(4, dtype=torch.int32)[None],
                    q_start=torch.tensor([0], dtype=torch.int32), q_len=torch.tensor([T], dtype=torch.int32),
                    ctx_len=torch.tensor([T], dtype=torch.int32), tiles=ops.prefill_tiles([T], 1))
    kv = [ops.new_kv_cache(4, model.hkv, model.cfg.head_dim, "cpu", torch.float32)
          for _ in range(model.cfg.num_layers)]
    return model.forward_logits(torch.tensor(ids, dtype=torch.int32), meta, kv)


def _hf_logits(hf, ids) -> torch.Tensor:
    with torch.no_grad():
        return hf(torch.tensor([ids])).logits[0].float()


# ------------------------------------------------------------------------- logits against HF
def test_mistral_window_logits_match_transformers(mistral_dir):
    """Every layer windowed; 37 positions over a window of 8.  Bound 1e-4 (fp32 on both
    sides), that of test_hf_checkpoint_cpu.py; without the mask the error is ~1.5."""
    hf, path = mistral_dir
    model = _load(path, sliding_window=True)
    cfg = model.cfg
    assert cfg.max_position == 2048 and cfg.sliding_window == W and cfg.window_layers is None
    assert [cfg.layer_window(i) for i in range(cfg.num_layers)] == [W, W]
    err = (_our_logits(model, IDS) - _hf_logits(hf, IDS)).abs().max().item()
    print(f"mistral W={W}: max |logits - transformers| {err:.3g}")
    assert err <= 1e-4


def test_qwen2_window_is_per_layer_and_logits_match_transformers(qwen2_dir):
    """max_window_layers = 1: layer 0 full, layer 1 windowed (the saved layer_types say so)."""
    hf, path = qwen2_dir
    model = _load(path, sliding_window=True)
    cfg = model.cfg
    assert cfg.max_position == 2048 and cfg.sliding_window == W and cfg.qkv_bias
    assert [cfg.layer_window(i) for i in range(cfg.num_layers)] == [0, W]
    err = (_our_logits(model, IDS) - _hf_logits(hf, IDS)).abs().max().item()
    print(f"qwen2 W={W}, layer 1: max |logits - transformers| {err:.3g}")
    assert err <= 1e-4


def test_default_still_clamps_to_the_window(mistral_dir, qwen2_dir):
    for _, path in (mistral_dir, qwen2_dir):
        for cfg in (llama_config_from_hf(str(path)), llama_config_from_hf(str(path), sliding_window=False)):
            assert cfg.max_position == W and cfg.sliding_window == 0 and cfg.window_layers is None
            assert [cfg.layer_window(i) for i in range(cfg.num_layers)] == [0, 0]


# ---------------------------------------------------------------------------- config reading
def _write_config(path, cfg: dict) -> str:
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    return str(path)


BASE = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=4, num_attention_heads=4,
            num_key_value_heads=2, max_position_embeddings=2048, rms_norm_eps=1e-5)


def test_window_layers_from_layer_types_and_the_family_rules(tmp_path):
    m = {**BASE, "model_type": "mistral", "sliding_window": 128}
    c = llama_config_from_hf(_write_config(tmp_path / "m", m), sliding_window=True)
    assert (c.max_position, c.sliding_window, c.window_layers) == (2048, 128, None)
    # layer_types wins over the family rule
    lt = ["full_attention", "sliding_attention", "full_attention", "sliding_attention"]
    c = llama_config_from_hf(_write_config(tmp_path / "ml", {**m, "layer_types": lt}), sliding_window=True)
    assert c.window_layers == (1, 3) and [c.layer_window(i) for i in range(4)] == [0, 128, 0, 128]
    # Qwen2 without layer_types: the layers i >= max_window_layers
    q = {**BASE, "model_type": "qwen2", "sliding_window": 128, "use_sliding_window": True, "max_window_layers": 3}
    c = llama_config_from_hf(_write_config(tmp_path / "q", q), sliding_window=True)
    assert c.window_layers == (3,) and c.max_position == 2048
    # an inactive window, a window that covers every position, and a llama: nothing changes
    for name, cfg in (("q0", {**q, "use_sliding_window": False}), ("mw", {**m, "sliding_window": 4096}),
                      ("mn", {**m, "sliding_window": None}), ("l", {**m, "model_type": "llama"})):
        c = llama_config_from_hf(_write_config(tmp_path / name, cfg), sliding_window=True)
        assert (c.max_position, c.sliding_window, c.window_layers) == (2048, 0, None), name
    # no layer is windowed: a full-attention model
    c = llama_config_from_hf(_write_config(tmp_path / "qf", {**q, "layer_types": ["full_attention"] * 4}),
                             sliding_window=True)
    assert (c.max_position, c.sliding_window) == (2048, 0)


def test_unknown_layer_type_raises(tmp_path):
    cfg = {**BASE, "model_type": "qwen2", "sliding_window": 128, "use_sliding_window": True,
           "layer_types": ["full_attention", "chunked_attention", "sliding_attention", "sliding_attention"]}
    d = _write_config(tmp_path / "c", cfg)
    for kw in ({"sliding_window": True}, {}):
        with pytest.raises(ValueError, match="chunked_attention"):
            llama_config_from_hf(d, **kw)


def test_layer_window_helper_and_negative_windows():
    c = LlamaConfig(num_layers=4, sliding_window=16, window_layers=(1, 3))
    assert [c.layer_window(i) for i in range(4)] == [0, 16, 0, 16]
    assert [LlamaConfig(num_layers=2, sliding_window=16).layer_window(i) for i in range(2)] == [16, 16]
    assert [LlamaConfig(num_layers=2).layer_window(i) for i in range(2)] == [0, 0]
    q = torch.randn(3, 2, 8)
    with pytest.raises(ValueError):
        ref.attention(q, q, q, 1.0, 0, window=-1)
    kc, vc = ops.new_kv_cache(2, 2, 8, "cpu", torch.float32)
    bt, cl = torch.zeros(1, 1, dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.paged_decode_attention(q[:1].reshape(1, 16), kc, vc, bt, cl, 1.0, window=-1)
    with pytest.raises(ValueError):
        ops.paged_prefill_attention(q.reshape(3, 16), kc, vc, bt, torch.tensor([0], dtype=torch.int32), cl, cl,
                                    ops.prefill_tiles([3], 1), 2, 1.0, window=-2)
    # window >= context is no window; the reference's window is the mask p - W < j <= p
    full = ref.attention(q, q, q, 1.0, 0)
    assert torch.equal(ref.attention(q, q, q, 1.0, 0, window=3), full)
    w1 = ref.attention(q, q, q, 1.0, 0, window=1)
    assert torch.allclose(w1, q)          # each token sees itself only: softmax over one key, V = q


# ------------------------------------------------------------------------------------ engine
def test_engine_generates_transformers_tokens_past_the_window(mistral_dir):
    """Prompts of 5, 20 and 70 tokens; max_prefill_tokens = 32 cuts the 70-token prompt into
    chunks whose cached prefix (32, 64) is longer than the window, and every decode step has
    a context past it.  Each of the 12 greedy tokens is the argmax of transformers'
    teacher-forced logits over prompt + output, or within 1e-3 nats of it."""
    from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
    hf, path = mistral_dir
    model = _load(path, sliding_window=True)
    g = torch.Generator().manual_seed(11)
    prompts = [[int(t) for t in torch.randint(3, 512, (n,), generator=g)] for n in (5, 20, 70)]
    eng = LLMEngine(model, None, num_blocks=32, max_model_len=512, max_prefill_tokens=32)
    assert eng.stats["sliding_window"] == W and eng.max_model_len == 512
    reqs = eng.generate(prompts, SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True))
    assert eng.stats["prefill_steps"] + eng.stats["mixed_steps"] >= 3      # the long prompt came in chunks
    for p, r in zip(prompts, reqs):
        out = list(r.output_ids)
        assert len(out) == 12
        lp = torch.log_softmax(_hf_logits(hf, p + out)[len(p) - 1: len(p) + 11].double(), -1)
        for i, t in enumerate(out):
            gap = float(lp[i].max() - lp[i, t])
            assert gap <= 1e-3, f"prompt of {len(p)}: token {i} is {gap:.3g} nats below transformers' argmax"


def test_registry_serves_the_window(mistral_dir, monkeypatch):
    from langstream_amd.services import ServiceRegistry
    _, path = mistral_dir
    monkeypatch.delenv("LS_SLIDING_WINDOW", raising=False)
    base = {"model-path": str(path), "device": "cpu", "num-blocks": 16, "use-graphs": "false", "max-model-len": 256}

    def engine(extra):
        reg = ServiceRegistry({**base, **extra})
        try:
            eng = reg.llm_engine(None)
            return eng.stats["sliding_window"], eng.cfg.max_position, eng.max_model_len
        finally:
            reg.shutdown()

    assert engine({"sliding-window": True}) == (W, 2048, 256)
    assert engine({"sliding-window": "true"}) == (W, 2048, 256)
    assert engine({}) == (0, W, W)                      # the default: served up to the window
    monkeypatch.setenv("LS_SLIDING_WINDOW", "true")
    assert engine({}) == (W, 2048, 256)                 # unset key: the environment variable
    assert engine({"sliding-window": False}) == (0, W, W)   # the key wins over the environment


def test_config_documents_declare_the_key():
    from langstream_amd.core.config_model import docs_markdown
    row = "| `sliding-window` | boolean |"
    assert row in docs_markdown()
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "docs", "CONFIG_REFERENCE.md"), encoding="utf-8") as f:
        assert row in f.read()
