"""Serving a Hugging Face directory (config.json, *.safetensors, tokenizer.json): tiny
random Qwen2 / Llama / Mistral models are built from a config object with the installed
``transformers``, saved, read back through ``models.loader`` and compared with the library's
own forward.  Nothing is fetched."""
from __future__ import annotations

import os

os.environ["HF_HUB_OFFLINE"] = "1"
os.environ["TRANSFORMERS_OFFLINE"] = "1"

import dataclasses  # noqa: E402
import json  # noqa: E402
import shutil  # noqa: E402
import socket  # noqa: E402

import pytest  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from langstream_amd import ops  # noqa: E402
from langstream_amd.models.llama import AttnMeta, LlamaModel, PRESETS, TPInfo  # noqa: E402
from langstream_amd.models.loader import (convert_hf_llama, llama_config_from_hf, load_packed,  # noqa: E402
                                          shard_llama)

SHAPE = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, max_position_embeddings=2048, tie_word_embeddings=False)
IDS = [int(t) for t in torch.randint(3, 512, (37,), generator=torch.Generator().manual_seed(3))]
LLAMA3_ROPE = {"rope_type": "llama3", "rope_theta": 500000.0, "factor": 8.0, "low_freq_factor": 1.0,
               "high_freq_factor": 4.0, "original_max_position_embeddings": 16}


def _save(kind: str, path) -> "torch.nn.Module":
    """A tiny random fp32 model of one family, every *_proj.bias drawn from N(0, 0.5) (the
    library initialises them to zero, which would hide a dropped bias), saved to ``path``."""
    import transformers as tf
    torch.manual_seed(0)
    if kind == "qwen2":
        cfg = tf.Qwen2Config(**SHAPE, rope_parameters={"rope_theta": 1e6, "rope_type": "default"})
        model = tf.Qwen2ForCausalLM(cfg)
    elif kind == "llama":
        cfg = tf.LlamaConfig(**SHAPE, rope_parameters=dict(LLAMA3_ROPE))
        model = tf.LlamaForCausalLM(cfg)
    else:
        cfg = tf.MistralConfig(**SHAPE, sliding_window=64)
        model = tf.MistralForCausalLM(cfg)
    model = model.float().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("_proj.bias"):
                p.normal_(0.0, 0.5)
    model.save_pretrained(str(path))
    return model


def _prefill_meta(T: int, nb: int) -> AttnMeta:
    return AttnMeta(positions=torch.arange(T, dtype=torch.int32), slots=torch.arange(T, dtype=torch.int64),
                    num_decode=0, num_prefill_tokens=T, p_block_tables=torch.arange(nb, dtype=torch.int32)[None],
                    q_start=torch.tensor([0], dtype=torch.int32), q_len=torch.tensor([T], dtype=torch.int32),
                    ctx_len=torch.tensor([T], dtype=torch.int32), tiles=ops.prefill_tiles([T], 1))


def _load(path) -> LlamaModel:
    cfg = llama_config_from_hf(str(path))
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32)
    model.load_state_dict(load_packed(str(path)))
    return model


def _our_logits(model: LlamaModel, ids) -> torch.Tensor:
    """One prefill of ``ids`` through the paged cache -> logits [T, V]."""
    kv = [ops.new_kv_cache(4, model.hkv, model.cfg.head_dim, "cpu", torch.float32)
          for _ in range(model.cfg.num_layers)]
    return model.forward_logits(torch.tensor(ids, dtype=torch.int32), _prefill_meta(len(ids), 4), kv)


def _hf_logits(hf, ids) -> torch.Tensor:
    with torch.no_grad():
        return hf(torch.tensor([ids])).logits[0].float()


@pytest.fixture(scope="module")
def qwen2_dir(tmp_path_factory):
    path = tmp_path_factory.mktemp("qwen2")
    return _save("qwen2", path), path


# ------------------------------------------------------------------------- logits against HF
def test_qwen2_logits_match_transformers(qwen2_dir):
    """The QKV biases and the RoPE base of ``rope_parameters``: 37-token prefill, bound 1e-4
    (fp32 on both sides; measured 7e-7 with the bias added before RoPE, 1.53 without it)."""
    hf, path = qwen2_dir
    model = _load(path)
    assert model.cfg.qkv_bias and model.cfg.rope_theta == 1e6 and model.cfg.rms_eps == 1e-6
    assert float(model.layers[0].qkv_b.abs().max()) > 0.5
    err = (_our_logits(model, IDS) - _hf_logits(hf, IDS)).abs().max().item()
    print(f"qwen2: max |logits - transformers| {err:.3g}")
    assert err <= 1e-4


def test_llama3_rope_parameters_logits_match_transformers(tmp_path):
    """A Llama saved by transformers 5: base and llama3 scaling inside ``rope_parameters``."""
    hf = _save("llama", tmp_path)
    model = _load(tmp_path)
    assert not model.cfg.qkv_bias and model.cfg.rope_theta == 500000.0
    assert model.cfg.rope_scaling["rope_type"] == "llama3" and model.cfg.rope_scaling["factor"] == 8.0
    err = (_our_logits(model, IDS) - _hf_logits(hf, IDS)).abs().max().item()
    print(f"llama3 rope: max |logits - transformers| {err:.3g}")
    assert err <= 1e-4


def test_mistral_sliding_window_logits_match_transformers(tmp_path):
    """An active sliding window caps max_position at the window; up to there full attention
    is windowed attention."""
    hf = _save("mistral", tmp_path)
    model = _load(tmp_path)
    assert model.cfg.max_position == 64
    err = (_our_logits(model, IDS) - _hf_logits(hf, IDS)).abs().max().item()
    print(f"mistral: max |logits - transformers| {err:.3g}")
    assert err <= 1e-4


# ---------------------------------------------------------------------------- config reading
def _write_config(path, cfg: dict) -> str:
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    return str(path)


def test_rope_top_level_keys_and_rope_parameters_agree(tmp_path):
    base = dict(model_type="llama", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=2048, rms_norm_eps=1e-5)
    scaling = {k: v for k, v in LLAMA3_ROPE.items() if k != "rope_theta"}
    old = llama_config_from_hf(_write_config(tmp_path / "old", {**base, "rope_theta": 500000.0,
                                                                 "rope_scaling": scaling}))
    new = llama_config_from_hf(_write_config(tmp_path / "new", {**base, "rope_parameters": dict(LLAMA3_ROPE)}))
    assert old == new and old.rope_theta == 500000.0 and old.rope_scaling["original_max_position_embeddings"] == 16
    plain_old = llama_config_from_hf(_write_config(tmp_path / "po", {**base, "rope_theta": 1e6}))
    plain_new = llama_config_from_hf(_write_config(tmp_path / "pn", {**base, "rope_parameters": {
        "rope_theta": 1e6, "rope_type": "default"}}))
    assert plain_old == plain_new and plain_old.rope_theta == 1e6 and plain_old.rope_scaling is None
    # generation_config.json: its eos ids are merged in
    d = _write_config(tmp_path / "gen", {**base, "eos_token_id": 2})
    with open(os.path.join(d, "generation_config.json"), "w") as f:
        json.dump({"eos_token_id": [2, 7, 9]}, f)
    assert llama_config_from_hf(d).eos_token_ids == (2, 7, 9)
    # Qwen2's window counts only with use_sliding_window
    q = {**base, "model_type": "qwen2", "sliding_window": 128}
    assert llama_config_from_hf(_write_config(tmp_path / "q0", q)).max_position == 2048
    qc = llama_config_from_hf(_write_config(tmp_path / "q1", {**q, "use_sliding_window": True}))
    assert qc.max_position == 128 and qc.qkv_bias


def test_unsupported_model_type_and_rope_type_raise(tmp_path):
    base = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4)
    with pytest.raises(ValueError, match="gemma"):
        llama_config_from_hf(_write_config(tmp_path / "g", {**base, "model_type": "gemma"}))
    with pytest.raises(ValueError, match="yarn"):
        llama_config_from_hf(_write_config(tmp_path / "y", {**base, "model_type": "qwen2", "rope_parameters": {
            "rope_theta": 1e6, "rope_type": "yarn", "factor": 4.0}}))
    with pytest.raises(ValueError, match="linear"):
        llama_config_from_hf(_write_config(tmp_path / "l", {**base, "model_type": "llama", "rope_theta": 1e4,
                                                            "rope_scaling": {"type": "linear", "factor": 2.0}}))


def test_unconsumed_checkpoint_tensor_raises(qwen2_dir, tmp_path):
    from safetensors.torch import load_file, save_file
    _, path = qwen2_dir
    sd = load_file(os.path.join(str(path), "model.safetensors"))
    assert "model.layers.0.self_attn.q_proj.bias" in sd
    convert_hf_llama(dict(sd))   # whole: accepted
    convert_hf_llama({**sd, "model.layers.0.self_attn.rotary_emb.inv_freq": torch.zeros(32)})   # the one skipped name
    sd["model.layers.0.self_attn.o_proj.bias"] = torch.zeros(256)
    shutil.copy(os.path.join(str(path), "config.json"), tmp_path / "config.json")
    save_file(sd, str(tmp_path / "model.safetensors"))
    with pytest.raises(ValueError, match=r"model\.layers\.0\.self_attn\.o_proj\.bias"):
        load_packed(str(tmp_path))


# ------------------------------------------------------------------------------- TP sharding
def _biased_tiny(seed: int = 5) -> LlamaModel:
    model = LlamaModel(PRESETS["qwen2-tiny"], device="cpu", dtype=torch.float32, seed=seed)
    g = torch.Generator().manual_seed(seed)
    for layer in model.layers:
        layer.qkv_b.copy_(torch.randn(layer.qkv_b.numel(), generator=g) * 0.5)
    return model


@pytest.mark.parametrize("world", [2, 4])   # 4 ranks on 2 KV heads: every KV head on two ranks
def test_shard_llama_slices_the_bias_like_its_rows(world):
    cfg = PRESETS["qwen2-tiny"]
    full = _biased_tiny()
    sd = full.state_dict()
    assert "layers.0.qkv_b" in sd and cfg.num_params == sum(
        v.numel() for k, v in sd.items()) - (0 if not cfg.tie_embeddings else sd["lm_head"].numel())
    D, Hq, Hkv = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
    x = torch.randn(3, cfg.hidden_size, generator=torch.Generator().manual_seed(1))
    y = (x @ sd["layers.1.qkv_w"].T + sd["layers.1.qkv_b"]).view(3, Hq + 2 * Hkv, D)
    q, k, v = y[:, :Hq], y[:, Hq: Hq + Hkv], y[:, Hq + Hkv:]
    hq = Hq // world
    for rank in range(world):
        part = shard_llama(sd, cfg, rank, world)
        got = x @ part["layers.1.qkv_w"].T + part["layers.1.qkv_b"]
        # the KV heads of the rank's query heads (GQA: query head j reads KV head j // (Hq / Hkv))
        kvh = sorted({j // (Hq // Hkv) for j in range(rank * hq, (rank + 1) * hq)})
        exp = torch.cat([q[:, rank * hq:(rank + 1) * hq], k[:, kvh], v[:, kvh]], 1).reshape(3, -1)
        assert got.shape == exp.shape and torch.allclose(got, exp, atol=1e-6), rank
        shard = LlamaModel(cfg, device="cpu", dtype=torch.float32, tp=TPInfo(rank, world, None))
        shard.load_state_dict(part)   # shapes fit the TP model


PROMPTS = [list(range(3, 3 + n)) for n in (5, 64, 97)]


def _port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
        cfg = PRESETS["qwen2-tiny"]
        m = LlamaModel(cfg, device="cpu", dtype=torch.float32, tp=TPInfo(rank, world, None))
        m.load_state_dict(shard_llama(_biased_tiny().state_dict(), cfg, rank, world))
        eng = LLMEngine(m, None, num_blocks=64, max_model_len=512)
        if rank == 0:
            out = [r.output_ids for r in eng.generate(PROMPTS, SamplingParams(max_tokens=6, temperature=0.0,
                                                                             ignore_eos=True))]
            eng.stop()
            q.put(out)
        else:
            eng.worker_loop()
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_biased_model_matches_single():
    """gloo, 2 ranks (the harness of tests/test_distributed_cpu.py): greedy tokens of the
    sharded qwen2-tiny equal TP = 1, and the bias matters for them."""
    from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
    sp = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    single = [r.output_ids for r in LLMEngine(_biased_tiny(), None, num_blocks=64, max_model_len=512).generate(
        PROMPTS, sp)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        out = q.get(timeout=240)
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert out == single
    plain = LlamaModel(PRESETS["qwen2-tiny"], device="cpu", dtype=torch.float32, seed=5)
    assert [r.output_ids for r in LLMEngine(plain, None, num_blocks=64, max_model_len=512).generate(
        PROMPTS, sp)] != single


# --------------------------------------------------------------------------------- tokeniser
_HEAD = r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|"
_TAIL = r"| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"
QWEN2_SPLIT = _HEAD + r"\p{N}" + _TAIL
LLAMA3_SPLIT = _HEAD + r"\p{N}{1,3}" + _TAIL
TEXTS = [
    "7", "42", "123", "1234", "12345", "123456", "1234567",
    "In 2024 the 3 agents read 1234567 records, 98765 of them twice.",
    "it's fine, we'll see; I'VE said they're done and don't care",
    "first line\nsecond line\n\nthird  line after a blank one\n",
    "café naïve über straße 中文 日本語 42 привет",
    "port 9042, offset 100200300 (partition 7); total: 12.5% of 80000",
]


def _train_tokenizer(path, split: str, vocab_size: int = 512) -> "object":
    """A small byte-level BPE trained with the ``tokenizers`` library on the built-in corpus."""
    from tokenizers import Regex, Tokenizer, decoders, models, pre_tokenizers, trainers
    from langstream_amd.tokenizers import builtin_corpus
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.Sequence([
        pre_tokenizers.Split(Regex(split), behavior="isolated", invert=False),
        pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["<|endoftext|>", "<|im_start|>", "<|im_end|>"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(builtin_corpus(), trainer)
    tok.save(str(path))
    return tok


@pytest.mark.parametrize("split,digits", [(QWEN2_SPLIT, 1), (LLAMA3_SPLIT, 3)], ids=["qwen2", "llama3"])
def test_from_hf_json_matches_the_tokenizers_library(tmp_path, split, digits):
    """Token ids equal the library's with Qwen2's pattern (digits one at a time) and with
    Llama-3's (digits in threes).  The pre-tokeniser is the documented approximation of the
    cl100k rule (native/tokenizer.cpp): every non-ASCII character counts as a letter, and
    a contraction is only split off before a non-letter.  TEXTS stay inside what it covers:
    their non-ASCII characters are letters (no non-ASCII digits, punctuation or spaces) and
    their contractions end a word."""
    from langstream_amd.tokenizers import BPETokenizer
    lib = _train_tokenizer(tmp_path / "tokenizer.json", split, 1500)   # room for merges of digits
    ours = BPETokenizer.from_hf_json(str(tmp_path / "tokenizer.json"))
    assert ours.max_digits == digits
    for t in TEXTS:
        exp = lib.encode(t, add_special_tokens=False).ids
        assert ours.encode(t) == exp, t
        assert ours.decode(exp) == t
    # the rule is what separates the two: a 7-digit run is 7 pieces or 3, and with pieces
    # of three the vocabulary has tokens of several digits
    pieces = [p for p, _ in lib.pre_tokenizer.pre_tokenize_str("1234567")]
    assert pieces == (list("1234567") if digits == 1 else ["123", "456", "7"])
    longest = max(len(lib.decode([i])) for t in TEXTS[:8] for i in lib.encode(t, add_special_tokens=False).ids
                  if lib.decode([i]).isdigit())
    assert (longest == 1) == (digits == 1)
    assert BPETokenizer.synthetic(512).max_digits == 3


# ----------------------------------------------------------------------------- chat template
def test_chatml_chat_prompt_exact():
    from langstream_amd.agents.genai.services import ChatMessage, chatml_chat_prompt, llama3_chat_prompt
    msgs = [ChatMessage("system", "You are terse."), ChatMessage("user", "What is 2+2?")]
    assert chatml_chat_prompt(msgs) == ("<|im_start|>system\nYou are terse.<|im_end|>\n"
                                        "<|im_start|>user\nWhat is 2+2?<|im_end|>\n"
                                        "<|im_start|>assistant\n")
    assert llama3_chat_prompt(msgs).startswith("<|begin_of_text|><|start_header_id|>system<|end_header_id|>")


def _hf_greedy(hf, ids, n):
    """Greedy decode by recomputing the whole sequence every token."""
    ids, out = list(ids), []
    for _ in range(n):
        t = int(_hf_logits(hf, ids)[-1].argmax())
        out.append(t)
        ids.append(t)
    return out


def test_registry_serves_a_model_path(qwen2_dir):
    """local-gpu-configuration {model-path}: the shape, weights and tokenizer.json of the
    directory, ChatML for qwen2, and a greedy 8-token chat completion equal to the
    Hugging Face model's own greedy tokens for the same prompt ids."""
    from langstream_amd.agents.genai.services import ChatMessage, chatml_chat_prompt
    from langstream_amd.services import ServiceRegistry
    hf, path = qwen2_dir
    lib = _train_tokenizer(path / "tokenizer.json", QWEN2_SPLIT)
    reg = ServiceRegistry({"model-path": str(path), "device": "cpu", "num-blocks": 16, "use-graphs": "false",
                           "max-model-len": 256})
    try:
        svc = reg.completions_service({"local": {}}, "qwen2.5-7b-instruct")
        eng = svc.engine
        assert eng.chat_template == "chatml"
        cfg = eng.model.cfg
        assert (cfg.hidden_size, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.num_layers, cfg.vocab_size,
                cfg.qkv_bias, cfg.rope_theta) == (256, 4, 2, 64, 2, 512, True, 1e6)
        assert eng.tok.max_digits == 1 and eng.tok.token_to_id("<|im_start|>") == lib.token_to_id("<|im_start|>")
        msgs = [ChatMessage("system", "You are terse."), ChatMessage("user", "What is 12+30?")]
        ids = eng.tok.encode(chatml_chat_prompt(msgs))
        assert ids == lib.encode(chatml_chat_prompt(msgs), add_special_tokens=False).ids
        exp = _hf_greedy(hf, ids, 8)
        res = svc.get_chat_completions(msgs, None, {"max-tokens": 8, "temperature": 0, "ignore-eos": True}).result(120)
        assert res.completion_tokens == 8 and res.prompt_tokens == len(ids)
        assert res.content == eng.tok.decode(exp)
        # an explicit chat-template wins over the family's default
        reg2 = ServiceRegistry({"model-path": str(path), "device": "cpu", "num-blocks": 16, "use-graphs": "false",
                                "chat-template": "llama3", "max-model-len": 256})
        try:
            assert reg2.completions_service({"local": {}}, None).engine.chat_template == "llama3"
        finally:
            reg2.shutdown()
    finally:
        reg.shutdown()


def test_config_model_declares_the_new_keys():
    from langstream_amd.core.config_model import docs_markdown
    md = docs_markdown()
    assert "| `model-path` | string |" in md and "| `chat-template` | string |" in md
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "docs", "CONFIG_REFERENCE.md"), encoding="utf-8") as f:
        ref_md = f.read()
    assert "| `model-path` | string |" in ref_md and "| `chat-template` | string |" in ref_md
    assert dataclasses.is_dataclass(PRESETS["qwen2-small"]) and PRESETS["qwen2-small"].qkv_bias
