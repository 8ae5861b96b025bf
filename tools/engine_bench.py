"""Microbenchmarks of the GPU engines (not the driver's bench.py): Llama decode/prefill
throughput, BERT embedding throughput, kNN latency.  Prints one JSON line per test."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams  # noqa: E402
from langstream_amd.models.llama import LlamaModel, PRESETS  # noqa: E402


def sync():
    torch.cuda.synchronize()


def bench_llm(args):
    cfg = PRESETS[args.model]
    if args.qkv_bias:   # the same shape with a bias on the QKV projection (Qwen2)
        import dataclasses
        cfg = dataclasses.replace(cfg, name=cfg.name + "+qkv-bias", qkv_bias=True)
    t0 = time.time()
    model = LlamaModel(cfg, device="cuda", weights_dtype=args.weights_dtype)
    for layer in model.layers if args.qkv_bias else ():
        layer.qkv_b.normal_(0.0, 0.5)
    sync()
    print(json.dumps({"event": "model_init", "s": round(time.time() - t0, 2)}), flush=True)
    eng = LLMEngine(model, None, max_model_len=args.max_len, max_batch=args.batch, max_prefill_tokens=args.prefill_chunk,
                    kv_cache_dtype=args.kv_dtype)
    t0 = time.time()
    eng.capture_graphs([b for b in eng.buckets if b <= args.batch])
    sync()
    print(json.dumps({"event": "graphs", "s": round(time.time() - t0, 2), "blocks": eng.num_blocks,
                      "kv_cache_dtype": eng.kv_cache_dtype, "kv_bytes_per_block": eng.kv_bytes_per_block,
                      "weights_dtype": eng.stats["weights_dtype"], "weight_bytes": eng.stats["weight_bytes"]}), flush=True)
    sp = SamplingParams(max_tokens=args.gen, temperature=0.8, top_p=0.95, ignore_eos=True)
    prompts = [[(i * 31 + j) % 1000 + 100 for j in range(args.prompt)] for i in range(args.batch)]
    # warmup
    eng.generate(prompts[:4], SamplingParams(max_tokens=4, ignore_eos=True))
    sync()
    t0 = time.time()
    reqs = [eng.submit(p, sp) for p in prompts]
    eng._drain_inbox()
    # prefill phase
    while eng.waiting:
        eng.step()
    sync()
    t1 = time.time()
    while eng.running:
        eng.step()
    sync()
    t2 = time.time()
    ntok = sum(len(r.output_ids) for r in reqs)
    print(json.dumps({
        "test": "llm", "model": cfg.name, "batch": args.batch, "prompt": args.prompt, "gen": args.gen,
        "prefill_s": round(t1 - t0, 4), "prefill_tok_s": round(args.batch * args.prompt / (t1 - t0), 1),
        "decode_s": round(t2 - t1, 4), "decode_tok_s": round((ntok - args.batch) / (t2 - t1), 1),
        "ms_per_decode_step": round(1000 * (t2 - t1) / max(1, args.gen - 1), 3),
        "stats": eng.stats}), flush=True)


def bench_embed(args):
    from langstream_amd.engine.embedder import EmbeddingEngine
    from langstream_amd.models.bert import BertEncoder, PRESETS as BP
    from langstream_amd.tokenizers import WordPieceTokenizer, builtin_corpus
    enc = BertEncoder(BP["bge-small-en"], device="cuda")
    tok = WordPieceTokenizer.synthetic()
    eng = EmbeddingEngine(enc, tok)
    corpus = builtin_corpus()
    texts = [" ".join(corpus[i: i + 6]) for i in range(args.texts)]
    eng.embed(texts[:64])
    sync()
    t0 = time.time()
    for _ in range(args.iters):
        eng.embed(texts)
    sync()
    dt = (time.time() - t0) / args.iters
    ntok = sum(len(t) for t in tok.encode_batch(texts))
    # device-resident output (what the vector store consumes): no host list conversion
    eng.embed_tensor(texts[:64])
    sync()
    t0 = time.time()
    for _ in range(args.iters):
        for i in range(0, len(texts), 512):
            eng.embed_tensor(texts[i: i + 512])
    sync()
    dt_t = (time.time() - t0) / args.iters
    # encoder forward only (pre-tokenised, packed on the device)
    toks = tok.encode_batch(texts[:512])
    packed = [t.cuda() for t in enc.pack(toks)]
    enc.forward_packed(*packed)
    sync()
    t0 = time.time()
    for _ in range(args.iters * 4):
        enc.forward_packed(*packed)
    sync()
    dt_f = (time.time() - t0) / (args.iters * 4)
    print(json.dumps({"test": "embed", "fused": enc.fused_supported(), "texts": len(texts),
                      "avg_tokens": ntok / len(texts), "texts_per_s": round(len(texts) / dt, 1),
                      "tokens_per_s": round(ntok / dt, 1), "texts_per_s_device_out": round(len(texts) / dt_t, 1),
                      "encoder_forward_512_texts_ms": round(dt_f * 1000, 3),
                      "encoder_texts_per_s": round(512 / dt_f, 1)}), flush=True)


def _time_ms(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    sync()
    t0 = time.time()
    for _ in range(iters):
        fn()
    sync()
    return (time.time() - t0) / iters * 1000


def bench_knn(args):
    import numpy as np

    from langstream_amd import ops
    from langstream_amd.engine.vector_store import pack_mask
    X = torch.nn.functional.normalize(torch.randn(args.rows, 384, device="cuda"), dim=-1)
    if args.knn_metric != "cosine":   # rows of different lengths: unit vectors x [0.5, 2]
        X = X * (0.5 + 1.5 * torch.rand(args.rows, 1, device="cuda"))
    X = X.bfloat16()
    fracs = [float(f) for f in str(args.knn_filter_frac).split(",") if f]
    for nq in str(args.queries).split(","):
        Q = torch.nn.functional.normalize(torch.randn(int(nq), 384, device="cuda"), dim=-1)
        if args.knn_metric != "cosine":
            Q = Q * (0.5 + 1.5 * torch.rand(int(nq), 1, device="cuda"))
        Q = Q.bfloat16()
        if args.knn_metric == "euclidean":
            # the biased kernels (score = dot - |x|^2 / 2) next to the unbiased ones on the same
            # X and Q, interleaved in this process: medians over the rounds, and the spread of
            # the unbiased rounds to judge the ratio against.  A zero bias runs the biased
            # kernels on the unbiased scores: the same candidates, so the kernels' own cost
            # (the Euclidean scores pass the thresholds at another rate than the dot products)
            bias = X.float().pow(2).sum(-1).mul(-0.5).contiguous()
            zero = torch.zeros_like(bias)
            tu, tb, tz = [], [], []
            for _ in range(max(3, args.knn_rounds)):
                tu.append(_time_ms(lambda: ops.knn_topk(X, Q, 20)))
                tb.append(_time_ms(lambda: ops.knn_topk(X, Q, 20, bias=bias)))
                tz.append(_time_ms(lambda: ops.knn_topk(X, Q, 20, bias=zero)))
            mu, mb, mz = float(np.median(tu)), float(np.median(tb)), float(np.median(tz))
            print(json.dumps({"test": "knn_metric", "metric": "euclidean", "rows": args.rows, "queries": int(nq),
                              "unbiased_ms": round(mu, 4), "biased_ms": round(mb, 4),
                              "biased_over_unbiased": round(mb / mu, 4), "zero_bias_ms": round(mz, 4),
                              "zero_bias_over_unbiased": round(mz / mu, 4),
                              "unbiased_rounds_ms": [round(t, 4) for t in tu],
                              "biased_rounds_ms": [round(t, 4) for t in tb],
                              "unbiased_spread": round((max(tu) - min(tu)) / mu, 4)}), flush=True)
            continue
        ms = _time_ms(lambda: ops.knn_topk(X, Q, 20, _ablate=args.knn_ablate))
        print(json.dumps({"test": "knn", "rows": args.rows, "queries": int(nq), "ms": round(ms, 3),
                          "GB_per_s": round(args.rows * 384 * 2 / ms / 1e6, 1)}), flush=True)
        # --knn-filter-frac: the same queries restricted to a random subset of the rows (one
        # mask for the batch), through the masked kernels and through the compact route
        # (gather the admitted rows, search them unfiltered), next to the unfiltered time
        for frac in fracs:
            adm = np.random.default_rng(int(frac * 1e6)).random(args.rows) < frac
            mask = torch.from_numpy(pack_mask(adm)[None]).cuda()
            rows = torch.from_numpy(np.flatnonzero(adm)).cuda()
            qmask = torch.zeros(int(nq), dtype=torch.int32)
            ms_m = _time_ms(lambda: ops.knn_topk(X, Q, 20, mask=mask, qmask=qmask))
            ms_c = _time_ms(lambda: ops.knn_topk(X.index_select(0, rows), Q, 20))
            print(json.dumps({"test": "knn_filtered", "rows": args.rows, "queries": int(nq), "frac": frac,
                              "admitted": int(rows.numel()), "masked_ms": round(ms_m, 3),
                              "compact_ms": round(ms_c, 3), "unfiltered_ms": round(ms, 3),
                              "masked_over_unfiltered": round(ms_m / ms, 3)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="llm,embed,knn")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--gen", type=int, default=128)
    ap.add_argument("--max-len", type=int, default=4096)
    ap.add_argument("--prefill-chunk", type=int, default=16384)
    ap.add_argument("--kv-dtype", choices=("auto", "bf16", "fp8"), default="auto",
                    help="KV cache element type of the LLM engine (LLMEngine kv_cache_dtype)")
    ap.add_argument("--weights-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="LLM: element type of the layer projections (LlamaModel weights_dtype; fp8: W8A16 kernels)")
    ap.add_argument("--qkv-bias", action="store_true",
                    help="LLM: the model's shape with a random bias on the QKV projection (LlamaConfig.qkv_bias)")
    ap.add_argument("--texts", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", default="64", help="comma-separated query counts (knn)")
    ap.add_argument("--knn-ablate", type=int, default=0,
                    help="kNN main-pass timing ablation 1-3 (diagnosis only: WRONG results)")
    ap.add_argument("--knn-metric", choices=("cosine", "dot-product", "euclidean"), default="cosine",
                    help="kNN data and scoring: cosine (unit rows), dot-product (rows of different lengths, the same "
                         "kernels), euclidean (the per-row bias: biased and unbiased times and their ratio)")
    ap.add_argument("--knn-rounds", type=int, default=3, help="interleaved rounds of --knn-metric euclidean (>= 3)")
    ap.add_argument("--knn-filter-frac", default="",
                    help="comma-separated admitted fractions: also time the filtered search (masked kernels and "
                         "compact route) next to the unfiltered one, e.g. 0.5,0.1")
    a = ap.parse_args()
    for w in a.what.split(","):
        {"llm": bench_llm, "embed": bench_embed, "knn": bench_knn}[w](a)
