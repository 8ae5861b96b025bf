"""FP8 (e4m3) expert weights: the W8A16 grouped GEMMs of ops/csrc/moe.hip against ops.reference.moe_mlp
in float64 on code * s, and the engine with experts_dtype="fp8".  Inputs are test_moe_gpu._inputs with
every (expert, row) of both weight stacks multiplied by 2 ** randint(-2, 2) before quantising: rows,
gate / up halves and experts differ severalfold in scale, so a scale from the wrong one shows."""
import pytest
import torch

from test_moe_gpu import _check, _inputs
from test_weights_fp8_gpu import PROMPTS, _run_tops, _same_or_near_tie
from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaModel, PRESETS, quantize_experts_fp8
from langstream_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
MOE = PRESETS["qwen3-moe-tiny"]


def _fp8_inputs(T, E, H, k, F, norm=True, shift=0):
    """(x, router_w, gate_up codes, down codes, gate_up_s, down_s) on the CPU."""
    x, wr, gu, dn = _inputs(T, E, H, k, F, norm=norm, shift=shift)
    g = torch.Generator().manual_seed(11 * T + shift)
    q = [quantize_experts_fp8((w.float() * 2.0 ** torch.randint(-2, 3, (*w.shape[:2], 1), generator=g)).to(torch.bfloat16))
         for w in (gu, dn)]
    return x, wr, q[0][0], q[1][0], q[0][1], q[1][1]


def _run(t, k, norm, **kw):
    x, wr, gu, dn, gs, ds = (v if v is None else v.to(DEV) for v in t)
    return ops.moe_mlp(x, wr, gu, dn, k, norm, gate_up_s=gs, down_s=ds, **kw)


@pytest.mark.parametrize("T,E,k,H,F", [(1, 8, 2, 128, 64), (5, 8, 2, 192, 64), (17, 8, 2, 128, 192),
                                       (130, 8, 2, 256, 192), (300, 4, 2, 192, 64), (40, 128, 8, 256, 64)])
def test_moe_mlp_fp8(T, E, k, H, F):
    """One K step; the half step of the 128-code form in gate_up's K (H = 192) and in down's (F = 192);
    many 32-row tiles; the 128-row tile; E = 128.  Two calls on the same buffers, out a window of a
    sentinel buffer.  The seeds (shift) are ones at which an f32 evaluation on the CPU rounds no act
    element to another bf16 than the float64 oracle (shift 3 at T = 300 does: 1.15x the bound)."""
    buf = torch.full((T + 4, H), 7.0, dtype=torch.bfloat16, device=DEV)
    for shift in (1, 5):
        t = _fp8_inputs(T, E, H, k, F, shift=shift)
        want, y = ref.moe_mlp(*t[:4], k, True, slots=True, gate_up_s=t[4], down_s=t[5])
        ops.moe_launch_counts(reset=True)
        got = _run(t, k, True, out=buf[2:T + 2])
        census = ops.moe_launch_counts(reset=True)
        bm = 128 if T * k >= 64 * E else 32
        assert census == {"route_mfma" if T >= 16 else "route_dot": 1, "align": 1, f"gate_up_w8_bm{bm}": 1,
                          f"down_w8_bm{bm}": 1, "combine": 1}, census
        _check(got, want, y, f"moe_mlp fp8 T={T} E={E} H={H} F={F} shift={shift}")
        assert bool((buf[:2] == 7.0).all()) and bool((buf[T + 2:] == 7.0).all())


@pytest.mark.parametrize("route", ["last", "each"])
@pytest.mark.parametrize("tile_rows", [32, 128])
def test_moe_mlp_fp8_given_routes(route, tile_rows):
    """All tokens to expert E - 1, and one token per expert, scrambled: the scales' expert lookup, the scatter."""
    E, H, F = 8, 128, 64
    T = 40 if route == "last" else E
    t = _fp8_inputs(T, E, H, 1, F, norm=False)
    ids = torch.full((T, 1), E - 1, dtype=torch.int32) if route == "last" else (
        (3 * torch.arange(T, dtype=torch.int32) + 1) % E)[:, None].contiguous()
    w = (0.25 + torch.arange(T, dtype=torch.float32) / 64)[:, None].contiguous()
    want, y = ref.moe_mlp(*t[:4], 1, False, route=(ids, w), slots=True, gate_up_s=t[4], down_s=t[5])
    got = _run(t, 1, False, route=(ids.to(DEV), w.to(DEV)), tile_rows=tile_rows)
    _check(got, want, y, f"fp8 given route {route} bm{tile_rows}")


def test_engine_fp8_experts_graphs_match_eager_and_python():
    """HIP graphs against the eager runner and the Python executor; 264 decode rows take the 128-row tile."""
    from langstream_amd.engine.arena import PyStepExecutor
    from langstream_amd.engine.llm_engine import NSLOTS
    model = LlamaModel(MOE, device=DEV, experts_dtype="fp8")
    assert model.weight_bytes < LlamaModel(MOE, device=DEV).weight_bytes
    kw = dict(num_blocks=512, max_model_len=512, max_batch=320)
    many = [[5 + (7 * i + j) % 500 for j in range(3 + i % 5)] for i in range(264)]
    eng = [LLMEngine(model, None, **kw)] + [LLMEngine(model, None, use_graphs=False, **kw) for _ in range(2)]
    eng[2].exec = PyStepExecutor(model, eng[2].kv_caches, eng[2].layout, NSLOTS, eng[2].nsplit, eng[2].bps, eng[2].device)
    assert eng[0].stats["experts_dtype"] == "fp8"
    outs = []
    for i, e in enumerate(eng):
        ops.moe_launch_counts(reset=True)
        outs.append([_run_tops(e, p, SamplingParams(max_tokens=n, temperature=0.0, ignore_eos=True, logprobs=2 if i else 0))
                     for p, n in ((many, 3), (PROMPTS, 12))])
        census = ops.moe_launch_counts(reset=True)
        assert census.get("down_w8_bm32") and census.get("down_w8_bm128"), census
        assert not any(key in census for key in ("gate_up_bm32", "down_bm32", "gate_up_bm128", "down_bm128")), census
    assert eng[0].stats["graph_steps"] > 0
    for other in outs[1:]:
        for run, run_o in zip(outs[0], other):
            for a, b in zip(run, run_o):
                _same_or_near_tie(a, b)


def _runner_with_one_scale_list():
    m = LlamaModel(MOE, device=DEV, experts_dtype="fp8")
    L = m.layers
    kv = [ops.new_kv_cache(2, m.hkv, 64, DEV, torch.bfloat16) for _ in L]
    ops.hip().LlamaRunner(m.embed, [l.qkv_w for l in L], [l.o_w for l in L], [], [], [l.in_norm for l in L],
                          [l.post_norm for l in L], m.final_norm, m.lm_head, [k for k, _ in kv], [v for _, v in kv],
                          m.cos_sin, m.hq, m.hkv, 64, 1e-6, m.scale, 512, 0, None, router_w=[l.router_w for l in L],
                          experts_gate_up_w=[l.experts_gate_up_w for l in L], experts_down_w=[l.experts_down_w for l in L],
                          experts_per_token=2, norm_topk=True, experts_gate_up_s=[l.experts_gate_up_s for l in L])


def _mlp_with(change):
    t = list(_fp8_inputs(5, 8, 128, 2, 64))
    change(t)
    _run(t, 2, True)


@pytest.mark.parametrize("call,match", [
    (lambda: LlamaModel(PRESETS["llama-tiny"], device=DEV, experts_dtype="fp8"), "dense model"),
    (lambda: LlamaModel(MOE, device=DEV, experts_dtype="fp8", weights_dtype="fp8"), "experts_dtype"),
    (_runner_with_one_scale_list, "experts_gate_up_s and experts_down_s are given together"),
    (lambda: _mlp_with(lambda t: t.__setitem__(4, t[4][:, :-1].contiguous())), "gate_up_s has shape"),
    (lambda: _mlp_with(lambda t: t.__setitem__(5, t[5].double())), "down_s must be float32"),
    (lambda: _mlp_with(lambda t: t.__setitem__(slice(4, 6), (None, None))), "float8_e4m3fn codes but")],
    ids=["dense", "weights-fp8", "one-list", "shape", "dtype", "no-scales"])
def test_fp8_experts_refusals(call, match):
    with pytest.raises((ValueError, RuntimeError), match=match):
        call()
