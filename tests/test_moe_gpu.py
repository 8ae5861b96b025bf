"""Mixture-of-experts kernels (ops/csrc/moe.hip) against ops.reference in float64, and the engine.

Routing inputs are EXACT: column e < E of x holds ((a e + 7 t) mod E) / (8 E) against an identity
block of the router, the other columns hold {-1, 0, 1} / (8 E) against E {-1, 0, 1}.  Every value
is a bf16, every partial sum a multiple of 1 / (8 E) that f32 holds exactly, and the E logits of
a row are distinct modulo 1 / 8: f32 and float64 select the same experts in any summation order."""
import pytest
import torch

from test_weights_fp8_gpu import PROMPTS, _run_tops, _same_or_near_tie
from langstream_amd import ops
from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaModel, PRESETS
from langstream_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _inputs(T, E, H, k, F=0, norm=True, shift=0):
    """(x, router_w[, gate_up_w, down_w]) on the CPU in bf16; asserts the premises on the reference."""
    g = torch.Generator().manual_seed(1000 * T + E + shift)
    a = 5 if E % 5 else 3
    x = torch.randint(-1, 2, (T, H), generator=g).double()
    x[:, :E] = (a * torch.arange(E)[None, :] + 7 * (torch.arange(T)[:, None] + shift)) % E
    wr = E * torch.randint(-1, 2, (E, H), generator=g).double()
    wr[:, :E] = torch.eye(E)
    x, wr = (x / (8 * E)).to(torch.bfloat16), wr.to(torch.bfloat16)
    lg = (x.double() @ wr.double().t()).sort(-1).values
    assert float((lg[:, 1:] - lg[:, :-1]).min()) >= 1.0 / (8 * E)
    assert not norm or float(ref.moe_route(x, wr, k, True)[1].min()) > 2.0 ** -7
    if not F:
        return x, wr
    # g and u of order 1 for x of order 1 / (8 E); every expert its own Gaussian weights
    gu = (torch.randn(E, 2 * F, H, generator=g) * (8 * E / H ** 0.5)).to(torch.bfloat16)
    dn = (torch.randn(E, H, F, generator=g) / F ** 0.5).to(torch.bfloat16)
    return x, wr, gu, dn


@pytest.mark.parametrize("T,E,H,k,norm", [(1, 8, 128, 2, True), (5, 8, 128, 2, True), (130, 8, 256, 2, True),
                                          (7, 128, 256, 8, True), (300, 128, 512, 8, True), (64, 64, 128, 4, True),
                                          (300, 128, 512, 8, False)])
def test_moe_route(T, E, H, k, norm):
    x, wr = _inputs(T, E, H, k, norm=norm)
    want_ids, want_w = ref.moe_route(x, wr, k, norm)
    ops.moe_launch_counts(reset=True)
    ids, w = ops.moe_route(x.to(DEV), wr.to(DEV), k, norm)
    assert ops.moe_launch_counts(reset=True) == {"route_mfma" if T >= 16 else "route_dot": 1}
    assert torch.equal(ids.cpu(), want_ids)
    rel = ((w.cpu().double() - want_w.double()).abs() / want_w.double()).max().item()
    print(f"route T={T} E={E}: max relative error of topk_w {rel:.3g}")
    assert rel <= 2.0 ** -20


def _check(got, want, y, what):
    bound = 2.0 ** -7 * y.abs().sum(1) + 1e-6
    err = (got.cpu().double() - want.double()).abs()
    print(f"{what}: max |got - ref| / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("T,E,k,H,F", [(1, 8, 2, 128, 64), (5, 8, 2, 128, 64), (17, 8, 2, 192, 128),
                                       (130, 8, 2, 256, 192), (300, 4, 2, 128, 64), (40, 128, 8, 256, 64)])
def test_moe_mlp(T, E, k, H, F):
    """Two calls with different x on the same buffers; out is a window of a sentinel buffer."""
    buf = torch.full((T + 4, H), 7.0, dtype=torch.bfloat16, device=DEV)
    for shift in (0, 3):
        x, wr, gu, dn = _inputs(T, E, H, k, F, shift=shift)
        want, y = ref.moe_mlp(x, wr, gu, dn, k, True, slots=True)
        ops.moe_launch_counts(reset=True)
        got = ops.moe_mlp(x.to(DEV), wr.to(DEV), gu.to(DEV), dn.to(DEV), k, True, out=buf[2:T + 2])
        census = ops.moe_launch_counts(reset=True)
        bm = 128 if T * k >= 64 * E else 32   # the rule beside the launcher: a mean of 64 rows per expert
        assert census == {"route_mfma" if T >= 16 else "route_dot": 1, "align": 1, f"gate_up_bm{bm}": 1,
                          f"down_bm{bm}": 1, "combine": 1}, census
        _check(got, want, y, f"moe_mlp T={T} E={E} shift={shift}")
        assert bool((buf[:2] == 7.0).all()) and bool((buf[T + 2:] == 7.0).all())


@pytest.mark.parametrize("route", ["last", "each"])
@pytest.mark.parametrize("tile_rows", [32, 128])
def test_moe_mlp_given_routes(route, tile_rows):
    """Every token to expert E - 1 alone (two short tiles of one expert), and one token per
    expert in a scrambled order: the gather, the scatter and the expert lookup without the router."""
    E, H, F = 8, 128, 64
    T = 40 if route == "last" else E
    x, wr, gu, dn = _inputs(T, E, H, 1, F, norm=False)
    ids = torch.full((T, 1), E - 1, dtype=torch.int32) if route == "last" else (
        (3 * torch.arange(T, dtype=torch.int32) + 1) % E)[:, None].contiguous()
    w = (0.25 + torch.arange(T, dtype=torch.float32) / 64)[:, None].contiguous()
    want, y = ref.moe_mlp(x, wr, gu, dn, 1, False, route=(ids, w), slots=True)
    got = ops.moe_mlp(x.to(DEV), wr.to(DEV), gu.to(DEV), dn.to(DEV), 1, False, route=(ids.to(DEV), w.to(DEV)),
                      tile_rows=tile_rows)
    _check(got, want, y, f"given route {route} bm{tile_rows}")


def test_engine_moe_graphs_match_eager_and_python():
    """qwen3-moe-tiny: HIP graphs against the eager native runner and the Python executor.  264
    decode rows take the 128-row tile (T k >= 64 E from T = 256), the five long prompts the 32-row one."""
    from langstream_amd.engine.arena import PyStepExecutor
    from langstream_amd.engine.llm_engine import NSLOTS
    model = LlamaModel(PRESETS["qwen3-moe-tiny"], device=DEV)
    kw = dict(num_blocks=512, max_model_len=512, max_batch=320)
    many = [[5 + (7 * i + j) % 500 for j in range(3 + i % 5)] for i in range(264)]
    eng = [LLMEngine(model, None, **kw)] + [LLMEngine(model, None, use_graphs=False, **kw) for _ in range(2)]
    eng[2].exec = PyStepExecutor(model, eng[2].kv_caches, eng[2].layout, NSLOTS, eng[2].nsplit, eng[2].bps, eng[2].device)
    outs = []
    for i, e in enumerate(eng):
        ops.moe_launch_counts(reset=True)
        outs.append([_run_tops(e, p, SamplingParams(max_tokens=n, temperature=0.0, ignore_eos=True, logprobs=2 if i else 0))
                     for p, n in ((many, 3), (PROMPTS, 12))])
        census = ops.moe_launch_counts(reset=True)
        assert census.get("down_bm32") and census.get("down_bm128"), census
    assert eng[0].stats["graph_steps"] > 0
    for other in outs[1:]:
        for run, run_o in zip(outs[0], other):
            for a, b in zip(run, run_o):
                _same_or_near_tie(a, b)


@pytest.mark.parametrize("kw,match", [(dict(weights_dtype="fp8"), "fp8 or int4"), (dict(weights_dtype="int4"), "fp8 or int4")])
def test_engine_moe_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        LlamaModel(PRESETS["qwen3-moe-tiny"], device=DEV, **kw)
    model = LlamaModel(PRESETS["qwen3-moe-tiny"], device=DEV)
    L = model.layers
    args = [model.embed, [l.qkv_w for l in L], [l.o_w for l in L], [], [], [l.in_norm for l in L], [l.post_norm for l in L],
            model.final_norm, model.lm_head, [], [], model.cos_sin, model.hq, model.hkv, 64, 1e-6, model.scale, 512, 0]
    moe = dict(router_w=[l.router_w for l in L], experts_gate_up_w=[l.experts_gate_up_w for l in L],
               experts_down_w=[l.experts_down_w for l in L], experts_per_token=2, norm_topk=True)
    kv = [ops.new_kv_cache(2, model.hkv, 64, DEV, torch.bfloat16) for _ in L]
    args[9], args[10] = [k for k, _ in kv], [v for _, v in kv]
    with pytest.raises(RuntimeError, match="tensor parallelism"):
        ops.hip().LlamaRunner(*args, object(), **moe)
    with pytest.raises(RuntimeError, match="together"):
        ops.hip().LlamaRunner(*args, None, **dict(moe, experts_down_w=None))
    with pytest.raises(RuntimeError, match="shape rule"):
        ops.hip().LlamaRunner(*args, None, **dict(moe, experts_per_token=9))
