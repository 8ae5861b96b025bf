"""FP8 activations without a GPU: the reference quantiser, the option's way from the service
configuration to the model, and that the CPU model with it differs from the W8A16 one."""
import pytest
import torch

from langstream_amd.engine.llm_engine import LLMEngine, SamplingParams
from langstream_amd.models.llama import LlamaModel, PRESETS
from langstream_amd.ops import reference as ref


def test_reference_quantiser_round_trips_within_half_an_ulp():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(9, 2816, generator=g) * torch.logspace(-3, 3, 9)[:, None]
    x[4] = 0.0
    x[5, 7] = 1.0e5          # the rest of the row lands on subnormal codes or zero
    xq, xs = ref.quantize_rows_fp8(x.to(torch.bfloat16))
    xf = x.to(torch.bfloat16).double()
    assert xs[4] == 1.0 and bool((xq[4].float() == 0).all())
    assert torch.equal(xs, torch.where(xf.abs().amax(1) > 0, xf.abs().amax(1).float() / 448.0, torch.ones(9)))
    err = (xf - xq.double() * xs.double()[:, None]).abs()
    assert bool((err <= 2.0 ** -4 * xf.abs() + 2.0 ** -10 * xs.double()[:, None]).all())
    assert float(xq.float().abs().max()) == 448.0


def test_activations_dtype_is_validated():
    with pytest.raises(ValueError, match="needs weights_dtype='fp8'"):
        LlamaModel(PRESETS["llama-tiny"], device="cpu", dtype=torch.float32, activations_dtype="fp8")
    with pytest.raises(ValueError, match="activations_dtype must be"):
        LlamaModel(PRESETS["llama-tiny"], device="cpu", dtype=torch.float32, weights_dtype="fp8", activations_dtype="int8")


def test_activations_dtype_flows_from_configuration_and_environment(monkeypatch):
    from langstream_amd.services import ServiceRegistry
    base = {"device": "cpu", "num-blocks": 16, "use-graphs": "false", "max-model-len": 256, "chat-model": "llama-tiny",
            "weights-dtype": "fp8"}

    def engine(**extra):
        reg = ServiceRegistry({**base, **extra})
        try:
            e = reg.llm_engine("llama-tiny")
            return e.stats["activations_dtype"], e.model.activations_dtype
        finally:
            reg.shutdown()

    monkeypatch.delenv("LS_ACTIVATIONS_DTYPE", raising=False)
    assert engine() == ("bf16", "bf16")
    assert engine(**{"activations-dtype": "fp8"}) == ("fp8", "fp8")
    monkeypatch.setenv("LS_ACTIVATIONS_DTYPE", "fp8")
    assert engine() == ("fp8", "fp8")
    assert engine(**{"activations-dtype": "bf16"}) == ("bf16", "bf16")     # the key wins over the environment
    with pytest.raises(ValueError, match="needs weights_dtype"):
        engine(**{"weights-dtype": "bf16"})
    monkeypatch.delenv("LS_ACTIVATIONS_DTYPE")
    with pytest.raises(ValueError, match="activations-dtype"):
        engine(**{"activations-dtype": "auto"})
    from langstream_amd.core.config_model import docs_markdown
    assert "| `activations-dtype` | string |" in docs_markdown()


def test_cpu_a8_model_differs_from_w8a16_only_above_four_rows():
    m16 = LlamaModel(PRESETS["llama-tiny"], device="cpu", dtype=torch.float32, weights_dtype="fp8")
    m8 = LlamaModel(PRESETS["llama-tiny"], device="cpu", dtype=torch.float32, weights_dtype="fp8", activations_dtype="fp8")
    m8.load_state_dict(m16.state_dict())

    def first_top(model, n):
        e = LLMEngine(model, None, num_blocks=16, max_model_len=256, max_batch=4)
        got = []
        r = e.submit(list(range(3, 3 + n)), SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True, logprobs=5),
                     callback=got.append)
        while not r.finished:
            e.step()
        e._flush()
        return got[0].top

    assert first_top(m8, 4) == first_top(m16, 4)          # T <= 4 keeps the W8A16 projection
    a, b = first_top(m8, 40), first_top(m16, 40)
    assert a != b and abs(a[0][1] - b[0][1]) < 0.05       # the option does something, and not much
