"""``Llama(logits_all=True)``, ``Llama.score`` and echoed prompt log-probabilities on the CPU and
reference backends (plain host implementations: every row's logits, log_softmax in fp64), and the
``LOGITS_ALL`` setting. The MI355X engine's route is tests/test_score_engine_gpu.py."""
import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.config import Settings
from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf

# the C++ CPU backend's logits against the fp32 reference are held to this (tests/test_cpu_backend.py)
CPU_VS_REF = 0.06
TEXT = "the quick brown fox jumps over the lazy dog"


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    return write_synthetic_gguf("tiny-llama3-q4_k_m", str(tmp_path_factory.mktemp("score_models") / "m.gguf"))


def _llm(path, backend, **kw):
    return Llama(path, n_ctx=64, backend=backend, seed=0, n_threads=2, verbose=False, **kw)


def test_echo_logprobs_need_logits_all(path):
    gen = dict(max_tokens=4, temperature=0.0, echo=True, logprobs=1)
    off, on, ref = _llm(path, "cpu"), _llm(path, "cpu", logits_all=True), _llm(path, "reference", logits_all=True)
    a = off.create_completion(TEXT, **gen)["choices"][0]["logprobs"]
    b = on.create_completion(TEXT, **gen)["choices"][0]["logprobs"]
    n = len(off.tokenize(TEXT)) - 1   # echoed tokens listed (BOS is not)
    assert a["token_logprobs"][:n] == [None] * n and a["top_logprobs"][:n] == [None] * n
    assert None not in b["token_logprobs"] and len(b["token_logprobs"]) == n + 4
    assert b["tokens"] == a["tokens"] and b["token_logprobs"][n:] == a["token_logprobs"][n:]
    assert all(1 <= len(d) <= 2 and max(d.values()) <= 0 for d in b["top_logprobs"][:n])
    want = ref.create_completion(TEXT, **gen)["choices"][0]["logprobs"]["token_logprobs"][:n]
    assert rel_err(b["token_logprobs"][:n], want) < CPU_VS_REF
    assert b["token_logprobs"][:n] == on.score(TEXT)["token_logprobs"][1:]
    # logprobs=0: every position, generated ones included, carries its own value and no alternative
    z = on.create_completion(TEXT, **dict(gen, logprobs=0))["choices"][0]["logprobs"]
    assert z["token_logprobs"] == b["token_logprobs"] and all(len(d) == 1 for d in z["top_logprobs"])


@pytest.mark.parametrize("backend", ["reference", "cpu"])
def test_score_input_forms(path, backend):
    llm = _llm(path, backend, logits_all=True)
    toks = llm.tokenize(TEXT, add_bos=True, special=True)
    one = llm.score(TEXT)
    assert one["tokens"] == toks and one["token_logprobs"][0] is None and one["greedy"][0] is None
    assert len(one["token_logprobs"]) == len(one["greedy"]) == len(toks)
    assert all(v <= 0 for v in one["token_logprobs"][1:]) and all(isinstance(g, bool) for g in one["greedy"][1:])
    assert abs(one["logprob"] - sum(one["token_logprobs"][1:])) < 1e-4
    assert llm.score(toks) == one                                  # a list of ids is one input
    two = llm.score([TEXT, toks[:5]])
    assert two[0] == one and two[1]["greedy"] == one["greedy"][:5]
    # causal: a prefix scores as it does inside the longer input (another GEMM shape: not bit-equal)
    assert np.allclose(two[1]["token_logprobs"][1:], one["token_logprobs"][1:5], rtol=0, atol=1e-3)
    assert llm.score([toks[:5]]) == [two[1]] and llm._kv_tokens == []
    for bad in ([], [[]], [toks[0], 10 ** 6], toks * 10):
        with pytest.raises(ValueError):
            llm.score(bad)
    with pytest.raises(RuntimeError, match="logits_all"):
        _llm(path, backend).score(TEXT)


def test_backends_that_refuse(path):
    llm = _llm(path, "cpu", logits_all=True)
    llm._backend.tp_size = 2
    with pytest.raises(NotImplementedError, match="cpu"):
        llm.score(TEXT)
    # a backend without the call (the hybrid and layer-split ones; built for real in test_score_engine_gpu)
    llm._backend, llm.backend_name = object(), "hybrid"
    with pytest.raises(NotImplementedError, match="hybrid"):
        llm.score(TEXT)


def test_setting_from_env(monkeypatch):
    from llama_fastapi_k8s_gpu_amd.engine import factory
    assert Settings.from_env().logits_all is False
    monkeypatch.setenv("LOGITS_ALL", "1")
    s = Settings.from_env()
    assert s.logits_all is True
    seen = {}
    monkeypatch.setattr("llama_fastapi_k8s_gpu_amd.engine.llama.Llama", lambda **kw: seen.update(kw))
    factory.build_engine(s)
    assert seen["logits_all"] is True
    s.logits_all = False
    seen.clear()
    factory.build_engine(s)
    assert "logits_all" not in seen
