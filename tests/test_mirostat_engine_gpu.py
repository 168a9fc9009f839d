"""Mirostat on the device sampler through the engine, the scheduler and the facade (tiny-llama3-q4_k_m,
n_ctx 256): every step's token against the fp64 reference of tests/mirostat_ref.py over that step's
logits with mu carried from 2 tau, graph equal to eager, plain rows untouched by a mirostat neighbour,
and a mirostat request decoding as a row of the shared batch. The reference carries mu in fp64 while
the device rounds it once per step (each within d_mu < the threshold bound), so step k asks its
decisions to be k + 2 bounds away instead of 1."""
import threading

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.engine.sampling import SamplingParams
from mirostat_ref import reference

pytestmark = pytest.mark.gpu

PROMPTS = [[1, 7, 42, 99, 5, 311, 17, 4], [1, 9, 9, 250, 33], [1, 100, 101, 102, 103, 104, 105, 106, 107, 108, 3]]
PLAIN = {"temperature": 0.9, "top_k": 40, "seed": 11, "repeat_penalty": 1.3, "presence_penalty": 0.5}


def _miro(mode):
    if mode == 1:   # (mirostat_ref: v1's k is exact only without bias, penalties and temperature)
        return SamplingParams(temperature=1.0, seed=5, repeat_penalty=1.0, mirostat_mode=1, mirostat_tau=3.0,
                              mirostat_eta=0.2)
    return SamplingParams(temperature=0.9, seed=5, repeat_penalty=1.3, presence_penalty=0.5, logit_bias={5: 4.0},
                          mirostat_mode=mode, mirostat_tau=3.0, mirostat_eta=0.2)


def _sp(p):
    from llama_fastapi_k8s_gpu_amd.runtime.hip_backend import gpu_sampling_dict
    return gpu_sampling_dict(p, 1 << 30)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    return write_synthetic_gguf("tiny-llama3-q4_k_m", str(tmp_path_factory.mktemp("miro_engine") / "m.gguf"))


def _engine(model, n_slots=4, graph=True):
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    return load_hip().Engine(model, n_ctx=256, n_batch=64, device=0, use_graph=graph, n_slots=n_slots)


def _follow(p, prompt, toks, logits_of):
    """Every token against the reference over logits_of(k), the window and the carried mu."""
    mu, margin = 2.0 * p.mirostat_tau, np.inf
    for k, tok in enumerate(toks):
        r = reference(np.asarray(logits_of(k), np.float32), p, (prompt + toks[:k])[-64:], mu, k, extreme=False)
        assert r["margin"] > k + 2, (k, r["margin"])
        assert tok == r["token"], (k, tok, r["token"], r["k"])
        mu, margin = r["mu"], min(margin, r["margin"])
    return margin


@pytest.mark.parametrize("mode", [2, 1])
def test_generate_follows_the_reference(model, mode):
    p, prompt = _miro(mode), PROMPTS[0]
    eng = _engine(model, n_slots=1)
    toks = eng.generate(prompt, 0, 8, _sp(p), [], None, None)["tokens"]
    assert len(toks) == 8
    eager = _engine(model, n_slots=1, graph=False).generate(prompt, 0, 8, _sp(p), [], None, None)["tokens"]
    assert eager == toks
    m = _follow(p, prompt, toks, lambda k: eng.eval_logits(prompt, 0) if k == 0 else
                eng.decode_logits(toks[k - 1], len(prompt) + k - 1))
    print(f"mirostat v{mode} generate: smallest margin = {m:.1f}")


def test_batch_step_beside_plain_rows(model):
    """Slots [2, 1, 3]; the third row is mirostat v2 in one engine and plain in the other."""
    p, slots = _miro(2), [2, 1, 3]
    a, b = _engine(model), _engine(model)
    ta = [a.slots_begin(slots, PROMPTS, [0, 0, 0], [PLAIN, PLAIN, _sp(p)])]
    tb = [b.slots_begin(slots, PROMPTS, [0, 0, 0], [PLAIN, PLAIN, dict(PLAIN, seed=5)])]
    logits = [None]
    for _ in range(3):
        ta.append(a.batch_step(slots))
        tb.append(b.batch_step(slots))
        la, lb = np.asarray(a.batch_logits(3)), np.asarray(b.batch_logits(3))
        assert np.array_equal(la[:2].view(np.int32), lb[:2].view(np.int32))
        logits.append(la[2])
    assert [t[:2] for t in ta] == [t[:2] for t in tb]
    logits[0] = b.eval_logits(PROMPTS[2], 0)   # (slot 0: none of the three rows)
    m = _follow(p, PROMPTS[2], [t[2] for t in ta], lambda k: logits[k])
    print(f"mirostat batch_step: smallest margin = {m:.1f}")
    assert a.healthy, a.last_error


def test_facade_mirostat_request_shares_the_batch(model):
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    llm = Llama(model, n_gpu_layers=-1, n_ctx=256, n_batch=64, seed=1, verbose=False, max_batch=4)
    be = llm._backend
    assert be.batches(SamplingParams(temperature=0.8, mirostat_mode=2))
    assert not be.batches(SamplingParams(temperature=0.8, mirostat_mode=2, n_probs=21))
    st0, out, errs = be.sched.stats(), {}, []

    def client(i):
        try:
            kw = {"temperature": 0.8, "mirostat_mode": 2, "seed": 3} if i == 0 else {"temperature": 0.0}
            out[i] = llm.create_completion(f"request number {i}: count", max_tokens=20, **kw)
        except Exception as e:  # pragma: no cover
            errs.append(e)
    th = [threading.Thread(target=client, args=(i,)) for i in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not errs, errs
    st = be.sched.stats()
    steps, rows = st["steps"] - st0["steps"], st["rows"] - st0["rows"]
    assert steps > 0 and rows > steps, (steps, rows)   # shared steps
    assert all(out[i]["usage"]["completion_tokens"] > 0 for i in range(3))
    llm.close()
