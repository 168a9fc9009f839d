"""Device token log-probabilities through the engine, the scheduler and the facade on the MI355X
(tiny-llama3-q4_k_m, n_ctx 256): every place a token is sampled hands out the record of exactly that
token and of the RAW logits that step left behind, a request asking for them decodes as a row of the
shared batch, and a run in which nobody asks queues no extra launch."""
import threading

import numpy as np
import pytest

from logprobs_ref import LP_ABS, LP_ULPS, check_logprobs, ulp32

pytestmark = pytest.mark.gpu

GREEDY = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
# a sampled (not greedy) chain with a bias and penalties: the records must still describe the raw logits
SAMPLED = {"temperature": 0.9, "top_k": 40, "seed": 11, "repeat_penalty": 1.3, "presence_penalty": 0.5,
           "logit_bias": {5: 4.0, 17: -3.0}}
PROMPTS = [[1, 7, 42, 99, 5, 311, 17, 4], [1, 9, 9, 250, 33], [1, 100, 101, 102, 103, 104, 105, 106, 107, 108, 3]]
N_PROBS = [5, 0, 20]
LOGIT_MAX = 32.0   # the synthetic model's logits stay below this (asserted where the logits are at hand)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    return write_synthetic_gguf("tiny-llama3-q4_k_m", str(tmp_path_factory.mktemp("lp_engine") / "m.gguf"))


def _engine(model, n_slots=4):
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    return load_hip().Engine(model, n_ctx=256, n_batch=64, device=0, use_graph=True, n_slots=n_slots)


def _sps():
    return [dict(SAMPLED if n else GREEDY, n_probs=n) for n in N_PROBS]


def _well_formed(entry, tok, n):
    lp, top = entry
    assert lp <= 0 and len(top) == n
    vals = [v for _, v in top]
    assert vals == sorted(vals, reverse=True) and all(v <= 0 for v in vals)
    for i, v in top:
        if i == tok:
            assert v == lp


def _begin(eng, slots):
    toks = eng.slots_begin(slots, PROMPTS, [0, 0, 0], _sps())
    first = eng.step_logprobs()
    assert len(first) == 3 and first[1] is None
    for b in (0, 2):
        _well_formed(first[b], toks[b], N_PROBS[b])
    return toks


def test_batch_step_records_describe_the_steps_logits(model):
    eng = _engine(model)
    slots = [2, 1, 3]
    _begin(eng, slots)
    n0 = eng.logprob_launches
    assert n0 == 2       # the two asking prompts' first tokens
    worst = 0.0
    for step in range(3):
        toks = eng.batch_step(slots)
        lps = eng.step_logprobs()
        logits = eng.batch_logits(3)
        assert np.abs(logits).max() < LOGIT_MAX
        assert len(lps) == 3 and lps[1] is None
        for b in (0, 2):
            worst = max(worst, check_logprobs(lps[b], logits[b], toks[b], N_PROBS[b]))
    assert eng.logprob_launches == n0 + 3
    # one active row: the single-row decode graph of that slot
    tok = eng.batch_step([3])
    worst = max(worst, check_logprobs(eng.step_logprobs()[0], eng.batch_logits(1)[0], tok[0], 20))
    # a row that does not ask, alone: no launch, no entries
    n1 = eng.logprob_launches
    eng.batch_step([1])
    assert eng.step_logprobs() == [] and eng.logprob_launches == n1
    print(f"logprobs engine batch_step: worst error / bound = {worst:.3f}")
    assert eng.healthy, eng.last_error


def test_generate_records_against_decode_logits(model):
    eng = _engine(model, n_slots=1)
    prompt = PROMPTS[0]
    seen = []
    r = eng.generate(prompt, 0, 7, dict(SAMPLED, n_probs=4), [], None, lambda t: seen.append(("tok", t)),
                     lambda e: seen.append(("lp", e)))
    toks, lps = r["tokens"], r["logprobs"]
    assert len(toks) == 7 and len(lps) == 7
    # each entry reaches the caller right before its token
    assert [k for k, _ in seen] == ["lp", "tok"] * 7
    assert [e for k, e in seen if k == "lp"] == lps and [t for k, t in seen if k == "tok"] == toks
    _well_formed(lps[0], toks[0], 4)
    worst = 0.0
    for k in range(1, 7):   # the logits that produced token k: token k - 1 fed at its position
        logits = np.asarray(eng.decode_logits(toks[k - 1], len(prompt) + k - 1))
        worst = max(worst, check_logprobs(lps[k], logits, toks[k], 4))
    print(f"logprobs engine generate: worst error / bound = {worst:.3f}")
    plain = eng.generate(prompt, 0, 7, dict(SAMPLED), [], None, None)
    assert plain["tokens"] == toks and plain["logprobs"] == []


def test_pipelined_records_pair_with_their_own_step(model):
    """Two steps in flight: step k's records must be those of step k's logits and tokens."""
    slots = [1, 2, 3]
    a, b = _engine(model), _engine(model)
    assert _begin(a, slots) == _begin(b, slots)
    a.batch_launch(slots)
    a.batch_launch(slots)
    got = []
    for _ in range(2):
        toks = a.batch_collect()
        got.append((toks, a.step_logprobs()))
    ref_logits = []
    for k in range(2):
        assert b.batch_step(slots) == got[k][0]
        ref_logits.append(b.batch_logits(3))
    for k in range(2):
        toks, lps = got[k]
        assert len(lps) == 3 and lps[1] is None
        for r in (0, 2):
            check_logprobs(lps[r], ref_logits[k][r], toks[r], N_PROBS[r])
            with pytest.raises(AssertionError):   # (and the neighbouring step's logits are told apart)
                check_logprobs(lps[r], ref_logits[1 - k][r], toks[r], N_PROBS[r])
    assert a.healthy, a.last_error


def _llama(model, max_batch):
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    return Llama(model, n_gpu_layers=-1, n_ctx=256, n_batch=64, seed=1, verbose=False, max_batch=max_batch)


def test_facade_device_and_host_routes_agree(model):
    llm = _llama(model, 1)
    eng = llm._backend.engine
    n0 = eng.logprob_launches
    dev = llm.create_completion("the quick", max_tokens=8, temperature=0.0, logprobs=3)
    n1 = eng.logprob_launches
    assert n1 - n0 >= dev["usage"]["completion_tokens"] > 0      # the device path
    # a second facade, so both routes prefill the whole prompt (the first one's KV prefix would
    # leave the host route one token to evaluate - on the decode kernels, whose logits differ from
    # the prefill GEMM's in the third digit)
    llm2 = _llama(model, 1)
    host = llm2.create_completion("the quick", max_tokens=8, temperature=0.0, logprobs=21)
    assert llm2._backend.engine.logprob_launches == 0              # the host path
    llm2.close()
    d, h = dev["choices"][0]["logprobs"], host["choices"][0]["logprobs"]
    assert dev["choices"][0]["text"] == host["choices"][0]["text"] and d["tokens"] == h["tokens"]
    # the host's values are fp64 results rounded to fp32: one more ulp on top of the kernel's bound
    tol = LP_ABS + (LP_ULPS + 1) * ulp32(LOGIT_MAX)
    for k, (a, b) in enumerate(zip(d["token_logprobs"], h["token_logprobs"])):
        assert abs(a - b) <= tol, (k, a, b)
        da, hb = d["top_logprobs"][k], h["top_logprobs"][k]
        first = list(da)[:3]
        assert first == list(hb)[:3], (k, first, list(hb)[:3])
        assert all(abs(da[p] - hb[p]) <= tol for p in first)
    # streaming on the single-sequence device path: the engine hands each entry over before its token
    n2 = eng.logprob_launches
    text = [c["choices"][0] for c in llm.create_completion("the quick", max_tokens=8, temperature=0.0, logprobs=3,
                                                           stream=True) if c["choices"][0]["text"]]
    assert eng.logprob_launches > n2 and text
    for c in text:
        assert c["logprobs"] is not None and c["logprobs"]["token_logprobs"][0] <= 0, c
        assert c["text"].endswith(c["logprobs"]["tokens"][0])
    llm.close()


def test_facade_logprobs_request_shares_the_batch(model):
    from llama_fastapi_k8s_gpu_amd.engine.sampling import SamplingParams
    llm = _llama(model, 4)
    be = llm._backend
    assert be.batches(SamplingParams(temperature=0.0, n_probs=5))
    assert not be.batches(SamplingParams(temperature=0.0, n_probs=21))
    st0 = be.sched.stats()
    out, errs = {}, []

    def client(i):
        try:
            kw = {"logprobs": 5} if i == 0 else {}
            out[i] = llm.create_completion(f"request number {i}: count", max_tokens=20, temperature=0.0, **kw)
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
    print(f"logprobs beside the batch: {rows / steps:.2f} rows per step over {steps} steps")
    lp = out[0]["choices"][0]["logprobs"]
    n = out[0]["usage"]["completion_tokens"]
    assert len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["tokens"]) == n
    for k in range(n):
        assert lp["token_logprobs"][k] <= 0
        top = lp["top_logprobs"][k]
        assert top[lp["tokens"][k]] == lp["token_logprobs"][k]   # the token's own value where it is listed
        vals = list(top.values())[:5]   # (a token outside its top 5 is appended behind them)
        assert vals == sorted(vals, reverse=True), (k, vals)
    alone = llm.create_completion("request number 0: count", max_tokens=20, temperature=0.0, logprobs=5)
    assert alone["choices"][0]["text"] == out[0]["choices"][0]["text"]
    assert alone["choices"][0]["logprobs"]["tokens"] == lp["tokens"]
    # streaming: every text chunk carries the entry of its own token
    chunks = [c["choices"][0] for c in llm.create_completion("request number 0: count", max_tokens=20,
                                                             temperature=0.0, logprobs=5, stream=True)]
    text = [c for c in chunks if c["text"]]
    assert "".join(c["text"] for c in text) == alone["choices"][0]["text"]
    ref = alone["choices"][0]["logprobs"]
    k = 0
    for c in text:
        assert c["logprobs"] is not None, c
        piece, val = c["logprobs"]["tokens"][0], c["logprobs"]["token_logprobs"][0]
        # (a chunk may hold several tokens' text; its entry is its last token's)
        hit = [j for j in range(k, len(ref["tokens"]))
               if ref["token_logprobs"][j] == val and piece.endswith(ref["tokens"][j])]
        assert hit, (k, c)
        k = hit[0] + 1
    llm.close()


def test_no_logprobs_request_queues_no_launch(model):
    llm = _llama(model, 4)
    be = llm._backend
    outs = []
    th = [threading.Thread(target=lambda i=i: outs.append(
        llm.create_completion(f"plain request {i}", max_tokens=12, temperature=0.7, seed=i))) for i in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert len(outs) == 3
    assert be.engine.logprob_launches == 0 and be.health()["logprob_launches"] == 0
    llm.close()
    solo = _llama(model, 1)
    solo.create_completion("plain request", max_tokens=12, temperature=0.7, seed=1)
    assert solo._backend.engine.logprob_launches == 0
    solo.close()
