"""Prompt log-probabilities on the MI355X engine (``Engine.score``: embed's packed prefill ending in
the output RMSNorm as f16 rows and the scoring head, csrc/kernels/score.hip) against the fp32
reference model (``models/llama.py``, ``all_logits=True``) with log_softmax in fp64.

Bound: ``rel_err < 5e-2``, what every engine test gives a logits row against the fp32 reference
(test_engine_gpu / test_embed_engine_gpu: the engine's f16 / bf16 / int8 roundings), applied to each
input's vector of log-probabilities, of log-sum-exps and of the best tokens' log-probabilities.
The best id cannot be held to the reference's exactly (near-ties), but that bound on a logits row,
||d|| < 5e-2 ||l||, bounds how far the engine's pick b can lie under the reference's r: l_eng[b] >=
l_eng[r] gives l_ref[b] >= l_ref[r] - |d_b| - |d_r| >= l_ref[r] - sqrt(2) 5e-2 ||l_ref||, which is asserted
per row - also for the tokens ``Llama.score`` calls greedy."""
import numpy as np
import pytest

from gpu_helpers import rel_err

pytestmark = pytest.mark.gpu

SPEC = "tiny-llama3-q4_k_m"   # dense, n_embd 256: its head has a tile16 copy
_rng = np.random.default_rng(9)
INPUTS = [[int(t) for t in _rng.integers(3, 300, n)] for n in (42, 70, 34)]   # targets cross 32-row chunk borders


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    return write_synthetic_gguf(SPEC, str(tmp_path_factory.mktemp("score_models") / f"{SPEC}.gguf"))


@pytest.fixture(scope="module")
def ref(model):
    """Per input the reference's records [lp(next token), lse, best, lp(best)] and its logits [T][V]
    (fp64), computed once."""
    from llama_fastapi_k8s_gpu_amd.engine.backends import ReferenceBackend
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    be = ReferenceBackend(GGUFReader(model), 256)
    rows = [np.asarray(r, np.float64) for r in be.score(INPUTS)]
    logits = [be.model.forward(list(toks), 0, all_logits=True).numpy().astype(np.float64) for toks in INPUTS]
    return list(zip(rows, logits))


def check_best(ids, logits, tag):
    """Row r's pick ids[r] is within the logits row's bound of the reference's maximum (module docstring)."""
    ids = np.asarray(ids).astype(np.int64)
    rows = np.arange(len(ids))
    assert (ids >= 0).all() and (ids < logits.shape[1]).all(), tag
    slack = np.sqrt(2) * 5e-2 * np.linalg.norm(logits, axis=1)
    assert (logits[rows, ids] >= logits.max(1) - slack).all(), (tag, "best id")


def engine(path, n_slots, **kw):
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    args = dict(n_ctx=256, n_batch=32, device=0, use_graph=True, n_slots=n_slots, scoring=True)
    args.update(kw)
    return load_hip().Engine(path, **args)


def check(got, want_logits, tag, worst):
    want, logits = want_logits
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32, (tag, got.shape)
    assert np.isnan(got[-1, 0]) and np.isfinite(got[:-1]).all() and np.isfinite(got[-1, 1:]).all(), tag
    for col, name in ((0, "lp"), (1, "lse"), (3, "lp(best)")):
        n = len(got) - (col == 0)
        e = rel_err(got[:n, col], want[:n, col])
        worst[0] = max(worst[0], e / 5e-2)
        assert e < 5e-2, (tag, name, e)
    assert (got[:-1, 3] >= got[:-1, 0]).all(), tag
    check_best(got[:, 2], logits, tag)


def test_packed_and_alone_against_reference(model, ref, monkeypatch):
    """Four slots, packed chunks of 32 rows (LFK_JOINT_ROWS=0): three inputs in one call, every
    input in several pieces; each alone in a slot of its own; and one by one on a one-slot engine."""
    monkeypatch.setenv("LFK_JOINT_ROWS", "0")
    eng4, eng1 = engine(model, 4), engine(model, 1)
    monkeypatch.delenv("LFK_JOINT_ROWS", raising=False)
    assert eng4.scoring and eng1.scoring
    worst = [0.0]
    packed = eng4.score(INPUTS, [3, 0, 1])
    for i, toks in enumerate(INPUTS):
        check(packed[i], ref[i], ("packed", i), worst)
        check(eng4.score([toks], [2])[0], ref[i], ("alone", i), worst)
        check(eng1.score([toks], [0])[0], ref[i], ("one slot", i), worst)
    print(f"test_score_engine_gpu: vs reference / 5e-2 = {worst[0]:.3f}")
    with pytest.raises(RuntimeError, match="score"):
        eng4.score([[1], [2]], [1, 1])
    with pytest.raises(RuntimeError, match="score"):
        eng4.score([[1, 100000]], [1])
    with pytest.raises(RuntimeError, match="scoring"):
        engine(model, 1, scoring=False).score([[1, 2]], [0])
    assert eng4.healthy and eng1.healthy


def test_generation_is_unaffected(model):
    """slots_begin / batch_step on slots 1 and 2, a score on slot 3 between the steps: tokens and
    batch_logits bit-equal to a run without it."""
    sp = {"temperature": 0.9, "top_k": 20, "seed": 11, "repeat_penalty": 1.1}
    prompts = [INPUTS[0][:12], INPUTS[1][:9]]

    def run(with_score):
        eng = engine(model, 4, n_batch=64)
        out = [list(eng.slots_begin([1, 2], prompts, [0, 0], [sp, sp]))]
        logits = []
        for step in range(5):
            if with_score and step == 2:
                eng.score([INPUTS[2]], [3])
            out.append(list(eng.batch_step([1, 2])))
            logits.append(np.array(eng.batch_logits(2)))
        assert eng.healthy
        return out, logits
    (t0, l0), (t1, l1), (t2, l2) = run(False), run(True), run(False)
    assert t0 == t2 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(l0, l2)), \
        "two runs WITHOUT a score differ: the comparison below would say nothing"
    assert t0 == t1
    for a, b in zip(l0, l1):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refused_backends(model):
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    hybrid = Llama(model, n_gpu_layers=2, n_ctx=128, seed=4, verbose=False, logits_all=True)
    assert hybrid.backend_name == "hybrid"
    with pytest.raises(NotImplementedError, match="hybrid"):
        hybrid.score("hello")
    split = Llama(model, split_mode="layer", tensor_split=[1, 1, 2], layer_devices=[0, 0, 0], n_gpu_layers=-1,
                  n_ctx=128, seed=4, verbose=False, logits_all=True)
    assert split.backend_name == "layer"
    with pytest.raises(NotImplementedError, match="layer"):
        split.score("hello")


@pytest.mark.parametrize("max_batch", [1, 4])
def test_facade_echo_logprobs(model, ref, max_batch):
    """logits_all=True: create_completion(echo=True, logprobs=1) carries a log-probability for every
    prompt token but the first, equal to Llama.score's; generated positions equal those of the same
    call on a logits_all=False instance (whose echoed tokens keep None)."""
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    kw = dict(n_gpu_layers=-1, n_ctx=256, n_batch=32, seed=1, verbose=False)
    if max_batch > 1:
        kw["max_batch"] = max_batch
    gen = dict(max_tokens=6, temperature=0.0, top_k=1, repeat_penalty=1.0, echo=True, logprobs=1)
    toks = INPUTS[0]
    llm = Llama(model, logits_all=True, **kw)
    plain = Llama(model, **kw)
    try:
        a = llm.create_completion(toks, **gen)["choices"][0]["logprobs"]
        b = plain.create_completion(toks, **gen)["choices"][0]["logprobs"]
        n = len(toks)
        assert a["token_logprobs"][0] is None and None not in a["token_logprobs"][1:]
        assert b["token_logprobs"][:n] == [None] * n
        assert a["token_logprobs"][n:] == b["token_logprobs"][n:] and a["top_logprobs"][n:] == b["top_logprobs"][n:]
        assert a["tokens"] == b["tokens"] and all(1 <= len(d) <= 2 for d in a["top_logprobs"][1:n])
        sc = llm.score(toks)
        assert sc["token_logprobs"][1:] == a["token_logprobs"][1:n] and sc["token_logprobs"][0] is None
        assert rel_err(sc["token_logprobs"][1:], ref[0][0][:-1, 0]) < 5e-2
        greedy = [i for i, g in enumerate(sc["greedy"]) if g]          # token i is row i - 1's pick
        check_best([toks[i] for i in greedy], ref[0][1][[i - 1 for i in greedy]], "greedy")
        assert abs(sc["logprob"] - sum(sc["token_logprobs"][1:])) < 1e-3 and len(sc["greedy"]) == n
        with pytest.raises(RuntimeError, match="logits_all"):
            plain.score(toks)
    finally:
        llm.close()
        plain.close()
