"""Text embeddings on the MI355X engine (``Engine.embed``: a packed prefill with no lm_head and no
sampler that ends in the pooling epilogue, csrc/kernels/misc.hip pool_rows / pool_finish), against
the fp32 reference model pooled in fp64, on engines with four KV slots and with one; through the
``Llama`` facade with the batch scheduler beside running generations; and the backends that refuse.

Bounds: ``rel_err < 5e-2`` is what every engine test gives a logits row against the fp32 reference
(the engine's f16 / bf16 / int8 roundings); TIGHT is the batch tests' bound between two engine paths
of one spec. Mean pooling is compared on inputs whose rows do not cancel (asserted on the reference:
||mean of rows|| >= 0.25 mean ||row||), so that a relative error means something.
"""
import numpy as np
import pytest

from gpu_helpers import rel_err

pytestmark = pytest.mark.gpu

QWEN3_MD = {"qwen3.pooling_type": 3, "tokenizer.ggml.add_eos_token": True}
SPECS = ["tiny-llama3-q4_k_m", "tiny-tinyllama-q8_0", "tiny-qwen3-g4-hd64", "tiny-mixtral-q4_k_m"]
# test_batch_gpu.TIGHT / test_qwen3_gpu.TIGHT
TIGHT = {"tiny-llama3-q4_k_m": 1.5e-2, "tiny-tinyllama-q8_0": 1.5e-2, "tiny-qwen3-g4-hd64": 1.5e-2,
         "tiny-mixtral-q4_k_m": 3e-2}
MODES = {"none": 0, "mean": 1, "cls": 2, "last": 3}
_rng = np.random.default_rng(5)
SHORT = [[int(t) for t in _rng.integers(3, 300, n)] for n in (5, 12, 9)]
# repeated tokens: rows that do not cancel in the mean at these lengths; they cross 32-row chunk borders
LONG = [[7, 8, 9] * 14, [5] * 35 + [6] * 35, [11, 12] * 17]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    d = tmp_path_factory.mktemp("embed_models")
    return {s: write_synthetic_gguf(s, str(d / f"{s}.gguf"), extra_metadata=QWEN3_MD if "qwen3" in s else None)
            for s in SPECS}


@pytest.fixture(scope="module")
def ref_rows(models):
    """The reference's normed final rows (fp64) per (spec, input), computed once."""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    cache, refs = {}, {}

    def get(spec, toks):
        key = (spec, tuple(toks))
        if key not in cache:
            if spec not in refs:
                refs[spec] = ReferenceLlama(GGUFReader(models[spec]), n_ctx=256)
            cache[key] = refs[spec].hidden(list(toks)).numpy().astype(np.float64)
        return cache[key]
    return get


def engine(path, n_slots, **kw):
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    args = dict(n_ctx=256, n_batch=64, device=0, use_graph=True, n_slots=n_slots)
    args.update(kw)
    return load_hip().Engine(path, **args)


def pooled(rows, mode, normalize):
    from llama_fastapi_k8s_gpu_amd.engine.pooling import pool_host
    return pool_host(rows, mode, normalize, np.float64)


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def check_vs_reference(got, rows, mode, normalize, tag, worst):
    if mode == 1:
        assert np.linalg.norm(rows.mean(0)) >= 0.25 * np.linalg.norm(rows, axis=1).mean(), tag
    want = pooled(rows, mode, normalize)
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32, (tag, got.shape, want.shape)
    e = rel_err(got, want)
    worst[0] = max(worst[0], e / 5e-2)
    assert e < 5e-2, (tag, e)
    if got.ndim == 1:
        assert cosine(got, want) >= 0.99, (tag, cosine(got, want))
    else:
        assert min(cosine(g, w) for g, w in zip(got, want)) >= 0.99, tag
    if normalize:
        assert np.allclose(np.linalg.norm(got.reshape(-1, got.shape[-1]), axis=1), 1, atol=1e-5), tag


def embed_each(eng, slots, inputs, mode, normalize):
    """Engine.embed -> one array per input ([d], or for none [n_i][d])."""
    r = eng.embed(slots, inputs, mode, normalize)
    return list(r) if mode == 0 else [r[i] for i in range(len(inputs))]


@pytest.mark.parametrize("spec", SPECS)
def test_packed_and_alone_against_reference(models, ref_rows, spec):
    """Four slots: three inputs of different lengths packed in one call, all four modes, plain and
    normalised, against the reference; and against each input alone in a slot of its own (TIGHT).
    One slot: the same inputs one by one through slot 0."""
    eng4, eng1 = engine(models[spec], 4), engine(models[spec], 1)
    worst, worst_t = [0.0], 0.0
    for mname, mode in MODES.items():
        for normalize in (False, True):
            packed = embed_each(eng4, [3, 0, 1], SHORT, mode, normalize)
            for i, toks in enumerate(SHORT):
                tag = (spec, mname, normalize, i)
                check_vs_reference(packed[i], ref_rows(spec, toks), mode, normalize, tag, worst)
                alone = embed_each(eng4, [2], [toks], mode, normalize)[0]
                worst_t = max(worst_t, rel_err(packed[i], alone) / TIGHT[spec])
                assert rel_err(packed[i], alone) < TIGHT[spec], tag
                single = embed_each(eng1, [0], [toks], mode, normalize)[0]
                check_vs_reference(single, ref_rows(spec, toks), mode, normalize, tag + ("one slot",), worst)
    print(f"test_embed_engine_gpu packed/alone {spec}: vs reference / 5e-2 = {worst[0]:.3f}, "
          f"packed vs alone / TIGHT = {worst_t:.3f}")
    assert eng4.healthy and eng1.healthy


@pytest.mark.parametrize("spec", ["tiny-llama3-q4_k_m", "tiny-qwen3-g4-hd64"])
def test_inputs_across_chunk_borders(models, ref_rows, spec, monkeypatch):
    """LFK_JOINT_ROWS=0 with n_batch 32: packed chunks of 32 rows, so every input arrives in several
    pieces and the accumulator rows carry their sums; the one-slot engine takes its input in three
    chunks."""
    monkeypatch.setenv("LFK_JOINT_ROWS", "0")
    eng4, eng1 = engine(models[spec], 4, n_batch=32), engine(models[spec], 1, n_batch=32)
    monkeypatch.delenv("LFK_JOINT_ROWS", raising=False)
    worst = [0.0]
    for mname, mode in MODES.items():
        packed = embed_each(eng4, [1, 2, 3], LONG, mode, mode != 0)
        for i, toks in enumerate(LONG):
            check_vs_reference(packed[i], ref_rows(spec, toks), mode, mode != 0, (spec, mname, i), worst)
        single = embed_each(eng1, [0], [LONG[1]], mode, False)[0]
        check_vs_reference(single, ref_rows(spec, LONG[1]), mode, False, (spec, mname, "one slot"), worst)
    print(f"test_embed_engine_gpu chunk borders {spec}: vs reference / 5e-2 = {worst[0]:.3f}")


@pytest.mark.parametrize("n_slots", [4, 1])
def test_input_of_exactly_n_ctx(models, ref_rows, n_slots):
    spec = "tiny-llama3-q4_k_m"
    eng = engine(models[spec], n_slots, n_ctx=64, n_batch=32)
    toks = ([7, 8, 9] * 22)[:64]
    worst = [0.0]
    for mname, mode in MODES.items():
        got = embed_each(eng, [n_slots - 1], [toks], mode, True)[0]
        check_vs_reference(got, ref_rows(spec, toks), mode, True, (mname, n_slots), worst)
    print(f"test_embed_engine_gpu n_ctx tokens, {n_slots} slots: vs reference / 5e-2 = {worst[0]:.3f}")
    with pytest.raises(RuntimeError, match="context"):
        eng.embed([0], [toks + [1]], 1, False)
    assert eng.healthy


def test_refused_arguments(models):
    eng = engine(models["tiny-llama3-q4_k_m"], 4)
    for slots, inputs, mode in (([1, 1], [[1], [2]], 1), ([4], [[1]], 1), ([], [], 1), ([1], [[]], 1),
                                ([1], [[1]], 4), ([1, 2], [[1]], 1), ([0, 1, 2, 3, 0], [[1]] * 5, 1)):
        with pytest.raises(RuntimeError, match="embed"):
            eng.embed(slots, inputs, mode, False)
    with pytest.raises(RuntimeError, match="embed"):
        engine(models["tiny-llama3-q4_k_m"], 1).embed([0, 0], [[1], [2]], 1, False)


def test_generation_is_unaffected(models):
    """slots_begin / batch_step on slots 1 and 2, an embed on slot 3 between the steps: tokens and
    logits bit-equal to a run without it - it touches neither the other slots' KV nor any sampling
    state."""
    path = models["tiny-llama3-q4_k_m"]
    sp = {"temperature": 0.9, "top_k": 20, "seed": 11, "repeat_penalty": 1.1}
    prompts = [SHORT[1], SHORT[2]]

    def run(with_embed):
        eng = engine(path, 4)
        out = [list(eng.slots_begin([1, 2], prompts, [0, 0], [sp, sp]))]
        logits = []
        for step in range(5):
            if with_embed and step == 2:
                eng.embed([3], [LONG[0]], 1, True)
            out.append(list(eng.batch_step([1, 2])))
            logits.append(np.array(eng.batch_logits(2)))
        assert eng.healthy
        return out, logits
    (t0, l0), (t1, l1), (t2, l2) = run(False), run(True), run(False)
    # the premise: two runs without an embed are bit-equal themselves at this shape
    assert t0 == t2 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(l0, l2)), \
        "two runs WITHOUT an embed differ: the comparison below would say nothing about embed"
    assert t0 == t1
    for a, b in zip(l0, l1):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_facade_with_scheduler_beside_generations(models):
    """Llama(max_batch=4): create_embedding of five strings runs beside two greedy generations. The
    vectors equal the same call on the idle engine within TIGHT; the generations' tokens equal those
    of a run without it.

    The admission schedule is fixed, because a row that decodes alone takes the single-row path, whose
    roundings differ from the batched step's: a long embedding job goes in first, and while its passes
    run the two generations are submitted to the scheduler. Requests younger than a job wait for it,
    so both are admitted together in ONE joint admission (asserted) and decode as two rows of every
    step until both end after the same number of tokens. The facade's create_embedding then arrives
    as the youngest item and borrows the two remaining slots between their steps."""
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    spec = "tiny-qwen3-g4-hd64"
    llm = Llama(models[spec], n_gpu_layers=-1, n_ctx=256, n_batch=64, seed=1, verbose=False, max_batch=4)
    try:
        assert llm.pooling_type == 3 and llm.tokenizer.add_eos_token
        sched = llm._backend.sched
        texts = ["the quick brown fox", "hello world", "a b c d e", "jumps over the lazy dog", "x"]
        idle = llm.create_embedding(texts)
        assert [e["index"] for e in idle["data"]] == list(range(5))
        n = sum(len(llm.tokenize(t, add_bos=True, special=True)) + 1 for t in texts)     # + EOS each
        assert idle["usage"] == {"prompt_tokens": n, "total_tokens": n}
        greedy = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
        prompts = [llm.tokenize(p, add_bos=True, special=True) for p in ("once upon a time", "the answer is")]
        blocker = [[3 + (i + j) % 200 for j in range(200)] for i in range(96)]   # 24 passes of 4 x 200 rows

        def both(with_embedding):
            st0 = sched.stats()
            hold = sched.submit_embed(blocker, 1, False)
            gens = [sched.submit(p, 48, greedy, []) for p in prompts]
            busy = llm.create_embedding(texts) if with_embedding else None
            toks = []
            for g in gens:
                got = []
                while True:
                    r = sched.wait(g, len(got), 50)
                    got += r["tokens"]
                    if r["done"]:
                        break
                assert r["finish"] == "length" and len(got) == 48, r
                sched.release(g)
                toks.append(got)
            r = sched.wait_embed(hold, 10000)
            assert r["done"] and r["finish"] == "done"
            sched.release(hold)
            st = sched.stats()
            # the premise: both generations were admitted in one joint admission, behind the blocker
            assert st["joint_admissions"] - st0["joint_admissions"] == 1 and st["admitted"] - st0["admitted"] == 2, \
                "the generations were not admitted together: the schedule is not the one this test fixes"
            return toks, busy
        quiet, _ = both(False)
        beside, busy = both(True)
        assert beside == quiet
        worst = 0.0
        for a, b in zip(busy["data"], idle["data"]):
            worst = max(worst, rel_err(a["embedding"], b["embedding"]) / TIGHT[spec])
            assert rel_err(a["embedding"], b["embedding"]) < TIGHT[spec]
        print(f"test_embed_engine_gpu facade beside generations: busy vs idle / TIGHT = {worst:.3f}")
        st = llm.health()["batching"]
        assert st["embed_jobs"] == 4 and st["embed_inputs"] == 10 + 2 * 96 and st["embed_tokens"] == 2 * n + 2 * 96 * 200
        one = llm.embed(texts[0], normalize=True)
        assert abs(np.linalg.norm(one) - 1) < 1e-5
    finally:
        llm.close()


def test_facade_without_scheduler(models, ref_rows):
    """One KV slot: embed under the facade's lock on slot 0, and a generation afterwards equals a
    fresh facade's (the prefix bookkeeping was reset)."""
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    spec = "tiny-tinyllama-q8_0"
    kw = dict(n_gpu_layers=-1, n_ctx=256, n_batch=64, seed=1, verbose=False)
    gen_kw = dict(max_tokens=8, temperature=0.0, top_k=1, repeat_penalty=1.0)
    fresh = Llama(models[spec], **kw).create_completion(SHORT[1], **gen_kw)["choices"][0]["text"]
    llm = Llama(models[spec], **kw)
    assert llm.create_completion(SHORT[1], **gen_kw)["choices"][0]["text"] == fresh
    got = llm.embed([SHORT[1] + [4, 5], SHORT[0]], pooling_type=1)
    assert llm._kv_tokens == []
    worst = [0.0]
    check_vs_reference(np.asarray(got[1], np.float32), ref_rows(spec, SHORT[0]), 1, False, "facade", worst)
    assert llm.create_completion(SHORT[1], **gen_kw)["choices"][0]["text"] == fresh


def test_refused_backends(models):
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    path = models["tiny-llama3-q4_k_m"]
    hybrid = Llama(path, n_gpu_layers=2, n_ctx=128, seed=4, verbose=False)
    assert hybrid.backend_name == "hybrid"
    with pytest.raises(NotImplementedError, match="hybrid"):
        hybrid.embed("hello")
    split = Llama(path, split_mode="layer", tensor_split=[1, 1, 2], layer_devices=[0, 0, 0], n_gpu_layers=-1,
                  n_ctx=128, seed=4, verbose=False)
    assert split.backend_name == "layer"
    with pytest.raises(NotImplementedError, match="layer"):
        split.embed("hello")
