"""hip.Engine(kv_type="q8_0") and Llama(type_k=8, type_v=8) on a tiny llama, qwen2 (Q|K|V biases, G = 7) and
qwen3 (QK-norm). Bounds are the other engine tests': 5e-2 against the fp32 reference, TIGHT between a
batched row and the same row decoded singly (both read the same quantised cache format)."""
import numpy as np
import pytest

from gpu_helpers import rel_err

pytestmark = pytest.mark.gpu
SPECS = ["tiny-llama3-q4_k_m", "tiny-qwen2-g7", "tiny-qwen3-g4-hd64"]
TIGHT, GREEDY = 1.5e-2, {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    import torch
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("kv_q8_models")
    return {s: write_synthetic_gguf(s, str(d / f"{s}.gguf"), seed=3) for s in SPECS}


def _engine(path, n_slots=1, graph=True, kv_type="q8_0", **kw):
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    return load_hip().Engine(path, n_ctx=256, n_batch=128, device=0, use_graph=graph, n_slots=n_slots, kv_type=kv_type, **kw)


@pytest.mark.parametrize("spec", SPECS)
def test_prefill_and_greedy_decode_match_reference(models, spec):
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    ref = ReferenceLlama(GGUFReader(models[spec]), n_ctx=256)
    eng = _engine(models[spec])
    toks = [int(t) for t in np.random.default_rng(0).integers(0, ref.hp.n_vocab, 39)]
    got = eng.eval_logits(toks, 0)
    assert rel_err(got, ref.forward(toks, 0).numpy()) < 5e-2
    for i in range(39, 55):   # 16 greedy steps on the prefilled cache
        tok = int(np.argmax(got))
        got = eng.decode_logits(tok, i)
        e = rel_err(got, ref.forward([tok], i).numpy())
        assert e < 5e-2, (spec, i, e)
    # graph and eager on one cache (the graph engine's rows 0..53 copied over): the last step's logits,
    # and a further replay of the graph, bit-equal
    eager = _engine(models[spec], graph=False)
    eager.kv_load(eng.kv_save(54), 54)
    assert np.array_equal(np.asarray(got), np.asarray(eager.decode_logits(tok, 54)))
    assert np.array_equal(np.asarray(got), np.asarray(eng.decode_logits(tok, 54)))


@pytest.mark.parametrize("spec", SPECS)
def test_batched_rows_match_single_row_decode(models, spec):
    eng, one = _engine(models[spec], n_slots=4, graph=False), _engine(models[spec], graph=False)
    for p in eng.batch_plan(3):
        assert (p["qkv"], p["finish"], p["kv"]) == ("unfused", "rope_kv_append_q8", "q8_0"), p
    assert _engine(models[spec], n_slots=4, kv_type="f16").batch_plan(3)[0]["kv"] == "f16"
    rng = np.random.default_rng(3)
    slots, seqs, plen, rows = [3, 0, 1], {}, {}, {}
    for s, n in zip(slots, (5, 40, 17)):
        prompt = [int(t) for t in rng.integers(3, 300, n)]
        seqs[s], plen[s], rows[s] = prompt + [eng.slot_begin(s, prompt, 0, GREEDY)], n, []
    for _ in range(3):
        toks = eng.batch_step(slots)
        logits = eng.batch_logits(len(slots))
        for b, s in enumerate(slots):
            rows[s].append(np.array(logits[b]))
            seqs[s].append(toks[b])
    assert eng.healthy
    for s in slots:
        one.eval_logits(seqs[s][:plen[s]], 0)
        for k in range(3):
            e = rel_err(rows[s][k], one.decode_logits(seqs[s][plen[s] + k], plen[s] + k))
            assert e < TIGHT, (spec, s, k, e)


def test_device_bytes_shrink_by_the_kv_ratio(models):
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    path = models[SPECS[0]]
    md = GGUFReader(path).metadata
    n_layer, n_kv = int(md["llama.block_count"]), int(md["llama.attention.head_count_kv"])
    hd = int(md["llama.embedding_length"]) // int(md["llama.attention.head_count"])
    f16_kv = 2 * 3 * n_layer * n_kv * 256 * hd * 2   # K and V, 3 slots, n_ctx 256
    a, b = _engine(path, n_slots=3, kv_type="f16").device_bytes, _engine(path, n_slots=3).device_bytes
    assert abs((a - b) - f16_kv * (1 - 34 / 64)) <= 2 * 4096, (a, b, f16_kv)


def test_refusals(models):
    path = models[SPECS[0]]
    for kw, word in (({"kv_type": "q4_0"}, "kv_type"), ({"layer_begin": 1}, "kv_type=q8_0"), ({"layer_end": 1}, "kv_type=q8_0")):
        with pytest.raises(RuntimeError, match=word):
            _engine(path, **kw)


def test_facade(models):
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    path = models[SPECS[0]]
    llm = Llama(path, n_gpu_layers=-1, n_ctx=256, n_batch=64, seed=1, verbose=False, type_k=8, type_v=8, logits_all=True)
    assert llm._backend.kv_type == "q8_0"
    prompt = "the quick brown fox"
    first = llm(prompt, max_tokens=6, temperature=0.0)["choices"][0]["text"]
    state = llm.save_state()
    more = llm(prompt + first, max_tokens=6, temperature=0.0)["choices"][0]["text"]
    llm.load_state(state)
    assert llm(prompt + first, max_tokens=6, temperature=0.0)["choices"][0]["text"] == more
    assert np.isfinite(np.asarray(llm.embed(prompt))).all()
    assert np.isfinite([v for v in llm.score(prompt)["token_logprobs"] if v is not None]).all()
    f16 = Llama(path, n_gpu_layers=-1, n_ctx=256, n_batch=64, seed=1, verbose=False)
    with pytest.raises(Exception, match="size mismatch"):   # a state of one cache type, an engine of the other
        f16.load_state(state)
    with pytest.raises(ValueError, match="type_k=8 and type_v=1"):
        Llama(path, n_gpu_layers=-1, n_ctx=64, verbose=False, type_k=8, type_v=1)
    with pytest.raises(ValueError, match="type_k=2"):
        Llama(path, n_gpu_layers=-1, n_ctx=64, verbose=False, type_k=2)
