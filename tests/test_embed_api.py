"""Text embeddings through the public surfaces: ``Llama.embed`` / ``create_embedding`` on the
reference and C++ CPU backends over tiny synthetic GGUFs, and ``POST /v1/embeddings`` on the fake
engine."""
import asyncio
import base64
import struct

import httpx
import numpy as np
import pytest
from fastapi.testclient import TestClient

from gpu_helpers import rel_err
from llama_fastapi_k8s_gpu_amd.config import Settings
from llama_fastapi_k8s_gpu_amd.engine.fake import FakeEngine
from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
from llama_fastapi_k8s_gpu_amd.models.llama import LlamaHParams, ReferenceLlama
from llama_fastapi_k8s_gpu_amd.runtime import load_cpu
from llama_fastapi_k8s_gpu_amd.server.app import create_app

QWEN3_EMBED_MD = {"qwen3.pooling_type": 3, "tokenizer.ggml.add_eos_token": True}
TEXTS = ["the quick brown fox jumps over the lazy dog", "hello world", "a b c d e f g h i j k l m n o p"]
# mean pooling is compared on short inputs: the rows of these random models are nearly orthogonal, so
# the norm of the mean of n rows is about 1 / sqrt(n) of a row's (the tests assert >= 0.25 on the reference)
MEAN_INPUTS = [[5, 9, 200, 31, 77, 12], [40, 40, 40, 41, 42, 43, 44, 45, 46], list(range(100, 112))]
# the C++ CPU backend's logits against the fp32 reference are held to this (tests/test_cpu_backend.py)
CPU_VS_REF = 0.06


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("embed_models")
    return {"llama3": write_synthetic_gguf("tiny-llama3-q4_k_m", str(d / "llama3.gguf")),
            "qwen3": write_synthetic_gguf("tiny-qwen3-g4-hd64", str(d / "qwen3.gguf"), extra_metadata=QWEN3_EMBED_MD),
            "mean": write_synthetic_gguf("tiny-tinyllama-q8_0", str(d / "mean.gguf"),
                                         extra_metadata={"llama.pooling_type": 1}),
            "rank": write_synthetic_gguf("tiny-llama3-q4_k_m", str(d / "rank.gguf"),
                                         extra_metadata={"llama.pooling_type": 4})}


def _llm(path, backend, **kw):
    return Llama(path, n_ctx=kw.pop("n_ctx", 64), backend=backend, seed=0, n_threads=2, verbose=False, **kw)


# ----------------------------------------------------------------------------- metadata
def test_pooling_type_reaches_every_hparams(paths):
    assert LlamaHParams.from_metadata(GGUFReader(paths["qwen3"]).metadata).pooling_type == 3
    assert LlamaHParams.from_metadata(GGUFReader(paths["llama3"]).metadata).pooling_type == -1
    cpu = load_cpu()
    assert cpu.CpuEngine(paths["qwen3"], n_ctx=32, n_threads=1).hparams["pooling_type"] == 3
    assert cpu.CpuEngine(paths["llama3"], n_ctx=32, n_threads=1).hparams["pooling_type"] == -1


def test_pooling_resolution(paths):
    assert _llm(paths["qwen3"], "reference").pooling_type == 3            # from the metadata
    assert _llm(paths["qwen3"], "reference", pooling_type=1).pooling_type == 1   # the constructor wins
    assert _llm(paths["llama3"], "reference").pooling_type == 0           # absent: none
    assert _llm(paths["llama3"], "reference", embedding=True, pooling_type=-1).pooling_type == 0
    assert _llm(paths["mean"], "cpu").pooling_type == 1


def test_rank_pooling_is_refused(paths):
    llm = _llm(paths["rank"], "reference")      # loads (generation is unaffected) ...
    with pytest.raises(NotImplementedError, match="rank"):
        llm.embed("hello")                      # ... and refuses to embed
    with pytest.raises(NotImplementedError):
        _llm(paths["llama3"], "reference", pooling_type=4).embed("hello")
    with pytest.raises(NotImplementedError):
        _llm(paths["llama3"], "reference", pooling_type=7).embed("hello")


# ----------------------------------------------------------------------------- Llama.embed
@pytest.mark.parametrize("backend", ["reference", "cpu"])
def test_input_shapes_and_counts(paths, backend):
    llm = _llm(paths["mean"], backend)
    d = llm.hparams.n_embd
    one = llm.embed(TEXTS[0])
    assert isinstance(one, list) and len(one) == d and isinstance(one[0], float)     # a single string: one vector
    many = llm.embed(TEXTS)
    assert len(many) == 3 and all(len(v) == d for v in many)
    assert rel_err(many[0], one) < 1e-6                                             # single string against list
    assert rel_err(llm.embed([TEXTS[0]])[0], one) < 1e-6
    toks = llm.tokenize(TEXTS[0], add_bos=True, special=True)
    by_ids = llm.embed(toks)                                                        # a list of ints: one input
    assert len(by_ids) == 1 and rel_err(by_ids[0], one) < 1e-6
    lists = llm.embed([toks, llm.tokenize(TEXTS[1], add_bos=True, special=True)])
    assert len(lists) == 2 and rel_err(lists[1], many[1]) < 1e-6
    res, n = llm.embed(TEXTS, return_count=True)
    assert n == sum(len(llm.tokenize(t, add_bos=True, special=True)) for t in TEXTS)
    assert rel_err(res[2], many[2]) < 1e-6
    unit = llm.embed(TEXTS, normalize=True)
    for u, v in zip(unit, many):
        assert abs(np.linalg.norm(u) - 1) < 1e-5
        assert rel_err(u, np.asarray(v) / np.linalg.norm(v)) < 1e-5


@pytest.mark.parametrize("backend", ["reference", "cpu"])
def test_none_returns_rows(paths, backend):
    llm = _llm(paths["llama3"], backend)           # no pooling key: none
    toks = llm.tokenize(TEXTS[0], add_bos=True, special=True)
    rows = llm.embed(TEXTS[0])
    assert len(rows) == len(toks) and all(len(r) == llm.hparams.n_embd for r in rows)
    both = llm.embed(TEXTS[:2], normalize=True)
    assert len(both) == 2 and len(both[0]) == len(toks)
    assert all(abs(np.linalg.norm(r) - 1) < 1e-5 for r in both[0] + both[1])        # each row's own norm
    # the rows are causal: the first k rows of a longer input are the rows of its k-token prefix
    assert rel_err(llm.embed(toks[:3]), np.asarray(rows)[:3]) < (1e-5 if backend == "reference" else 2e-2)


@pytest.mark.parametrize("backend", ["reference", "cpu"])
def test_truncate_empty_and_full_context(paths, backend):
    llm = _llm(paths["mean"], backend, n_ctx=16)
    long = list(range(3, 3 + 40))
    v, n = llm.embed(long, return_count=True)                # truncate=True: cut to n_ctx tokens
    assert n == 16
    assert rel_err(v[0], llm.embed(long[:16])[0]) < 1e-6     # an input of exactly n_ctx tokens is served
    with pytest.raises(ValueError, match="exceed context window"):
        llm.embed(long, truncate=False)
    with pytest.raises(ValueError):
        llm.embed([[]])                                      # an input with no tokens
    with pytest.raises(ValueError):
        llm.embed([[1, 2], []])
    with pytest.raises(ValueError):
        llm.embed([])


def test_add_eos_token_appends_eos(paths):
    llm = _llm(paths["qwen3"], "reference")
    assert llm.tokenizer.add_eos_token is True and llm.tokenizer.eos_id >= 0
    plain = llm.tokenize(TEXTS[1], add_bos=True, special=True)
    v, n = llm.embed(TEXTS[1], return_count=True)
    assert n == len(plain) + 1
    assert rel_err(v, llm.embed(plain + [llm.tokenizer.eos_id])[0]) < 1e-6    # last pooling: the EOS row
    assert rel_err(v, llm.embed(plain)[0]) > 1e-3
    assert _llm(paths["llama3"], "reference").tokenizer.add_eos_token is False


def test_create_embedding_shape(paths):
    llm = _llm(paths["mean"], "cpu")
    out = llm.create_embedding(TEXTS[:2], model="m")
    n = sum(len(llm.tokenize(t, add_bos=True, special=True)) for t in TEXTS[:2])
    assert out["object"] == "list" and out["model"] == "m"
    assert out["usage"] == {"prompt_tokens": n, "total_tokens": n}
    assert [e["index"] for e in out["data"]] == [0, 1] and all(e["object"] == "embedding" for e in out["data"])
    assert rel_err(out["data"][1]["embedding"], llm.embed(TEXTS[1])) < 1e-6
    single = llm.create_embedding(TEXTS[0])
    assert len(single["data"]) == 1 and len(single["data"][0]["embedding"]) == llm.hparams.n_embd
    assert single["model"] == llm.model_path


# ----------------------------------------------------------------------------- CPU backend against the reference
@pytest.mark.parametrize("model", ["mean", "qwen3", "llama3"])
def test_cpu_backend_agrees_with_reference(paths, model):
    ref, cpu = _llm(paths[model], "reference"), _llm(paths[model], "cpu")
    for pooling in (1, 2, 3, 0):
        inputs = MEAN_INPUTS if pooling == 1 else TEXTS
        want = ref.embed(inputs, pooling_type=pooling)
        got = cpu.embed(inputs, pooling_type=pooling)
        for i, (g, w) in enumerate(zip(got, want)):
            if pooling == 1:
                # a relative error of the mean means something only while the rows do not cancel
                rows = np.asarray(ref.embed(inputs[i], pooling_type=0)[0])
                assert np.linalg.norm(rows.mean(0)) >= 0.25 * np.linalg.norm(rows, axis=1).mean(), (model, i)
            e = rel_err(g, w)
            assert e < CPU_VS_REF, (model, pooling, i, e)
        gotn = cpu.embed(TEXTS[0], pooling_type=pooling, normalize=True)
        assert rel_err(gotn, ref.embed(TEXTS[0], pooling_type=pooling, normalize=True)) < CPU_VS_REF


def test_reference_pools_in_float64(paths):
    llm = _llm(paths["mean"], "reference")
    toks = llm.tokenize(TEXTS[0], add_bos=True, special=True)
    model = ReferenceLlama(GGUFReader(paths["mean"]), n_ctx=64)
    rows = model.hidden(toks).numpy().astype(np.float64)
    assert rows.shape == (len(toks), llm.hparams.n_embd)
    assert rel_err(llm.embed(toks)[0], rows.mean(0)) < 1e-6
    assert rel_err(llm.embed(toks, pooling_type=2)[0], rows[0]) < 1e-6
    assert rel_err(llm.embed(toks, pooling_type=3)[0], rows[-1]) < 1e-6


@pytest.mark.parametrize("backend", ["reference", "cpu"])
def test_generation_after_embed_equals_a_fresh_one(paths, backend):
    kw = dict(max_tokens=6, temperature=0.0, seed=1)
    fresh = _llm(paths["mean"], backend).create_completion(TEXTS[0], **kw)["choices"][0]["text"]
    llm = _llm(paths["mean"], backend)
    first = llm.create_completion(TEXTS[0], **kw)["choices"][0]["text"]
    llm.embed(TEXTS[0] + " and something else entirely")     # shares a prefix with the prompt, overwrites the KV
    assert llm._kv_tokens == []                              # the prefix bookkeeping was reset
    again = llm.create_completion(TEXTS[0], **kw)["choices"][0]["text"]
    assert first == fresh and again == fresh


def test_cpu_tensor_parallel_refuses(paths):
    llm = _llm(paths["mean"], "cpu")
    llm._backend.tp_size = 2
    with pytest.raises(NotImplementedError, match="cpu"):
        llm.embed("hello")


# ----------------------------------------------------------------------------- POST /v1/embeddings (ENGINE=fake)
def _app(mode="echo", **kw):
    s = Settings()
    for k, v in kw.items():
        setattr(s, k, v)
    eng = FakeEngine(mode)
    return create_app(s, engine=eng), eng


def test_route_response_shape_usage_and_determinism():
    app, eng = _app()
    with TestClient(app) as c:
        r = c.post("/v1/embeddings", json={"input": ["one two", "three"], "model": "emb", "user": "u"})
        assert r.status_code == 200, r.text
        j = r.json()
        assert j["object"] == "list" and j["model"] == "emb"
        assert [e["index"] for e in j["data"]] == [0, 1] and all(e["object"] == "embedding" for e in j["data"])
        assert j["usage"]["prompt_tokens"] == j["usage"]["total_tokens"] == 3
        vecs = [np.asarray(e["embedding"]) for e in j["data"]]
        assert all(abs(np.linalg.norm(v) - 1) < 1e-6 for v in vecs) and rel_err(vecs[0], vecs[1]) > 0.1
        one = c.post("/v1/embeddings", json={"input": "one two"}).json()
        assert len(one["data"]) == 1 and np.allclose(one["data"][0]["embedding"], vecs[0])
        ids = c.post("/v1/embeddings", json={"input": [[1, 2, 3], [4]]}).json()
        assert len(ids["data"]) == 2 and ids["usage"]["total_tokens"] == 4
        assert len(c.post("/v1/embeddings", json={"input": [5, 6, 7]}).json()["data"]) == 1


def test_route_base64_and_dimensions():
    app, _ = _app()
    with TestClient(app) as c:
        f = c.post("/v1/embeddings", json={"input": "abc"}).json()["data"][0]["embedding"]
        b = c.post("/v1/embeddings", json={"input": "abc", "encoding_format": "base64"}).json()["data"][0]["embedding"]
        raw = base64.b64decode(b)
        assert len(raw) == 4 * len(f)
        assert list(struct.unpack(f"<{len(f)}f", raw)) == [float(np.float32(v)) for v in f]
        assert c.post("/v1/embeddings", json={"input": "abc", "dimensions": len(f)}).status_code == 200
        r = c.post("/v1/embeddings", json={"input": "abc", "dimensions": len(f) - 1})
        assert r.status_code == 400 and "dimensions" in r.json()["error"]["message"]
        assert c.post("/v1/embeddings", json={"input": "abc", "encoding_format": "hex"}).status_code == 400
        assert c.post("/v1/embeddings", json={"input": ""}).status_code == 400          # ValueError -> 400


def test_route_pooling_setting():
    """auto: the model's own pooling_type; absent or none: mean. An explicit setting wins."""
    class HP:
        pooling_type = -1

    app, eng = _app()
    with TestClient(app) as c:
        c.post("/v1/embeddings", json={"input": "abc"})
        assert eng.calls[-1]["pooling_type"] == 1          # the fake has no hparams at all: mean
        eng.hparams = HP()
        c.post("/v1/embeddings", json={"input": "abc"})
        assert eng.calls[-1]["pooling_type"] == 1          # key absent: mean
        HP.pooling_type = 0
        c.post("/v1/embeddings", json={"input": "abc"})
        assert eng.calls[-1]["pooling_type"] == 1          # none: mean (one vector per input)
        HP.pooling_type = 3
        c.post("/v1/embeddings", json={"input": "abc"})
        assert eng.calls[-1]["pooling_type"] == 3
    app, eng = _app(embedding_pooling="cls")
    eng.hparams = HP()
    with TestClient(app) as c:
        c.post("/v1/embeddings", json={"input": "abc"})
        assert eng.calls[-1]["pooling_type"] == 2


def test_setting_from_env(monkeypatch):
    assert Settings.from_env().embedding_pooling == "auto"
    monkeypatch.setenv("EMBEDDING_POOLING", "LAST")
    assert Settings.from_env().embedding_pooling == "last"
    monkeypatch.setenv("EMBEDDING_POOLING", "rank")
    with pytest.raises(ValueError):
        Settings.from_env()


def test_route_queue_full_503_and_timeout_408():
    async def burst(app, n):
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=60) as c:
                async def one(i):
                    await asyncio.sleep(0.01 * i)
                    return await c.post("/v1/embeddings", json={"input": f"text {i}"})
                return await asyncio.gather(*[one(i) for i in range(n)])
    app, _ = _app("sleep:0.2", timeout_seconds=20)
    codes = [r.status_code for r in asyncio.run(burst(app, 8))]
    assert codes.count(200) == 6 and codes.count(503) == 2, codes     # the same FIFO as the generation routes
    app, _ = _app("sleep:2", timeout_seconds=0.2)
    with TestClient(app) as c:
        assert c.post("/v1/embeddings", json={"input": "abc"}).status_code == 408


def test_route_engine_without_embeddings_is_400():
    class NoEmbed(FakeEngine):
        create_embedding = None

    app = create_app(Settings(), engine=NoEmbed("echo"))
    with TestClient(app) as c:
        assert c.post("/v1/embeddings", json={"input": "abc"}).status_code == 400


def test_facade_real_route(paths):
    """The route over the real facade (CPU backend): the server normalises and pools to one vector
    per input even where the model says none."""
    llm = _llm(paths["llama3"], "cpu")
    app = create_app(Settings(), engine=llm)
    with TestClient(app) as c:
        r = c.post("/v1/embeddings", json={"input": TEXTS[:2]})
        assert r.status_code == 200, r.text
        data = r.json()["data"]
    want = llm.embed(TEXTS[:2], normalize=True, pooling_type=1)
    assert len(data) == 2 and rel_err(data[0]["embedding"], want[0]) < 1e-6
    assert abs(np.linalg.norm(data[1]["embedding"]) - 1) < 1e-5


@pytest.mark.parametrize("backend", ["reference", "cpu"])
def test_token_ids_outside_the_vocabulary_are_refused(paths, backend):
    llm = _llm(paths["mean"], backend)
    for bad in ([1, 2, llm.n_vocab()], [[3], [-1, 4]]):
        with pytest.raises(ValueError, match="vocabulary"):
            llm.embed(bad)
    app = create_app(Settings(), engine=llm)
    with TestClient(app) as c:
        assert c.post("/v1/embeddings", json={"input": [[1, llm.n_vocab() + 5]]}).status_code == 400


def test_zero_vector_stays_zero_when_normalised():
    from llama_fastapi_k8s_gpu_amd.engine.pooling import pool_host
    rows = np.zeros((3, 8), np.float32)
    for pooling in (0, 1, 2, 3):
        assert (pool_host(rows, pooling, True) == 0).all()
