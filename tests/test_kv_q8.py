"""``Llama(type_k=, type_v=)`` where no GPU is needed: the values the facade refuses, the backends that
keep an f16 cache, and the ``KV_TYPE`` setting. The MI355X engine's route is tests/test_kv_q8_engine_gpu.py."""
import pytest

from llama_fastapi_k8s_gpu_amd.config import Settings
from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    return write_synthetic_gguf("tiny-llama3-q4_k_m", str(tmp_path_factory.mktemp("kv_q8_models") / "m.gguf"))


@pytest.mark.parametrize("backend", ["reference", "cpu"])
def test_backends_without_a_quantised_cache_refuse(path, backend):
    kw = dict(n_ctx=32, backend=backend, n_threads=2, verbose=False)
    with pytest.raises(NotImplementedError, match=f"q8_0.*{backend}"):
        Llama(path, type_k=8, type_v=8, **kw)
    assert Llama(path, type_k=1, type_v=None, **kw).backend_name == backend   # 1 and None both mean f16


@pytest.mark.parametrize("kw,words", [({"type_k": 8, "type_v": 1}, "type_k=8 and type_v=1"),
                                      ({"type_k": 8}, "type_k=8 and type_v=None"),
                                      ({"type_k": 2}, "type_k=2"), ({"type_v": 0, "type_k": 8}, "type_v=0")])
def test_values_the_facade_refuses(path, kw, words):
    with pytest.raises(ValueError, match=words):
        Llama(path, n_ctx=32, backend="reference", verbose=False, **kw)


def test_setting_from_env(monkeypatch):
    from llama_fastapi_k8s_gpu_amd.engine import factory
    assert Settings.from_env().kv_type == "f16"
    seen = {}
    monkeypatch.setattr("llama_fastapi_k8s_gpu_amd.engine.llama.Llama", lambda **kw: seen.update(kw))
    factory.build_engine(Settings.from_env())
    assert "type_k" not in seen and "type_v" not in seen
    monkeypatch.setenv("KV_TYPE", "Q8_0")
    s = Settings.from_env()
    assert s.kv_type == "q8_0"
    factory.build_engine(s)
    assert (seen["type_k"], seen["type_v"]) == (8, 8)
    monkeypatch.setenv("KV_TYPE", "q4_0")
    with pytest.raises(ValueError, match="KV_TYPE"):
        Settings.from_env()
