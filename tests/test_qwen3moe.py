"""Qwen3-MoE without a GPU: the hparams read, the CPU backend against the fp32 reference on the same
file, and the refusals (tensor parallelism; tests/test_qwen3.py pins the file without experts)."""
import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
from llama_fastapi_k8s_gpu_amd.models.llama import LlamaHParams, ReferenceLlama
from llama_fastapi_k8s_gpu_amd.runtime import load_cpu


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    return write_synthetic_gguf("tiny-qwen3moe", str(tmp_path_factory.mktemp("qwen3moe") / "m.gguf"), seed=3)


def test_hparams(path, tmp_path, monkeypatch):
    md = GGUFReader(path).metadata
    hp = LlamaHParams.from_metadata(md)
    assert md["qwen3moe.feed_forward_length"] == 2048      # the dense size: not the experts'
    assert (hp.arch, hp.n_expert, hp.n_expert_used, hp.n_ff, hp.head_dim, hp.rope_neox) == ("qwen3moe", 128, 8, 256, 64, True)
    eng = load_cpu().CpuEngine(path, n_ctx=32, n_threads=2)
    h = eng.hparams
    assert (h["arch"], h["n_expert"], h["n_expert_used"], h["n_ff"], h["qk_norm"]) == ("qwen3moe", 128, 8, 256, True)
    # without the key the experts' width is the tensor's shape
    import llama_fastapi_k8s_gpu_amd.gguf.synthetic as S
    orig = S.hparams_metadata
    monkeypatch.setattr(S, "hparams_metadata",
                        lambda spec, nv: {k: v for k, v in orig(spec, nv).items() if "expert_feed" not in k})
    p2 = write_synthetic_gguf("tiny-qwen3moe", str(tmp_path / "nokey.gguf"), seed=3)
    assert load_cpu().CpuEngine(p2, n_ctx=32, n_threads=2).hparams["n_ff"] == 256
    assert ReferenceLlama(GGUFReader(p2), n_ctx=32).hp.n_ff == 256


def test_cpu_backend_matches_reference(path):
    ref = ReferenceLlama(GGUFReader(path), n_ctx=64)
    eng = load_cpu().CpuEngine(path, n_ctx=64, n_threads=4)
    toks = [int(t) for t in np.random.default_rng(1).integers(0, ref.hp.n_vocab, 12)]
    want, got = ref.forward(toks, 0).numpy(), np.asarray(eng.eval_logits(toks, 0))
    e = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert e < 5e-2, e


def test_tensor_parallelism_and_layer_split_refused(path):
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    for kw in (dict(backend="hip", split_mode="row", tensor_split=[1, 1]), dict(backend="layer", tensor_split=[1, 1])):
        with pytest.raises(NotImplementedError, match="qwen3moe"):
            Llama(path, n_gpu_layers=-1, n_ctx=32, verbose=False, **kw)
