"""BF16 GGUF models on the MI355X engine: prefill (gemm_bf16w's 64-token tile), single-row decode
(the f32-activation GEMV launches), batched rows (gemm_bf16w's narrow tile through the rows path)
and embeddings against the fp32 torch reference, at the bounds tests/test_engine_gpu.py gives F16
and quantised models: 5e-2 of the logits' norm, greedy tokens equal or apart only at a near-tie."""
import numpy as np
import pytest

from gpu_helpers import rel_err
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf

pytestmark = pytest.mark.gpu
SPECS = ["tiny-llama-bf16", "tiny-qwen3-bf16"]
GREEDY = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("bf16_models")
    return {s: write_synthetic_gguf(s, str(d / f"{s}.gguf"), seed=3) for s in SPECS}


def _near_tie(got, want):
    return np.argmax(got) == np.argmax(want) or want[np.argmax(got)] > want.max() - 0.05 * np.abs(want).max()


@pytest.mark.parametrize("max_batch", [1, 4])
@pytest.mark.parametrize("spec", SPECS)
def test_bf16_model_matches_reference(models, spec, max_batch):
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    path = models[spec]
    ref = ReferenceLlama(GGUFReader(path), n_ctx=256)
    eng = load_hip().Engine(path, n_ctx=256, n_batch=64, device=0, use_graph=True, n_slots=max_batch)
    assert not eng.prefill_t16
    toks = [int(t) for t in np.random.default_rng(0).integers(3, 300, 44)]
    assert rel_err(eng.eval_logits(toks[:39], 0), ref.forward(toks[:39], 0).numpy()) < 5e-2, spec
    for i in range(39, 44):   # graph-replayed single-row decode on the prefilled cache
        want, got = ref.forward([toks[i]], i).numpy(), eng.decode_logits(toks[i], i)
        assert rel_err(got, want) < 5e-2 and _near_tie(got, want), (spec, i, rel_err(got, want))
    if max_batch > 1:   # three rows at different lengths through the rows path, greedy
        seqs = {s: toks[:n] for s, n in ((2, 5), (0, 40), (1, 17))}
        for s in seqs:
            seqs[s] = seqs[s] + [eng.slot_begin(s, seqs[s], 0, GREEDY)]
        for step in range(3):
            out, logits = eng.batch_step(list(seqs)), eng.batch_logits(3)
            for b, s in enumerate(seqs):
                want = ref.forward(seqs[s], 0).numpy()
                assert rel_err(logits[b], want) < 5e-2 and _near_tie(logits[b], want), (spec, step, s)
                assert out[b] == int(np.argmax(logits[b]))
                seqs[s].append(out[b])
    assert eng.healthy, eng.last_error


def test_bf16_graph_equals_eager(models):
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    outs = []
    for graph in (True, False):
        eng = load_hip().Engine(models[SPECS[0]], n_ctx=256, n_batch=128, device=0, use_graph=graph)
        outs.append(eng.generate([1, 2, 3, 4, 5], 0, 40, {"temperature": 1.0, "top_k": 40, "top_p": 0.95, "seed": 7},
                                 [], None, None)["tokens"])
    assert outs[0] == outs[1] and len(outs[0]) == 40


def test_bf16_llama_embed(models):
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    from llama_fastapi_k8s_gpu_amd.engine.pooling import pool_host
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    toks = [7, 8, 9] * 6
    llm = Llama(models[SPECS[0]], n_gpu_layers=-1, n_ctx=256, n_batch=64, verbose=False, max_batch=4)
    got = np.asarray(llm.embed(toks, pooling_type=1), np.float32)
    rows = ReferenceLlama(GGUFReader(models[SPECS[0]]), n_ctx=256).hidden(toks).numpy().astype(np.float64)
    assert rel_err(got, pool_host(rows, 1, False, np.float64)) < 5e-2
