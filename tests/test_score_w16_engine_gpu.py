"""``Engine.score`` on files whose output head is a BF16 or F16 matrix (score_head_w16: the head as
uploaded, no tile16 copy) against the fp32 reference model with log_softmax in fp64. Bounds, inputs
and structure are test_score_engine_gpu.py's: ``rel_err < 5e-2`` and the best-id slack."""
import numpy as np
import pytest

from gpu_helpers import rel_err
from test_score_engine_gpu import INPUTS, check, engine

pytestmark = pytest.mark.gpu

SPECS = ["tiny-llama-bf16", "tiny-qwen3-bf16", "tiny-llama-f16"]   # (qwen3: a tied BF16 head, the token embedding)
_BUILT = {}


def model_ref(spec, tmp_path_factory):
    """(path, per input the reference's records and fp64 logits), built once per spec."""
    if spec not in _BUILT:
        from llama_fastapi_k8s_gpu_amd.engine.backends import ReferenceBackend
        from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
        from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
        path = write_synthetic_gguf(spec, str(tmp_path_factory.mktemp("score_w16_models") / f"{spec}.gguf"))
        be = ReferenceBackend(GGUFReader(path), 256)
        rows = [np.asarray(r, np.float64) for r in be.score(INPUTS)]
        logits = [be.model.forward(list(toks), 0, all_logits=True).numpy().astype(np.float64) for toks in INPUTS]
        _BUILT[spec] = path, list(zip(rows, logits))
    return _BUILT[spec]


@pytest.mark.parametrize("spec", SPECS)
def test_packed_and_alone_against_reference(spec, tmp_path_factory, monkeypatch):
    """Four slots, packed 32-row chunks: three inputs in one call; each alone; a one-slot engine."""
    model, ref = model_ref(spec, tmp_path_factory)
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
    print(f"test_score_w16_engine_gpu {spec}: vs reference / 5e-2 = {worst[0]:.3f}")
    assert eng4.healthy and eng1.healthy


def test_facade_echo_logprobs(tmp_path_factory):
    """logits_all=True on a BF16 file: echoed prompt tokens but the first carry Llama.score's log-probabilities."""
    from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
    model, ref = model_ref("tiny-llama-bf16", tmp_path_factory)
    toks, n = INPUTS[0], len(INPUTS[0])
    llm = Llama(model, logits_all=True, n_gpu_layers=-1, n_ctx=256, n_batch=32, seed=1, verbose=False)
    try:
        a = llm.create_completion(toks, max_tokens=4, temperature=0.0, top_k=1, repeat_penalty=1.0, echo=True,
                                  logprobs=1)["choices"][0]["logprobs"]
        assert a["token_logprobs"][0] is None and None not in a["token_logprobs"][1:]
        sc = llm.score(toks)
        assert sc["token_logprobs"][1:] == a["token_logprobs"][1:n] and sc["token_logprobs"][0] is None
        assert rel_err(sc["token_logprobs"][1:], ref[0][0][:-1, 0]) < 5e-2
    finally:
        llm.close()
