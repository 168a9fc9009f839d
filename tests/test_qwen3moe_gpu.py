"""Qwen3-MoE (tiny-qwen3moe: 128 experts, top-8) on the MI355X engine against the fp32 reference: prompt
chunk and greedy decode with and without batching, batched rows against single-row decode, the
plan's new FFN path, graph replay against eager."""
import numpy as np
import pytest

from gpu_helpers import rel_err
from test_qwen3_gpu import GREEDY, _engine, torch  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
SPEC = "tiny-qwen3moe"
TOKS = [int(t) for t in np.random.default_rng(0).integers(0, 16000, 39)]


@pytest.fixture(scope="module")
def model(tmp_path_factory, torch):
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    path = write_synthetic_gguf(SPEC, str(tmp_path_factory.mktemp("qwen3moe") / f"{SPEC}.gguf"), seed=3)
    return path, ReferenceLlama(GGUFReader(path), n_ctx=256)


def assert_router_margin(ref, toks, n_past=0):
    """Before anything is compared: at every position and layer the fp32 reference's 8th and 9th router
    logits are further apart than the bf16 rounding of the prompt path's router operands can move them.
    Both operands of a product n_i w_i are rounded (2^-9 each), so a logit moves by at most
    2^-8 sum_i |n_i w_i|; the tiny spec's router rows read ONE coordinate, so that sum is |logit| itself."""
    trace = []
    out = ref.forward(toks, n_past, router_trace=trace)
    k = ref.hp.n_expert_used
    assert len(trace) == ref.hp.n_layer
    for lg in trace:
        s = np.sort(lg.numpy().astype(np.float64), axis=1)[:, ::-1]
        gap, move = s[:, k - 1] - s[:, k], 2.0 ** -8 * (np.abs(s[:, k - 1]) + np.abs(s[:, k]))
        assert np.all(gap > move), ("router margin", float((gap / move).min()))
    return out.numpy()


@pytest.mark.parametrize("max_batch", [1, 4])
def test_engine_prefill_and_greedy_decode_match_reference(model, max_batch):
    path, ref = model
    eng = _engine(path, n_slots=max_batch)
    hp = eng.hparams
    assert hp["arch"] == "qwen3moe" and (hp["n_expert"], hp["n_expert_used"], hp["n_ff"]) == (128, 8, 256)
    assert hp["qk_norm"] is True and hp["rope_neox"] is True
    want = assert_router_margin(ref, TOKS)
    got = eng.eval_logits(TOKS, 0)
    assert rel_err(got, want) < 5e-2, ("prefill", rel_err(got, want))
    forced = []
    for i in range(39, 47):   # 8 greedy steps on the prefilled cache
        tok = int(np.argmax(got))
        forced.append(tok)
        want = assert_router_margin(ref, [tok], i)
        got = eng.decode_logits(tok, i)
        print("qwen3moe decode", max_batch, i, rel_err(got, want) / 5e-2)
        assert rel_err(got, want) < 5e-2, ("decode", i, rel_err(got, want))
    # graph replay == eager on ONE cache, over several replays of the captured step. Not bit for bit: the
    # single-row expert down (gemv_moe_down, reused as it is) adds its 8 slots' split-K partials with
    # float atomics, whose order differs between launches (measured 2.1e-7). The bound is the f32 sum's own
    # rounding, 2^-23 x (8 slots x up to 4 K parts + the residual) ~ 4e-6 of the row, taken as 1e-5.
    eager = _engine(path, n_slots=max_batch, graph=False)
    n = len(TOKS)
    eng.eval_logits(TOKS, 0)
    eager.kv_load(eng.kv_save(n), n)
    for i in range(8):
        a, b = eng.decode_logits(forced[i], n + i), eager.decode_logits(forced[i], n + i)
        assert rel_err(a, b) < 1e-5, ("graph vs eager decode step", i, rel_err(a, b))


def test_batch_rows_match_single_row_decode_on_the_grouped_plan(model):
    path, ref = model
    eng, one = _engine(path, n_slots=4), _engine(path, n_slots=1, graph=False)
    plan = eng.batch_plan(3)
    assert [p["ffn"] for p in plan] == ["moe_grouped"] * ref.hp.n_layer, plan
    rng = np.random.default_rng(3)
    slots, seqs, plen, rows = [3, 0, 1], {}, {}, {}
    for s, n in zip(slots, (5, 40, 17)):
        prompt = [int(t) for t in rng.integers(3, 300, n)]
        seqs[s], plen[s], rows[s] = prompt + [eng.slot_begin(s, prompt, 0, GREEDY)], n, []
    for _ in range(3):   # the captured step, replayed
        toks = eng.batch_step(slots)
        logits = eng.batch_logits(len(slots))
        for b, s in enumerate(slots):
            rows[s].append(np.array(logits[b]))
            assert toks[b] == int(np.argmax(logits[b]))
            seqs[s].append(toks[b])
    assert eng.healthy
    for s in slots:
        want = assert_router_margin(ref, seqs[s][:plen[s] + 3])
        assert rel_err(rows[s][2], want) < 5e-2, (s, rel_err(rows[s][2], want))
        one.eval_logits(seqs[s][:plen[s]], 0)
        for j in range(3):
            i = plen[s] + j
            e = rel_err(rows[s][j], one.decode_logits(seqs[s][i], i))
            assert e < 1.5e-2, (s, j, e)   # test_batch_gpu.TIGHT


def test_other_wide_files_the_kernels_decline_keep_the_old_path(tmp_path, torch):  # noqa: F811
    """32 experts under general.architecture llama with an expert width of 576 (no multiple of 256): the wide
    kernels decline it, so it loads and runs on the few-expert paths as before (plan value grouped)."""
    from dataclasses import replace
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    spec = replace(SPECS["tiny-q8-oddff"], name="moe32-oddff", n_expert=32, n_expert_used=2)
    path = write_synthetic_gguf(spec, str(tmp_path / "moe32.gguf"), seed=3)
    eng = _engine(path, n_slots=4)
    assert [p["ffn"] for p in eng.batch_plan(3)] == ["grouped"] * spec.n_layer
    toks = [int(t) for t in np.random.default_rng(0).integers(3, 300, 20)]
    want = ReferenceLlama(GGUFReader(path), n_ctx=256).forward(toks, 0).numpy()
    assert rel_err(eng.eval_logits(toks, 0), want) < 5e-2
