"""Engine.batch_plan against configuration: the path every layer of a batched decode step takes
(BatchLayerPlan, docs/DESIGN.md) is what the bindings' own predicates answer for that layer's types
and shapes - so the plan and the launchers cannot disagree, and a predicate that moves a model to
another path moves these expectations with it. No step runs here: the engines only load."""
import pytest

from gpu_helpers import dense_ffn_path, hip

pytestmark = pytest.mark.gpu

SPECS = ["pd-llama-g4", "tiny-mixtral-d4k", "tiny-q8-1l", "tiny-llama3-q4_k_m"]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    d = tmp_path_factory.mktemp("plan_models")
    return {s: write_synthetic_gguf(s, str(d / f"{s}.gguf")) for s in SPECS}


def _engine(path, n_slots=4):
    return hip().Engine(path, n_ctx=128, n_batch=64, device=0, use_graph=True, n_slots=n_slots)


def _tensors(path):
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    return GGUFReader(path).tensors


def _check_qkv(path, plan, B, split_k_on=True):
    """split_k exactly where bmm_qkv_sk_supported takes the layer's types (no biases, no QK-norm here);
    else the epilogue where B rows of this width fit one part, else the unfused form."""
    t = _tensors(path)
    for l, p in enumerate(plan):
        q, k, v = (t[f"blk.{l}.attn_{x}.weight"] for x in "qkv")
        d = q.shape[0]
        sk = split_k_on and hip().bmm_qkv_sk_supported(int(q.ggml_type), int(k.ggml_type), int(v.ggml_type), d, B)
        fits = B <= 16 and hip().bmm_qkv_fits(d, B)
        want = ("split_k", "none") if sk else ("epilogue", "none") if fits else ("unfused", "rope_kv_prefill")
        assert (p["qkv"], p["finish"]) == want, (B, l, p)
        assert p["qkv_norm_folded"] == (sk or (fits and hip().bmm_norm_fits(d, B))), (B, l, p)
        assert p["zero_qkv"] == ("nobody" if not sk else "memset" if p["ffn"] == "grouped" else "down"), (B, l, p)
        assert p["tp"] == "none" and p["wo_rows"] == (B > 16), (B, l, p)


@pytest.mark.parametrize("chain", [None, "1", "2", "0"])
def test_dense_ffn_follows_the_chain_predicates(models, chain, monkeypatch):
    """pd-llama-g4 (d = 4096, Q4_K_M) at B = 3 under LFK_FFN_CHAIN unset (level 1) / 1 / 2 / 0: each
    layer's Wo + FFN path is the first of wo_ffn_chain (level 2) / ffn_chain (level >= 1) / swiglu that
    the bindings' predicates take for its types and shapes (gpu_helpers.dense_ffn_path)."""
    if chain is None:
        monkeypatch.delenv("LFK_FFN_CHAIN", raising=False)
    else:
        monkeypatch.setenv("LFK_FFN_CHAIN", chain)
    path = models["pd-llama-g4"]
    plan = _engine(path).batch_plan(3)
    assert len(plan) == 4
    for l, p in enumerate(plan):
        assert p["ffn"] == dense_ffn_path(path, l, 3, chain=int(chain or 1)), (chain, l, p)
        assert p["ffn_norm_folded"] == hip().bmm_norm_fits(4096, 3), (chain, l, p)
    if chain == "0":
        assert all(p["ffn"] == "swiglu" for p in plan), plan
    _check_qkv(path, plan, 3)


def test_moe_takes_the_stacked_experts(models):
    """tiny-mixtral-d4k: one stacked gate/up and one K-concatenated down where the expert types have
    tile16 copies and the rows fit one part (the engine's stacked-expert setup), else the grouped FFN."""
    path = models["tiny-mixtral-d4k"]
    t = _tensors(path)
    gate, down = t["blk.0.ffn_gate_exps.weight"], t["blk.0.ffn_down_exps.weight"]
    d, F = gate.shape[0], gate.shape[1]
    eng = _engine(path)
    for B in (2, 3, 4):
        stacked = (hip().bmm_supported(int(gate.ggml_type), d) and hip().bmm_supported(int(down.ggml_type), F) and
                   F % 256 == 0 and hip().bmm_qkv_fits(d, B))
        plan = eng.batch_plan(B)
        for p in plan:
            assert p["ffn"] == ("moe_stacked" if stacked else "grouped"), (B, p)
            assert p["ffn_norm_folded"] == (stacked and hip().bmm_norm_fits(d, B)), (B, p)
        _check_qkv(path, plan, B)


def test_q8_0_gate_up_declines_the_chains(models):
    """tiny-q8-1l: the chains take Q4_K-format gate/up only, so a Q8_0 layer runs gate/up and down as
    separate launches on the SwiGLU epilogue - whatever bmm_ffn_chain_supported says for its types."""
    from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
    path = models["tiny-q8-1l"]
    t = _tensors(path)
    gate, down = t["blk.0.ffn_gate.weight"], t["blk.0.ffn_down.weight"]
    assert gate.ggml_type == GGMLType.Q8_0
    eng = _engine(path)
    assert eng.batch_gemv == 2
    for B in (2, 3):
        takes = hip().bmm_ffn_chain_supported(int(gate.ggml_type), down.shape[0], gate.shape[0], int(down.ggml_type), B,
                                              hip().bmm_norm_fits(gate.shape[0], B))
        assert not takes
        (p,) = eng.batch_plan(B)
        assert p["ffn"] == "swiglu" == dense_ffn_path(path, 0, B), (B, p)
        _check_qkv(path, [p], B)


@pytest.mark.parametrize("B", [9, 16])
def test_more_than_eight_rows_never_split_k(models, B):
    """Past 8 rows the split-K Q|K|V declines (bmm_qkv_sk_supported) on every layer, and the chains
    with it (they take at most 8 rows): the one-part epilogue and the separate SwiGLU launches."""
    path = models["tiny-llama3-q4_k_m"]
    t = _tensors(path)
    eng = _engine(path, n_slots=16)
    assert eng.max_batch == 16 and eng.batch_gemv == 2
    plan = eng.batch_plan(B)
    for l, p in enumerate(plan):
        types = [int(t[f"blk.{l}.attn_{x}.weight"].ggml_type) for x in "qkv"]
        assert not hip().bmm_qkv_sk_supported(*types, t["blk.0.attn_q.weight"].shape[0], B)
        assert p["qkv"] != "split_k" and p["zero_qkv"] == "nobody", (B, l, p)
        assert p["ffn"] == "swiglu" == dense_ffn_path(path, l, B), (B, l, p)
    _check_qkv(path, plan, B)
    with pytest.raises(RuntimeError, match="batch_plan"):
        eng.batch_plan(17)
