"""Qwen2 / Qwen2.5 GGUF models on the CPU side: loader, hyper-parameters, the NeoX-RoPE row
permutation, the Q|K|V biases, tensor parallelism, tied output head, tokenizer and chat format.

The Python fp32 reference rotates NeoX pairs (i, i + head_dim/2) on the file's own weight rows; the
C++ CPU backend permutes the q / k rows inside each head at load and rotates adjacent pairs, as the
GPU engine does. That the two agree is the check of the permutation argument (docs/DESIGN.md).
"""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from llama_fastapi_k8s_gpu_amd.engine.chat_format import guess_chat_format
from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
from llama_fastapi_k8s_gpu_amd.engine.tokenizer import tokenizer_from_metadata
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, build_vocab, qkv_bias_std, write_synthetic_gguf
from llama_fastapi_k8s_gpu_amd.models.llama import LlamaHParams, ReferenceLlama
from llama_fastapi_k8s_gpu_amd.runtime import load_cpu

MODELS = ["tiny-qwen2-g7", "tiny-qwen2-g6-hd64"]
BOUND = 0.06   # tests/test_cpu_backend.py: the CPU backend (q8 activations, f16 KV) vs the fp32 reference


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-12))


TOKS = [int(t) for t in np.random.default_rng(1).integers(3, 500, 20)]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("qwen2_models")
    return {m: write_synthetic_gguf(m, str(d / f"{m}.gguf")) for m in MODELS}


@pytest.fixture(scope="module")
def refs(paths):
    """fp32 reference logits per model: prefill of TOKS and one decode step on top (computed once)."""
    out = {}
    for m, p in paths.items():
        ref = ReferenceLlama(GGUFReader(p), n_ctx=64)
        out[m] = (ref.forward(TOKS, 0).numpy(), ref.forward([7], len(TOKS)).numpy())
    return out


def test_gguf_round_trip_and_hparams(paths):
    spec = SPECS["tiny-qwen2-g7"]
    rd = GGUFReader(paths["tiny-qwen2-g7"])
    md = rd.metadata
    assert md["general.architecture"] == "qwen2"
    assert "qwen2.rope.dimension_count" not in md and not any(k.startswith("llama.") for k in md)
    assert md["tokenizer.ggml.pre"] == "qwen2" and md["tokenizer.ggml.add_bos_token"] is False
    for name, n in (("attn_q", spec.n_embd), ("attn_k", 256), ("attn_v", 256)):
        b = rd.dequant(f"blk.1.{name}.bias")
        assert b.dtype == np.float32 and b.size == n
    # real Qwen2 biases are large: at least the projection's own output on a normed input
    assert np.std(rd.dequant("blk.0.attn_q.bias")) > 0.9 * qkv_bias_std(spec) >= spec.weight_std * np.sqrt(spec.n_embd)
    hp = LlamaHParams.from_metadata(md)
    assert (hp.arch, hp.rope_neox, hp.head_dim, hp.gqa) == ("qwen2", True, 128, 7)
    assert hp.rope_base == 1e6 and hp.rms_eps == pytest.approx(1e-6)
    # the C++ reader (shared by the GPU engine and the CPU backend)
    h = load_cpu().CpuEngine(paths["tiny-qwen2-g7"], n_ctx=32, n_threads=2).hparams
    assert h["arch"] == "qwen2" and h["rope_neox"] is True and h["qkv_bias"] is True
    assert (h["n_head"], h["n_head_kv"], h["head_dim"], h["n_embd"]) == (14, 2, 128, 1792)
    assert h["rope_base"] == 1e6 and h["rms_eps"] == pytest.approx(1e-6)


def test_llama_files_report_no_flags(tmp_path):
    p = write_synthetic_gguf("tiny-llama3-f32", str(tmp_path / "l.gguf"))
    h = load_cpu().CpuEngine(p, n_ctx=32, n_threads=2).hparams
    assert h["arch"] == "llama" and h["rope_neox"] is False and h["qkv_bias"] is False


def test_partial_biases_and_rope_scaling_are_refused(tmp_path):
    cpu = load_cpu()
    spec = "tiny-qwen2-g6-hd64"
    p = write_synthetic_gguf(spec, str(tmp_path / "qonly.gguf"),
                             skip_tensors=("blk.1.attn_k.bias", "blk.1.attn_v.bias"))
    with pytest.raises(RuntimeError, match=r"blk\.1\.attn_k\.bias"):
        cpu.CpuEngine(p, n_ctx=32, n_threads=2)
    with pytest.raises(ValueError, match=r"blk\.1\.attn_q\.bias"):
        ReferenceLlama(GGUFReader(p), n_ctx=32)
    p = write_synthetic_gguf(spec, str(tmp_path / "yarn.gguf"), extra_metadata={"qwen2.rope.scaling.type": "yarn"})
    with pytest.raises(RuntimeError, match=r"qwen2\.rope\.scaling\.type"):
        cpu.CpuEngine(p, n_ctx=32, n_threads=2)
    with pytest.raises(NotImplementedError, match=r"qwen2\.rope\.scaling\.type"):
        LlamaHParams.from_metadata(GGUFReader(p).metadata)
    p = write_synthetic_gguf(spec, str(tmp_path / "none.gguf"), extra_metadata={"qwen2.rope.scaling.type": "none"})
    assert cpu.CpuEngine(p, n_ctx=32, n_threads=2).hparams["arch"] == "qwen2"
    # a file with no biases at all loads, with the flag off
    nob = tuple(f"blk.{l}.attn_{x}.bias" for l in range(2) for x in "qkv")
    p = write_synthetic_gguf(spec, str(tmp_path / "nobias.gguf"), skip_tensors=nob)
    assert cpu.CpuEngine(p, n_ctx=32, n_threads=2).hparams["qkv_bias"] is False


@pytest.mark.parametrize("model", MODELS)
def test_permuted_rows_equal_neox_rope(paths, refs, model):
    want, want2 = refs[model]
    eng = load_cpu().CpuEngine(paths[model], n_ctx=64, n_threads=4, n_batch=8)   # 20 tokens = 3 batches
    got = eng.eval_logits(TOKS, 0)
    got2 = eng.eval_logits([7], len(TOKS))
    assert got.shape == want.shape
    assert _rel(got, want) < BOUND, _rel(got, want)
    assert _rel(got2, want2) < BOUND, _rel(got2, want2)
    # the same weights under adjacent-pair RoPE are a different model: the bound tells them apart
    adj = ReferenceLlama(GGUFReader(paths[model]), n_ctx=64, rope_neox=False)
    assert _rel(got, adj.forward(TOKS, 0).numpy()) > BOUND
    assert _rel(got2, adj.forward([7], len(TOKS)).numpy()) > BOUND


@pytest.mark.parametrize("model", MODELS)
def test_a_dropped_bias_is_far_outside_the_bound(paths, refs, model):
    want, want2 = refs[model]
    nob = ReferenceLlama(GGUFReader(paths[model]), n_ctx=64, qkv_bias=False)
    assert not nob.hp.qkv_bias
    e1, e2 = _rel(nob.forward(TOKS, 0).numpy(), want), _rel(nob.forward([7], len(TOKS)).numpy(), want2)
    assert e1 > 10 * BOUND and e2 > 10 * BOUND, (e1, e2)


def test_tied_output_equals_explicit_output_weight(tmp_path, paths, refs):
    m = "tiny-qwen2-g6-hd64"
    assert "output.weight" not in GGUFReader(paths[m]).tensors
    untied = write_synthetic_gguf(m, str(tmp_path / "untied.gguf"), untie_output=True)
    rd = GGUFReader(untied)
    assert np.array_equal(np.asarray(rd.raw("output.weight")), np.asarray(rd.raw("token_embd.weight")))
    cpu = load_cpu()
    a = cpu.CpuEngine(paths[m], n_ctx=64, n_threads=4, n_batch=8).eval_logits(TOKS, 0)
    b = cpu.CpuEngine(untied, n_ctx=64, n_threads=4, n_batch=8).eval_logits(TOKS, 0)
    assert np.array_equal(a, b)
    assert _rel(ReferenceLlama(rd, n_ctx=64).forward(TOKS, 0).numpy(), refs[m][0]) == 0.0


# ---------------------------------------------------------------- tensor parallelism (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, path, tokens, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from llama_fastapi_k8s_gpu_amd.parallel.comm import host_collectives
        eng = load_cpu().CpuEngine(path, n_ctx=64, n_threads=2, n_batch=8, tp_rank=rank, tp_size=world)
        eng.set_comm(*host_collectives())
        np.save(os.path.join(out_dir, f"r{rank}_a.npy"), eng.eval_logits(tokens, 0))
        np.save(os.path.join(out_dir, f"r{rank}_b.npy"), eng.eval_logits([5], len(tokens)))
    finally:
        dist.destroy_process_group()


def test_tp2_matches_tp1(tmp_path):
    path = write_synthetic_gguf("tiny-qwen2-tp", str(tmp_path / "tp.gguf"))
    tokens = [int(t) for t in np.random.default_rng(0).integers(3, 400, 12)]
    ref = load_cpu().CpuEngine(path, n_ctx=64, n_threads=2, n_batch=8)
    want_a = ref.eval_logits(tokens, 0)
    want_b = ref.eval_logits([5], len(tokens))
    mp.start_processes(_rank_main, args=(2, _free_port(), path, tokens, str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    for r in range(2):
        for got, want in ((np.load(tmp_path / f"r{r}_a.npy"), want_a), (np.load(tmp_path / f"r{r}_b.npy"), want_b)):
            assert got.shape == want.shape
            assert np.linalg.norm(got - want) / np.linalg.norm(want) < 5e-3   # tests/test_tensor_parallel.py
            assert int(np.argmax(got)) == int(np.argmax(want))


# ---------------------------------------------------------------- tokenizer and facade
def _tok(pre, **md_extra):
    md, _ = build_vocab(SPECS["tiny-qwen2-g7"])
    md = dict(md, **{"tokenizer.ggml.pre": pre}, **md_extra)
    return tokenizer_from_metadata(md)


def test_qwen2_pretokenizer_digits_contractions_and_bos():
    text = "abc1234 I'M"
    q = _tok("qwen2")
    pieces = [m.group(0) for m in q.pre_re.finditer(text)]
    assert pieces == ["abc", "1", "2", "3", "4", " I", "'M"]
    md, _ = build_vocab(SPECS["tiny-qwen2-g7"])
    md = {k: v for k, v in md.items() if k != "tokenizer.ggml.add_bos_token"}
    l3 = tokenizer_from_metadata(dict(md, **{"tokenizer.ggml.pre": "llama-bpe"}))
    assert [m.group(0) for m in l3.pre_re.finditer(text)] == ["abc", "123", "4", " I", "'M"]
    # no BOS: the file says add_bos_token = false; for pre = qwen2 an absent key means the same
    ids = q.encode(text, add_bos=True)
    assert ids and ids[0] != q.bos_id and ids == q.encode(text, add_bos=False)
    assert q.decode(ids) == text
    q2 = tokenizer_from_metadata(dict(md, **{"tokenizer.ggml.pre": "qwen2"}))
    assert q2.encode(text, add_bos=True) == ids
    assert l3.encode(text, add_bos=True)[0] == l3.bos_id   # llama-bpe, key absent: BOS as before
    # both end-of-generation tokens, whatever the file's eos id is
    for name in ("<|im_end|>", "<|endoftext|>"):
        assert q.is_eog(q.tokens.index(name))
    assert q.eos_id == q.tokens.index("<|im_end|>")


def test_add_bos_token_false_is_honoured_by_both_tokenizers():
    """The key is the file's word for BPE and SPM vocabularies alike; absent, both add the BOS."""
    md, _ = build_vocab(SPECS["tiny-tinyllama-q8_0"])
    spm = tokenizer_from_metadata(md)
    assert spm.encode("hello", add_bos=True)[0] == spm.bos_id
    absent = tokenizer_from_metadata({k: v for k, v in md.items() if k != "tokenizer.ggml.add_bos_token"})
    assert absent.encode("hello", add_bos=True) == spm.encode("hello", add_bos=True)
    off = tokenizer_from_metadata(dict(md, **{"tokenizer.ggml.add_bos_token": False}))
    assert off.encode("hello", add_bos=True) == spm.encode("hello", add_bos=False)
    bpe_md, _ = build_vocab(SPECS["tiny-llama3-q4_k_m"])
    bpe_off = tokenizer_from_metadata(dict(bpe_md, **{"tokenizer.ggml.add_bos_token": False}))
    assert bpe_off.encode("hello", add_bos=True) == bpe_off.encode("hello", add_bos=False)


def test_both_eog_tokens_stop_a_cpu_generation(paths):
    llm = Llama(paths["tiny-qwen2-g6-hd64"], n_ctx=128, backend="cpu", seed=0, n_threads=2, verbose=False)
    assert llm.chat_format == "chatml"
    assert llm.tokenize(b"hello", add_bos=True) == llm.tokenize(b"hello", add_bos=False)
    free = llm.create_completion("hello world", max_tokens=6, temperature=0.0)
    assert free["usage"]["completion_tokens"] == 6 or free["choices"][0]["finish_reason"] == "stop"
    for name in ("<|im_end|>", "<|endoftext|>"):
        tid = llm.tokenizer.tokens.index(name)
        out = llm.create_completion("hello world", max_tokens=6, temperature=0.0, logit_bias={tid: 1e4})
        c = out["choices"][0]
        assert c["finish_reason"] == "stop" and c["text"] == "", (name, c)
        assert out["usage"]["completion_tokens"] <= 1


def test_long_unknown_template_on_a_qwen2_file_is_chatml():
    md, _ = build_vocab(SPECS["tiny-qwen2-g7"])
    assert guess_chat_format(dict(md, **{"general.architecture": "qwen2"})) == "chatml"
    long_tmpl = ("{%- if tools %}{{- '<|im_start|>system\\n' }}{{- '# Tools\\n\\nYou may call one or more functions' }}"
                 "{%- endif %}" + md["tokenizer.chat_template"])
    assert guess_chat_format({"general.architecture": "qwen2", "tokenizer.chat_template": long_tmpl}) == "chatml"
    # other architectures keep rendering an unknown template with Jinja2
    assert guess_chat_format({"general.architecture": "llama", "tokenizer.chat_template": long_tmpl}) is None
