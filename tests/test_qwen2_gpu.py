"""Qwen2 / Qwen2.5 on the MI355X engine: the kernels' new ground (GQA groups 3, 5, 6, 7 in the
decode attention and the MFMA prefill attention, Q|K|V biases in the single-row QKV kernel) against
fp64, and the engine on the tiny Qwen2 specs (NeoX RoPE by row permutation, biases at every site
that finishes a Q|K|V sum) against the fp32 reference, which rotates NeoX pairs on the file's own rows.

Forms and bounds are those of tests/test_kernels_gpu.py, test_engine_gpu.py, test_batch_gpu.py and
test_tp_gpu.py for the Llama specs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_helpers import dev_bytes, hip, make_matrix, q8_emulate, rel_err, rmsnorm, stream, to_planar
from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_SPECS = ["tiny-qwen2-g7", "tiny-qwen2-g6-hd64", "tiny-qwen2-g5", "tiny-qwen2-d896"]
TIGHT = 1.5e-2   # test_engine_gpu.TIGHT / test_batch_gpu.TIGHT for tiny-llama3-q4_k_m
GREEDY = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def models(tmp_path_factory, torch):
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    d = tmp_path_factory.mktemp("qwen2_gpu_models")
    return {s: write_synthetic_gguf(s, str(d / f"{s}.gguf"), seed=3) for s in ENGINE_SPECS}


# ---------------------------------------------------------------- kernels
def _attn_ref(q, K, V, L, scale):
    # q [H, D], K/V [Hkv, n_ctx, D]
    H, D = q.shape
    G = H // K.shape[0]
    out = np.zeros((H, D))
    for h in range(H):
        k = K[h // G, :L].astype(np.float64)
        s = k @ q[h].astype(np.float64) * scale
        p = np.exp(s - s.max())
        p /= p.sum()
        out[h] = p @ V[h // G, :L].astype(np.float64)
    return out


def _swizzle4(x):
    """bmm's k order inside each 4-group: (0, 2, 1, 3)."""
    return x.reshape(*x.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(x.shape)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("G", [3, 5, 6, 7])
@pytest.mark.parametrize("L", [1, 65, 1000])
def test_attn_decode_groups(torch, hd, G, L):
    rng = np.random.default_rng(L + hd + G)
    n_ctx, Hkv = 1024, 2
    H = G * Hkv
    q = rng.standard_normal((H, hd)).astype(np.float32)
    K = rng.standard_normal((Hkv, n_ctx, hd)).astype(np.float16)
    V = rng.standard_normal((Hkv, n_ctx, hd)).astype(np.float16)
    dq, dK, dV = (torch.from_numpy(a).cuda() for a in (q, K, V))
    pos = torch.tensor([L - 1], dtype=torch.int32, device="cuda")
    ws = torch.zeros(hip().attn_decode_workspace_floats(n_ctx, H, hd), device="cuda")
    out = torch.zeros(H, hd, device="cuda")
    cnt = torch.zeros(64, dtype=torch.int32, device="cuda")
    scale = 1 / np.sqrt(hd)
    ref = _attn_ref(q, K, V, L, scale)
    for _ in range(3):  # repeated launches: the split counters must return to zero
        out.zero_()
        hip().attn_decode(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), pos.data_ptr(), n_ctx, H, Hkv, hd, scale,
                          ws.data_ptr(), out.data_ptr(), stream(), cnt.data_ptr())
        torch.cuda.synchronize()
        assert rel_err(out.cpu().numpy(), ref) < 3e-3
    assert int(cnt.abs().sum()) == 0


PREFILL_CASES = [(H, 2, T, pos0) for H in (6, 10, 12, 14) for T, pos0 in ((1, 0), (40, 23), (130, 0))]
PREFILL_CASES.append((14, 2, 33, 0))   # G = 7: a padded wave's tile partly past T


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,Hkv,T,pos0", PREFILL_CASES)
def test_attn_prefill_groups_bf16_f16(torch, hd, H, Hkv, T, pos0):
    """Groups 3, 5, 6, 7 on the MFMA kernel (blocks of 4 heads, the last one padded with waves that
    store nothing): the bf16 and f16 outputs the engine feeds its Wo GEMMs."""
    rng = np.random.default_rng(T + pos0 + 7 * H + Hkv)
    n_ctx = 256
    q = rng.standard_normal((T, H, hd)).astype(np.float32)
    K = rng.standard_normal((Hkv, n_ctx, hd)).astype(np.float16)
    V = rng.standard_normal((Hkv, n_ctx, hd)).astype(np.float16)
    scale = 1 / np.sqrt(hd)
    dq, dK, dV = (torch.from_numpy(a).cuda() for a in (q, K, V))
    ref = np.stack([_attn_ref(q[t], K, V, pos0 + t + 1, scale) for t in range(T)])
    # (the row past T is a canary for stores of query rows >= T. The padded waves load a clamped real
    # head, so their store predicate only saves redundant stores over head G - 1.)
    ob = torch.full((T + 1, H, hd), 7.0, device="cuda", dtype=torch.bfloat16)
    hip().attn_prefill(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), T, pos0, n_ctx, H, Hkv, hd, scale,
                       ob.data_ptr(), stream(), True)
    torch.cuda.synchronize()
    assert rel_err(ob[:T].float().cpu().numpy(), ref) < 8e-3
    assert bool((ob[T] == 7.0).all())
    oh = torch.full((T + 1, H * hd), 7.0, device="cuda", dtype=torch.float16)
    hip().attn_prefill(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), T, pos0, n_ctx, H, Hkv, hd, scale,
                       oh.data_ptr(), stream(), out_h=True)
    torch.cuda.synchronize()
    assert rel_err(_swizzle4(oh[:T].float().cpu().numpy()).reshape(T, H, hd), ref) < 3e-3
    assert bool((oh[T] == 7.0).all())


def test_attn_prefill_group3_f32_keeps_the_scalar_path(torch):
    """f32 output, no pieces, group 3: the scalar kernel's 1e-4 (tests/test_kernels_gpu.py pins it)."""
    rng = np.random.default_rng(5)
    T, pos0, H, Hkv, hd, n_ctx = 17, 3, 6, 2, 64, 64
    q = rng.standard_normal((T, H, hd)).astype(np.float32)
    K = rng.standard_normal((Hkv, n_ctx, hd)).astype(np.float16)
    V = rng.standard_normal((Hkv, n_ctx, hd)).astype(np.float16)
    dq, dK, dV = (torch.from_numpy(a).cuda() for a in (q, K, V))
    out = torch.zeros(T, H, hd, device="cuda")
    hip().attn_prefill(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), T, pos0, n_ctx, H, Hkv, hd, 1 / np.sqrt(hd),
                       out.data_ptr(), stream())
    torch.cuda.synchronize()
    ref = np.stack([_attn_ref(q[t], K, V, pos0 + t + 1, 1 / np.sqrt(hd)) for t in range(T)])
    assert rel_err(out.cpu().numpy(), ref) < 1e-4


def test_attn_prefill_pieces_group7(torch):
    """One packed launch, G = 7: three pieces of unequal length at their own positions and KV slots."""
    rng = np.random.default_rng(11)
    H, Hkv, hd, n_ctx, n_slots = 14, 2, 128, 128, 3
    pieces = [(0, 40, 0, 1), (40, 5, 23, 0), (45, 33, 10, 2)]   # (row, n, pos, slot)
    R = sum(p[1] for p in pieces)
    q = rng.standard_normal((R, H, hd)).astype(np.float32)
    K = rng.standard_normal((n_slots, Hkv, n_ctx, hd)).astype(np.float16)
    V = rng.standard_normal((n_slots, Hkv, n_ctx, hd)).astype(np.float16)
    dq, dK, dV = (torch.from_numpy(a).cuda() for a in (q, K, V))
    scale = 1 / np.sqrt(hd)
    ob = torch.full((R + 1, H, hd), 7.0, device="cuda", dtype=torch.bfloat16)
    hip().attn_prefill(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), 0, 0, n_ctx, H, Hkv, hd, scale, ob.data_ptr(),
                       stream(), True, pieces=[list(p) for p in pieces], slot_stride=Hkv * n_ctx * hd)
    torch.cuda.synchronize()
    got = ob.float().cpu().numpy()
    for row, n, pos, slot in pieces:
        ref = np.stack([_attn_ref(q[row + t], K[slot], V[slot], pos + t + 1, scale) for t in range(n)])
        assert rel_err(got[row:row + n], ref) < 8e-3, (row, n, pos, slot)
    assert bool((ob[R] == 7.0).all())


@pytest.mark.parametrize("tq,tk,tv,K", [(GGMLType.Q4_K, GGMLType.Q4_K, GGMLType.Q6_K, 512),   # two runs, one launch
                                        (GGMLType.Q8_0, GGMLType.Q8_0, GGMLType.Q8_0, 896),   # one run, K % 256 != 0
                                        (GGMLType.Q4_K, GGMLType.Q4_K, GGMLType.Q4_K, 8192),  # the one-CU launch
                                        (GGMLType.Q6_K, GGMLType.Q4_K, GGMLType.Q6_K, 512)])  # per-segment launches
def test_gemv_qkv_bias_rope_kvstore(torch, tq, tk, tv, K):
    """The single-row QKV kernel with biases: (W x + b) rotated, q out, K / V rows appended."""
    rng = np.random.default_rng(10)
    hd, nh, nkv, n_ctx, pos = 64, 14, 2, 32, 5
    (rq, Wq), (rk, Wk), (rv, Wv) = make_matrix(tq, nh * hd, K, rng), make_matrix(tk, nkv * hd, K, rng), \
        make_matrix(tv, nkv * hd, K, rng)
    dq, dk, dv = (dev_bytes(to_planar(t, r, R, K)) for t, r, R in ((tq, rq, nh * hd), (tk, rk, nkv * hd), (tv, rv, nkv * hd)))
    x = rng.standard_normal(K).astype(np.float32)
    nw = np.ones(K, np.float32)
    bq, bk, bv = (rng.standard_normal(n).astype(np.float32) * 2 for n in (nh * hd, nkv * hd, nkv * hd))
    dx, dn, dbq, dbk, dbv = (torch.from_numpy(a).cuda() for a in (x, nw, bq, bk, bv))
    qo = torch.zeros(nh * hd, device="cuda")
    kc = torch.zeros(nkv, n_ctx, hd, dtype=torch.float16, device="cuda")
    vc = torch.zeros_like(kc)
    dpos = torch.tensor([pos], dtype=torch.int32, device="cuda")
    inv = 10000.0 ** (-2 * np.arange(hd // 2) / hd)
    ang = np.arange(n_ctx)[:, None] * inv[None]
    rope = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)).cuda()
    hip().gemv_qkv(dq.data_ptr(), int(tq), dk.data_ptr(), int(tk), dv.data_ptr(), int(tv), nh * hd, nkv * hd, K,
                   dx.data_ptr(), dn.data_ptr(), 1e-5, qo.data_ptr(), kc.data_ptr(), vc.data_ptr(), n_ctx, hd,
                   dpos.data_ptr(), rope.data_ptr(), stream(), bq=dbq.data_ptr(), bk=dbk.data_ptr(), bv=dbv.data_ptr())
    torch.cuda.synchronize()
    xq = q8_emulate(rmsnorm(x, nw)).astype(np.float64)

    def rot(v):
        v = v.reshape(-1, hd)
        c, s = np.cos(ang[pos]), np.sin(ang[pos])
        o = v.copy()
        o[:, 0::2] = v[:, 0::2] * c - v[:, 1::2] * s
        o[:, 1::2] = v[:, 0::2] * s + v[:, 1::2] * c
        return o
    assert rel_err(qo.cpu().numpy().reshape(nh, hd), rot(Wq @ xq + bq)) < 1e-3
    assert rel_err(kc[:, pos].float().cpu().numpy(), rot(Wk @ xq + bk)) < 2e-3
    assert rel_err(vc[:, pos].float().cpu().numpy(), (Wv @ xq + bv).reshape(nkv, hd)) < 2e-3
    assert float(kc[:, pos + 1].abs().sum()) == 0.0 and float(vc[:, pos + 1].abs().sum()) == 0.0
    # the biases matter at this bound: the same launch without them is far from the biased reference
    assert rel_err(qo.cpu().numpy().reshape(nh, hd), rot(Wq @ xq)) > 0.1


def _run_sampler(torch, logits, ring_tokens, params, seed, step=0):
    """tests/test_kernels_gpu.py's sampler harness: one row, both stages."""
    h = hip()
    V = logits.shape[0]
    dl = torch.from_numpy(logits).cuda()
    pb = np.frombuffer(h.sampler_params_bytes(params.top_k, params.top_p, params.min_p, params.temperature,
                                              params.repeat_penalty, params.frequency_penalty,
                                              params.presence_penalty, params.last_n, seed,
                                              int(params.temperature <= 0), params.tfs_z, params.typical_p,
                                              dict(params.logit_bias)), np.uint8)
    dp = torch.from_numpy(pb.copy()).cuda()
    ring = np.zeros(64, np.int32)
    rl = min(len(ring_tokens), 64)
    ring[:rl] = ring_tokens[-rl:] if rl else []
    state = np.zeros(8, np.int32)
    state[2], state[3], state[4] = step, rl, rl & 63
    dr, ds = torch.from_numpy(ring).cuda(), torch.from_numpy(state).cuda()
    cand = torch.zeros(h.sampler_cand_words(V), dtype=torch.int32, device="cuda")
    h.sample(dl.data_ptr(), V, dp.data_ptr(), dr.data_ptr(), ds.data_ptr(), cand.data_ptr(), 0, 0, 1, stream())
    torch.cuda.synchronize()
    return int(ds[0].item())


def test_sampler_qwen2_vocabulary(torch):
    """152064 logits (Qwen2.5: 149 stage-1 slices, past the 128 the sampler took): greedy with
    penalties is the host chain's argmax - wherever the winner's slice lies - and seeded sampling
    matches the host chain as it does at the Llama vocabularies."""
    from llama_fastapi_k8s_gpu_amd.engine.sampling import SamplingParams, apply_penalties, filtered_candidates, sample_token
    rng = np.random.default_rng(13)
    V = 152064
    for where in (5, 131072 + 17, V - 1):   # first slice, a slice past 128, the last (partial) slice
        logits = rng.standard_normal(V).astype(np.float32) * 4
        logits[where] = 40.0
        top2 = int(np.argsort(logits)[-2])
        p = SamplingParams(temperature=0.0, top_k=1, repeat_penalty=1.5, frequency_penalty=2.0, presence_penalty=1.0)
        assert _run_sampler(torch, logits, [top2, top2, 7], p, 0) == where
        assert where == int(np.argmax(apply_penalties(logits, [top2, top2, 7], p)))
    agree = outside = 0
    n = 12
    for i in range(n):
        logits = (rng.standard_normal(V) * 3).astype(np.float32)
        hist = list(rng.integers(0, V, 80))
        p = SamplingParams(temperature=1.2, top_k=40, top_p=0.9, min_p=0.05, repeat_penalty=1.1,
                           frequency_penalty=0.7, presence_penalty=0.8, seed=1000 + i)
        tok = _run_sampler(torch, logits, hist, p, p.seed, step=i)
        ids, _ = filtered_candidates(logits, hist[-64:], p)
        outside += tok not in set(ids.tolist())   # f32 vs f64 can move a top-p / min-p boundary by one candidate
        agree += tok == sample_token(logits, hist[-64:], p, i)
    assert outside <= 1 and agree >= n - 1, (outside, agree)


# ---------------------------------------------------------------- engine
def _engine(path, n_slots=1, graph=True, n_ctx=256):
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    return load_hip().Engine(path, n_ctx=n_ctx, n_batch=128, device=0, use_graph=graph, n_slots=n_slots)


@pytest.mark.parametrize("max_batch", [1, 4])   # 1: planar prefill GEMM; 4: batching on (tile16 prefill where K allows)
@pytest.mark.parametrize("spec", ENGINE_SPECS)
def test_engine_prefill_and_greedy_decode_match_reference(models, spec, max_batch):
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    path = models[spec]
    ref = ReferenceLlama(GGUFReader(path), n_ctx=256)
    emu = ReferenceLlama(GGUFReader(path), n_ctx=256)
    assert ref.hp.rope_neox and ref.hp.qkv_bias
    eng = _engine(path, n_slots=max_batch)
    hp = eng.hparams
    assert hp["arch"] == "qwen2" and hp["rope_neox"] is True and hp["qkv_bias"] is True
    if max_batch == 1:
        assert not eng.prefill_t16
    elif spec in ("tiny-qwen2-g7", "tiny-qwen2-g6-hd64"):
        assert eng.prefill_t16, spec
    ppath = "prefill16" if eng.prefill_t16 else "prefill"
    toks = [int(t) for t in np.random.default_rng(0).integers(0, ref.hp.n_vocab, 39)]
    got = eng.eval_logits(toks, 0)
    e = rel_err(got, ref.forward(toks, 0).numpy())
    assert e < 5e-2, (spec, "prefill", e)
    e = rel_err(got, emu.forward(toks, 0, path=ppath).numpy())
    assert e < TIGHT, (spec, ppath, e)
    for i in range(39, 47):   # 8 greedy decode steps on the prefilled cache
        tok = int(np.argmax(got))
        got = eng.decode_logits(tok, i)
        ref_dec = ref.forward([tok], i).numpy()
        e = rel_err(got, ref_dec)
        assert e < 5e-2, (spec, "decode", i, e)
        e = rel_err(got, emu.forward([tok], i, path="decode").numpy())
        assert e < TIGHT, (spec, "decode", i, e)
    assert np.argmax(got) == np.argmax(ref_dec) or \
        ref_dec[np.argmax(got)] > ref_dec.max() - 0.05 * np.abs(ref_dec).max()
    # graph == eager
    sp = {"temperature": 1.0, "top_k": 40, "top_p": 0.95, "seed": 7}
    a = eng.generate(toks[:9], 0, 16, sp, [], None, None)["tokens"]
    b = _engine(path, n_slots=max_batch, graph=False).generate(toks[:9], 0, 16, sp, [], None, None)["tokens"]
    assert a == b and len(a) == 16


def _batch_case(path):
    """B = 3 rows at different positions through batch_step, each row's logits against the same
    sequence decoded one at a time (prefill + single-row decode steps on a second engine), and the
    last step against the fp32 reference. Returns the errors (the caller asserts)."""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    eng = _engine(path, n_slots=4, graph=False)
    one = _engine(path, n_slots=1, graph=False)
    rng = np.random.default_rng(3)
    slots = [3, 0, 1]
    seqs, plen, rows = {}, {}, {s: [] for s in slots}
    for s, n in zip(slots, (5, 40, 17)):
        prompt = [int(t) for t in rng.integers(3, 300, n)]
        seqs[s] = prompt + [eng.slot_begin(s, prompt, 0, GREEDY)]
        plen[s] = n
    picks_ok = True
    for _ in range(3):
        toks = eng.batch_step(slots)
        logits = eng.batch_logits(len(slots))
        for b, s in enumerate(slots):
            rows[s].append(np.array(logits[b]))
            picks_ok = picks_ok and toks[b] == int(np.argmax(logits[b]))
            seqs[s].append(toks[b])
    vs_single, vs_ref = [], []
    for s in slots:
        one.eval_logits(seqs[s][:plen[s]], 0)
        for k in range(3):
            i = plen[s] + k
            vs_single.append(rel_err(rows[s][k], one.decode_logits(seqs[s][i], i)))
        want = ReferenceLlama(GGUFReader(path), n_ctx=256).forward(seqs[s][:plen[s] + 3], 0).numpy()
        vs_ref.append(rel_err(rows[s][2], want))
    return {"vs_single": vs_single, "vs_ref": vs_ref, "picks_ok": bool(picks_ok), "healthy": bool(eng.healthy),
            "defers_rope": bool(hip().bmm_qkv_sk_defers_rope()), "plan": eng.batch_plan(len(slots))}


def _check_batch(r, what, path, split_k):
    """The errors of _batch_case, and the Q|K|V path its engine planned for every (biased) layer:
    split-K with the RoPE and the biases left to the attention, or - split_k False - the one-part
    epilogue where B = 3 rows of this width fit one LDS-staged part, else bprep + bmm + rope_kv_prefill."""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    assert r["healthy"] and r["picks_ok"], (what, r)
    assert max(r["vs_ref"]) < 5e-2, (what, r)
    assert max(r["vs_single"]) < TIGHT, (what, r)
    fits = hip().bmm_qkv_fits(int(GGUFReader(path).metadata["qwen2.embedding_length"]), 3)
    want = ("split_k", "none") if split_k else ("epilogue", "none") if fits else ("unfused", "rope_kv_prefill")
    for l, p in enumerate(r["plan"]):
        assert (p["qkv"], p["finish"]) == want, (what, l, p)
        assert p["sk_defers_rope"] == split_k, (what, l, p)


def _split_k_capable(path, B=3):
    """Does every layer's Q|K|V type mix take the split-K batched projection at B rows?"""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    rd = GGUFReader(path)
    d = int(rd.metadata["qwen2.embedding_length"])
    n_layer = int(rd.metadata["qwen2.block_count"])
    return all(hip().bmm_qkv_sk_supported(*(int(rd.tensors[f"blk.{l}.attn_{x}.weight"].ggml_type) for x in "qkv"), d, B)
               for l in range(n_layer))


# split-K with biases in the batched attention: G = 7 / hd 128 and G = 6 / hd 64 (q4_k_m: Q|K Q4_K
# with V Q4_K or Q6_K); tiny-qwen2-g5 mixes three types per layer, so it takes the one-part /
# unfused path under every setting
BATCH_SPECS = [("tiny-qwen2-g7", True), ("tiny-qwen2-g6-hd64", True), ("tiny-qwen2-g5", False)]


@pytest.mark.parametrize("spec,split_k", BATCH_SPECS)
def test_batch_step_rows_match_single_row_decode(models, spec, split_k, monkeypatch):
    assert _split_k_capable(models[spec]) == split_k, spec
    # the default form: split-K Q|K|V (where the types allow), RoPE and biases in the batched attention
    r = _batch_case(models[spec])
    assert r["defers_rope"]
    _check_batch(r, "default", models[spec], split_k)
    # the one-part Q|K|V epilogue (or, where the rows do not fit it, the unfused RoPE / KV-append kernel)
    monkeypatch.setenv("LFK_QKV_SK", "0")
    _check_batch(_batch_case(models[spec]), "LFK_QKV_SK=0", models[spec], False)


@pytest.mark.parametrize("spec", ["tiny-qwen2-g7", "tiny-qwen2-g6-hd64", "tiny-qwen2-g5"])
def test_batch_step_without_deferred_rope_in_a_child(models, spec):
    """LFK_BMM_IL=0 is read once per process: the split-K partials arrive rotated, so a biased layer
    must leave the split-K path (never drop the bias, never throw mid-step)."""
    env = dict(os.environ, LFK_BMM_IL="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), models[spec]], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert not r["defers_rope"]
    _check_batch(r, "LFK_BMM_IL=0", models[spec], False)


@pytest.mark.parametrize("joint_rows", ["default", "0"])
@pytest.mark.parametrize("spec", ["tiny-qwen2-g7", "tiny-qwen2-g6-hd64"])
def test_joint_admission_matches_sequential(models, spec, joint_rows, monkeypatch):
    """slots_begin packs prompts of unequal length into shared prefill chunks: per-row position / KV
    slot in the biased RoPE / KV-append kernel and every prompt piece in ONE attention launch (padded
    head blocks at G = 7 / 6), one prompt reusing its slot's resident prefix. First tokens and the rows
    of the following batched steps equal slot-by-slot admission (tests/test_batch_gpu.py's form and
    1e-3) and sit within 5e-2 of the fp32 reference. LFK_JOINT_ROWS=0: chunks of n_batch = 32 rows, so
    pieces cross chunk boundaries."""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    if joint_rows != "default":
        monkeypatch.setenv("LFK_JOINT_ROWS", joint_rows)
    kw = dict(n_ctx=256, n_batch=32, device=0, use_graph=False, n_slots=4)
    joint, seq = load_hip().Engine(models[spec], **kw), load_hip().Engine(models[spec], **kw)
    monkeypatch.delenv("LFK_JOINT_ROWS", raising=False)
    assert joint.prefill_t16
    rng = np.random.default_rng(12)
    base = [int(t) for t in rng.integers(3, 300, 21)]
    for e in (joint, seq):                 # slot 1 holds `base`: the joint round reuses it
        e.slot_begin(1, base, 0, GREEDY)
    prompts = [[int(t) for t in rng.integers(3, 300, n)] for n in (45, 7)] + [base + [11, 12, 13]]
    slots, keep = [3, 0, 1], [0, 0, len(base)]
    a = joint.slots_begin(slots, prompts, keep, [GREEDY] * 3)
    b = [seq.slot_begin(s, p, k, GREEDY) for s, p, k in zip(slots, prompts, keep)]
    assert a == b
    seqs = [p + [t] for p, t in zip(prompts, a)]
    for _ in range(3):
        ta, tb = joint.batch_step(slots), seq.batch_step(slots)
        la, lb = joint.batch_logits(3), seq.batch_logits(3)
        for r in range(3):
            assert rel_err(la[r], lb[r]) < 1e-3, (r, rel_err(la[r], lb[r]))
        assert ta == tb
        for r in range(3):
            seqs[r].append(ta[r])
    for r in range(3):   # the last step's rows against the exact model on each row's own sequence
        want = ReferenceLlama(GGUFReader(models[spec]), n_ctx=256).forward(seqs[r][:-1], 0).numpy()
        assert rel_err(la[r], want) < 5e-2, (r, rel_err(la[r], want))
    assert joint.healthy, joint.last_error


def test_hybrid_partial_offload_matches_full_gpu(models):
    """0 < n_gpu_layers < n_layer: CPU layer 0 + GPU layer 1 == all-GPU logits (test_engine_gpu's form)."""
    from llama_fastapi_k8s_gpu_amd.runtime import load_cpu, load_hip
    path = models["tiny-qwen2-g7"]
    full = _engine(path, graph=False)
    toks = [int(t) for t in np.random.default_rng(5).integers(3, 300, 24)]
    want = full.eval_logits(toks, 0)
    want_dec = full.decode_logits(9, 24)
    cpu = load_cpu().CpuEngine(path, n_ctx=256, n_threads=4, n_batch=16, layer_end=1, load_head=False)
    gpu = load_hip().Engine(path, n_ctx=256, n_batch=128, device=0, use_graph=False, layer_begin=1)
    got = gpu.eval_hidden(cpu.eval_hidden(toks, 0), 0)
    got_dec = gpu.eval_hidden(cpu.eval_hidden([9], 24), 24)
    assert rel_err(got, want) < 3e-2
    assert rel_err(got_dec, want_dec) < 3e-2


# ---------------------------------------------------------------- tensor parallelism, two ranks on one GPU
def _tp_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _tp_outputs(llm, toks):
    eng = llm._backend.engine
    out = {"prefill": eng.eval_logits(toks[:39], 0)}
    out["decode"] = [eng.decode_logits(toks[39 + i], 39 + i) for i in range(4)]
    pf = [eng.slot_begin(1, toks[:6], 0, GREEDY), eng.slot_begin(2, toks[3:12], 0, GREEDY)]
    out["batched"] = pf + list(eng.batch_step([1, 2])) + list(eng.batch_step([1, 2]))
    out["healthy"] = bool(llm.health()["ok"])
    return out


def _tp_worker(rank, world, port, path, toks, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world), LOCAL_RANK="0")
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
        kw = dict(n_gpu_layers=-1, n_ctx=256, n_batch=64, seed=5, verbose=False, max_batch=3)
        llm = Llama(path, split_mode="row", tp_comm="ipc", device=0, **kw)
        assert llm._backend.tp_size == world
        res = None
        if rank > 0:
            llm.follow()
            llm.close()
        else:
            got = _tp_outputs(llm, toks)
            llm.close()
            res = (got, _tp_outputs(Llama(path, split_mode="none", **kw), toks))
        dist.barrier()
        q.put((rank, res, None))
        dist.destroy_process_group()
    except BaseException:  # report instead of hanging the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.timeout(300)
def test_tp2_one_gpu_matches_tp1(tmp_path, torch):
    import torch.multiprocessing as mp

    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    path = write_synthetic_gguf("tiny-qwen2-tp", str(tmp_path / "tp.gguf"), seed=4)
    toks = [int(t) for t in np.random.default_rng(11).integers(3, 400, 44)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, path, toks, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            rank, out, err = q.get(timeout=280)
            res[rank] = (out, err)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank in (0, 1):
        assert res[rank][1] is None, f"rank {rank}:\n{res[rank][1]}"
    got, ref = res[0][0]
    exact = ReferenceLlama(GGUFReader(path), n_ctx=256)
    x = [exact.forward(toks[:39], 0).numpy()] + [exact.forward([toks[39 + i]], 39 + i).numpy() for i in range(4)]
    g = [got["prefill"]] + list(got["decode"])
    r1 = [ref["prefill"]] + list(ref["decode"])
    d_tp1 = [_tp_rel(a, b) for a, b in zip(g, r1)]
    e_tp = [_tp_rel(a, b) for a, b in zip(g, x)]
    e_1 = [_tp_rel(a, b) for a, b in zip(r1, x)]
    # tests/test_tp_gpu.py: prefill within 5e-3 of TP=1, decode within 1e-2, and no further from the
    # exact model than TP=1 is (+2e-3)
    for d, tl, t, o in zip(d_tp1, [5e-3] + [1e-2] * 4, e_tp, e_1):
        assert d <= tl and t <= o + 2e-3, (d_tp1, e_tp, e_1)
    assert got["healthy"] and got["batched"] == ref["batched"], (got["batched"], ref["batched"])


if __name__ == "__main__":   # the child of test_batch_step_without_deferred_rope_in_a_child
    print(json.dumps(_batch_case(sys.argv[1])))
