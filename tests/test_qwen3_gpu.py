"""Qwen3 on the MI355X engine: QK-norm at every site that finishes a Q|K|V sum, and a head width that
is not n_embd / n_head.

Kernel level, against the fp64 reference of qknorm_ref.py under qkv_ref.check_qkv (NORM_BOUND 3e-3 per
segment, ELEM_BOUND per element, sentinel-filled caches and q buffers with guard slots): the head norm
+ RoPE + KV append kernel alone, the batched split-K Q|K|V followed by the QKNORM attention, and the
single-row raw-sum GEMV followed by the norm kernel at T = 1. Every site has one case whose head-norm
eps is about half a head's mean square: a kernel that omits eps, or norms the sums before the row
scale, passes at the model's 1e-6 (tests/test_qknorm_ref.py shows it).

Engine level: the tiny Qwen3 specs against the fp32 reference (which norms the file's own rows and
rotates NeoX pairs) and its path emulation; forms and bounds are test_qwen2_gpu.py's.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_helpers import dev_bytes, hip, make_matrix, q8_emulate, rel_err, rmsnorm, stream, to_planar
from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from qknorm_ref import SK_CASES, head_norm, qknorm_from_rows, qknorm_reference, splitk_inputs
from qkv_ref import _rope_pairs, _rope_table, check_qkv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_SPECS = ["tiny-qwen3-g2-hd128", "tiny-qwen3-g4-hd64", "tiny-qwen3-g5", "tiny-qwen3-g8", "tiny-qwen3-tp"]
TIGHT = 1.5e-2   # test_engine_gpu.TIGHT / test_batch_gpu.TIGHT for tiny-llama3-q4_k_m
GREEDY = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
ATTN_BOUND = 5e-3   # test_bmm_qkv_splitk_then_attention's bound on the attention output against fp64
GUARD = 1           # guard slots in front of and behind the slots the kernels see


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def models(tmp_path_factory, torch):
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    d = tmp_path_factory.mktemp("qwen3_gpu_models")
    return {s: write_synthetic_gguf(s, str(d / f"{s}.gguf"), seed=3) for s in ENGINE_SPECS}


def _norm_weights(rng, hd):
    """[q_norm | k_norm] as the synthetic files draw them (1 + 0.5 N(0, 1)), already in kernel order."""
    return (1.0 + 0.5 * rng.standard_normal(2 * hd)).astype(np.float32)


def _sentinel_caches(torch, rng, n_slots, Hkv, n_ctx, hd):
    """K / V allocations of n_slots + 2 GUARD slots, random f16 sentinels; (host K, host V, device K,
    device V, pointer to the kernels' slot 0 of each)."""
    shape = (n_slots + 2 * GUARD, Hkv, n_ctx, hd)
    sK, sV = rng.standard_normal(shape).astype(np.float16), rng.standard_normal(shape).astype(np.float16)
    dK, dV = torch.from_numpy(sK).cuda(), torch.from_numpy(sV).cuda()
    off = GUARD * Hkv * n_ctx * hd * 2
    return sK, sV, dK, dV, dK.data_ptr() + off, dV.data_ptr() + off


# ---------------------------------------------------------------- the head norm + RoPE + KV append kernel
NORM_CASES = [(hd, G, form, False) for hd in (64, 128) for G in (2, 5, 8) for form in ("prompt", "batched")]
NORM_CASES += [(128, 5, "batched", True), (64, 2, "prompt", True)]   # eps = half a head's mean square


@pytest.mark.parametrize("hd,G,form,big_eps", NORM_CASES,
                         ids=[f"hd{h}-G{g}-{f}{'-big_eps' if e else ''}" for h, g, f, e in NORM_CASES])
def test_qk_norm_rope_kv(torch, hd, G, form, big_eps):
    """One wave per head of one token: head norm, rotation, q out as f32, k / v as f16 into the slot
    caches. Prompt form T = 3 at pos0 = 5; batched form with per-row positions (one past the context
    end, clamped) and slots."""
    rng = np.random.default_rng(hd + 7 * G + (form == "prompt"))
    Hkv, n_ctx, R = 2, 32, 3
    nq, nkv = G * Hkv * hd, Hkv * hd
    rows = rng.standard_normal((R, nq + 2 * nkv)).astype(np.float32)   # unit variance: a head's mean square is ~1
    w = _norm_weights(rng, hd)
    eps = 0.5 if big_eps else 1e-6
    tab = _rope_table(n_ctx, hd)
    if form == "prompt":
        pos0, n_slots = 5, 1
        pos, slots = np.arange(pos0, pos0 + R, dtype=np.int32), np.zeros(R, np.int32)
    else:
        n_slots = 3
        pos, slots = np.array([0, n_ctx - 1, n_ctx + 4], np.int32), np.array([2, 0, 1], np.int32)   # the last one clamps
    ref = qknorm_from_rows(rows, nq, nkv, w, eps, pos, slots, tab, n_ctx, hd)
    assert ref.pos.tolist() == ([5, 6, 7] if form == "prompt" else [0, n_ctx - 1, n_ctx - 1])
    sK, sV, dK, dV, pK, pV = _sentinel_caches(torch, rng, n_slots, Hkv, n_ctx, hd)
    sq = rng.standard_normal((R + 1, nq)).astype(np.float32)
    dq = torch.from_numpy(sq).cuda()
    drows, dw, dtab = torch.from_numpy(rows).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(tab).cuda()
    if form == "prompt":
        hip().qk_norm_rope_kv(drows.data_ptr(), R, 5, nq, nkv, hd, n_ctx, dtab.data_ptr(), dw.data_ptr(), eps,
                              dq.data_ptr(), pK, pV, stream())
    else:
        dpos, dslots = torch.from_numpy(pos).cuda(), torch.from_numpy(slots).cuda()
        hip().qk_norm_rope_kv(drows.data_ptr(), R, 0, nq, nkv, hd, n_ctx, dtab.data_ptr(), dw.data_ptr(), eps,
                              dq.data_ptr(), pK, pV, stream(), pos_arr=dpos.data_ptr(), slot_arr=dslots.data_ptr(),
                              slot_stride=Hkv * n_ctx * hd)
    torch.cuda.synchronize()
    if form == "batched":   # rows 1 and 2 of the batched form write slots 0 and 1 at the same position: both kept
        assert ref.slots.tolist() == [2, 0, 1]
    worst = check_qkv(dq.cpu().numpy(), dK.cpu().numpy(), dV.cpu().numpy(), ref, sK, sV, sentinel_q=sq, slot0=GUARD)
    print("qk_norm_rope_kv", hd, G, form, big_eps, worst)


# ---------------------------------------------------------------- batched split-K Q|K|V, then the QKNORM attention
def _attn_ref(q, K, V, L, scale):
    H, D = q.shape
    G = H // K.shape[0]
    out = np.zeros((H, D))
    for h in range(H):
        s = K[h // G, :L].astype(np.float64) @ q[h].astype(np.float64) * scale
        p = np.exp(s - s.max())
        p /= p.sum()
        out[h] = p @ V[h // G, :L].astype(np.float64)
    return out


# (live, timeline): every LIVE mode, and the timeline (TL) instantiations with and without LIVE
SK_MODES = [(0, False), (1, False), (2, False), (0, True), (1, True)]


@pytest.mark.parametrize("live,tl", SK_MODES, ids=[f"live{l}{'-tl' if t else ''}" for l, t in SK_MODES])
@pytest.mark.parametrize("hd,G,big_eps", SK_CASES, ids=[f"hd{h}-G{g}{'-big_eps' if e else ''}" for h, g, e in SK_CASES])
def test_bmm_qkv_splitk_then_qknorm_attention(torch, hd, G, big_eps, live, tl):
    """bmm_qkv_sk leaves raw sums of f16(x * norm_w) . W and the rows' sums of squares; the QKNORM
    attention computes rot(headnorm(q rs, q_norm)) scale, rot(headnorm(k rs, k_norm)) and v rs, appends
    the new K / V rows and attends. Checked: those rows (check_qkv; q itself never leaves the kernel,
    the attention output stands for it) and the output against an fp64 attention over the
    reference cache. L = 1, 65 (the second 64-key split) and the context end. The inputs are
    qknorm_ref.splitk_inputs's, whose f16 staging test_qknorm_ref.py measures on the CPU. tl: the
    timeline form must give the same results and stamp every block's entry and exit."""
    t = GGMLType.Q4_K
    B, Hkv, K, n_ctx, n_slots = 3, 2, 512, 128, 4
    assert hip().bmm_qkv_sk_supported(int(t), int(t), int(t), K, B)
    assert hip().bmm_qkv_sk_defers_rope()
    c = splitk_inputs(hd, G, big_eps, t)
    rng, X, nw, w, eps, qkn_eps, pos, slots = (c[k] for k in ("rng", "X", "nw", "w", "eps", "qkn_eps", "pos", "slots"))
    H = G * Hkv
    nq, nkv = H * hd, Hkv * hd
    mats = []
    for (raw, W), R in zip(c["mats"], (nq, nkv, nkv)):
        dw = dev_bytes(to_planar(t, raw, R, K))
        tw = torch.empty(hip().t16_bytes(int(t), R, K), dtype=torch.uint8, device="cuda")
        hip().t16_repack(dw.data_ptr(), int(t), R, K, tw.data_ptr(), stream())
        mats.append((tw, W, dw))
    assert pos.tolist() == [0, 64, n_ctx - 1] and X.shape == (B, K)   # L = 1, 65, n_ctx
    tab = _rope_table(n_ctx, hd)
    ref = qknorm_reference(X, nw, eps, [m[1] for m in mats], w, qkn_eps, pos, slots, tab, n_ctx, hd, staging="folded")
    ldo = nq + 2 * nkv
    dx, dn, dwn = torch.from_numpy(X).cuda(), torch.from_numpy(nw).cuda(), torch.from_numpy(w).cuda()
    dtab, dpos, dslots = torch.from_numpy(tab).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(slots).cuda()
    dfreq = torch.from_numpy((5e5 ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)).astype(np.float32)).cuda()
    out = torch.zeros(B, ldo, device="cuda")
    ss = torch.zeros(16, device="cuda")
    hip().bmm_qkv_sk(mats[0][0].data_ptr(), int(t), nq, mats[1][0].data_ptr(), int(t), mats[2][0].data_ptr(), int(t),
                     nkv, K, dx.data_ptr(), K, dn.data_ptr(), eps, B, out.data_ptr(), ldo, ss.data_ptr(),
                     dpos.data_ptr(), dtab.data_ptr(), hd, n_ctx, stream())
    sK, sV, dK, dV, pK, pV = _sentinel_caches(torch, rng, n_slots, Hkv, n_ctx, hd)
    part = torch.zeros(B * hip().attn_decode_workspace_floats(n_ctx, H, hd), device="cuda")
    cnt = torch.zeros(64 * B, dtype=torch.int32, device="cuda")
    aout = torch.zeros(B, nq, device="cuda")
    aouth = torch.zeros(B, nq, dtype=torch.float16, device="cuda")
    scale = 1 / np.sqrt(hd)
    nblk = Hkv * ((n_ctx + 63) // 64) * B          # the launch's blocks, 16 stamps each; 16 guard words behind
    clk = torch.zeros(16 * nblk + 16, dtype=torch.int64, device="cuda")
    hip().attn_decode(out.data_ptr(), pK, pV, dpos.data_ptr(), n_ctx, H, Hkv, hd, scale,
                      part.data_ptr(), aout.data_ptr(), stream(), cnt.data_ptr(), dbg_clk=clk.data_ptr() if tl else 0,
                      batch=B, slots=dslots.data_ptr(),
                      slot_stride=Hkv * n_ctx * hd, out_h=aouth.data_ptr(), qkv_raw=out.data_ptr(), qkv_ld=ldo, k_off=nq,
                      v_off=nq + nkv, ss=ss.data_ptr(), inv_k=1.0 / K, eps=eps, rope_freq=dfreq.data_ptr(), live=live,
                      qk_norm=dwn.data_ptr(), qkn_eps=qkn_eps)
    torch.cuda.synchronize()
    Kg, Vg = dK.cpu().numpy(), dV.cpu().numpy()
    worst = check_qkv(ref.q.astype(np.float32), Kg, Vg, ref, sK, sV, slot0=GUARD)
    ao = aout.cpu().numpy()
    worst_attn = 0.0
    for b in range(B):
        s, p = GUARD + int(slots[b]), int(pos[b])
        Kr, Vr = sK[s].copy(), sV[s].copy()
        Kr[:, p], Vr[:, p] = ref.k[b].astype(np.float16), ref.v[b].astype(np.float16)
        want = _attn_ref(ref.q[b].reshape(H, hd), Kr, Vr, p + 1, scale)
        e = rel_err(ao[b].reshape(H, hd), want)
        worst_attn = max(worst_attn, e / ATTN_BOUND)
        assert e < ATTN_BOUND, (b, e)
    assert int(cnt.abs().sum()) == 0
    stamps = clk.cpu().numpy()
    assert not stamps[16 * nblk:].any()
    if tl:   # every block stamps its entry (word 0); a block with keys to serve stamps its loads (word 2)
        st = stamps[:16 * nblk].reshape(nblk, 16)
        assert (st[:, 0] > 0).all() and (st[:, 2] > 0).any()
    else:
        assert not stamps.any()
    print("splitk+qknorm attention", hd, G, big_eps, live, tl, worst, "attn", worst_attn)


# ---------------------------------------------------------------- single row: raw-sum GEMV, then the norm kernel
GEMV_CASES = [((GGMLType.Q4_K, GGMLType.Q4_K, GGMLType.Q6_K), 512, False),   # two runs, one launch
              ((GGMLType.Q8_0,) * 3, 896, False),                            # one run, K % 256 != 0
              ((GGMLType.Q6_K, GGMLType.Q4_K, GGMLType.Q6_K), 512, False),   # per-segment launches
              ((GGMLType.Q4_0,) * 3, 512, False),                            # a legacy type (gemv_legacy.hip)
              ((GGMLType.Q4_K, GGMLType.Q4_K, GGMLType.Q6_K), 512, True)]


@pytest.mark.parametrize("types,K,big_eps", GEMV_CASES,
                         ids=["q4k_q4k_q6k", "q8_0_K896", "q6k_q4k_q6k", "q4_0", "q4k_q4k_q6k-big_eps"])
def test_gemv_qkv_raw_then_qk_norm(torch, types, K, big_eps):
    """gemv_qkv's raw form stores the normalised sums [nq | nkv | nkv] and nothing else; qk_norm_rope_kv
    at T = 1 finishes them at the position read from the device. Against the q8-emulated fp64 product
    (test_gemv_qkv_bias_rope_kvstore's reference and bounds: 1e-3 for q, 2e-3 for the f16 k / v)."""
    tq, tk, tv = types
    rng = np.random.default_rng(10 + K + int(tq))
    hd, nh, nkvh, n_ctx, pos = 64, 8, 2, 32, 5
    nq, nkv = nh * hd, nkvh * hd
    mats = [make_matrix(t, R, K, rng, std=1.0) for t, R in ((tq, nq), (tk, nkv), (tv, nkv))]
    dq, dk, dv = (dev_bytes(to_planar(t, m[0], R, K)) for t, m, R in zip(types, mats, (nq, nkv, nkv)))
    x = rng.standard_normal(K).astype(np.float32)
    nw = np.ones(K, np.float32)
    w = _norm_weights(rng, hd)
    qkn_eps = 0.5 * K if big_eps else 1e-6
    tab = _rope_table(n_ctx, hd)
    dx, dn, dwn, dtab = (torch.from_numpy(a).cuda() for a in (x, nw, w, tab))
    sraw = rng.standard_normal(nq + 2 * nkv + 8).astype(np.float32)
    draw = torch.from_numpy(sraw).cuda()
    sK, sV, dK, dV, pK, pV = _sentinel_caches(torch, rng, 1, nkvh, n_ctx, hd)
    sq = rng.standard_normal((2, nq)).astype(np.float32)
    dqo = torch.from_numpy(sq).cuda()
    dpos = torch.tensor([pos], dtype=torch.int32, device="cuda")
    hip().gemv_qkv(dq.data_ptr(), int(tq), dk.data_ptr(), int(tk), dv.data_ptr(), int(tv), nq, nkv, K,
                   dx.data_ptr(), dn.data_ptr(), 1e-5, 0, 0, 0, n_ctx, hd, dpos.data_ptr(), 0, stream(),
                   raw_out=draw.data_ptr())
    torch.cuda.synchronize()
    got_raw = draw.cpu().numpy()
    assert np.array_equal(got_raw[nq + 2 * nkv:], sraw[nq + 2 * nkv:])           # nothing past the row
    assert np.array_equal(dK.cpu().numpy().view(np.uint16), sK.view(np.uint16))  # the raw form appends nothing
    xq = q8_emulate(rmsnorm(x, nw)).astype(np.float64)
    raw = np.concatenate([m[1].astype(np.float64) @ xq for m in mats])
    assert rel_err(got_raw[:nq + 2 * nkv], raw) < 1e-3
    hip().qk_norm_rope_kv(draw.data_ptr(), 1, 0, nq, nkv, hd, n_ctx, dtab.data_ptr(), dwn.data_ptr(), qkn_eps,
                          dqo.data_ptr(), pK, pV, stream(), pos_dev=dpos.data_ptr())
    torch.cuda.synchronize()
    ref = qknorm_from_rows(raw[None], nq, nkv, w, qkn_eps, [pos], [0], tab, n_ctx, hd)
    got_q, Kg, Vg = dqo.cpu().numpy(), dK.cpu().numpy(), dV.cpu().numpy()
    e = (rel_err(got_q[0], ref.q[0]), rel_err(Kg[GUARD, :, pos], ref.k[0]), rel_err(Vg[GUARD, :, pos], ref.v[0]))
    print("gemv raw + qk_norm", [int(t) for t in types], K, big_eps, e)
    assert e[0] < 1e-3 and e[1] < 2e-3 and e[2] < 2e-3, e
    check_qkv(got_q, Kg, Vg, ref, sK, sV, sentinel_q=sq, slot0=GUARD)            # and nothing else was written
    # the norm matters at this bound: the same launch is far from the reference without it
    plain = _rope_pairs(raw[:nq], pos, tab)
    assert rel_err(got_q[0], plain) > 0.1
    assert rel_err(Kg[GUARD, :, pos].ravel(), _rope_pairs(raw[nq:nq + nkv], pos, tab)) > 0.1
    if big_eps:   # and so does eps
        assert rel_err(got_q[0], _rope_pairs(head_norm(raw[:nq], w[:hd], 0.0, hd), pos, tab)) > 0.1


# ---------------------------------------------------------------- engine
def _engine(path, n_slots=1, graph=True, n_ctx=256):
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    return load_hip().Engine(path, n_ctx=n_ctx, n_batch=128, device=0, use_graph=graph, n_slots=n_slots)


@pytest.mark.parametrize("max_batch", [1, 4])   # 1: planar prefill GEMM; 4: batching on (tile16 prefill where K allows)
@pytest.mark.parametrize("spec", ENGINE_SPECS)
def test_engine_prefill_and_greedy_decode_match_reference(models, spec, max_batch):
    """tiny-qwen3-g2-hd128 has n_q = 1024 at n_embd = 768: n_q != n_embd end to end."""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    path = models[spec]
    ref = ReferenceLlama(GGUFReader(path), n_ctx=256)
    emu = ReferenceLlama(GGUFReader(path), n_ctx=256)
    assert ref.hp.rope_neox and ref.hp.qk_norm and not ref.hp.qkv_bias
    eng = _engine(path, n_slots=max_batch)
    hp = eng.hparams
    assert hp["arch"] == "qwen3" and hp["rope_neox"] is True and hp["qk_norm"] is True and hp["qkv_bias"] is False
    assert hp["head_dim"] == SPECS[spec].head_dim
    if spec == "tiny-qwen3-g2-hd128":
        assert hp["n_head"] * hp["head_dim"] == 1024 != hp["n_embd"] == 768
    if max_batch == 1:
        assert not eng.prefill_t16
    ppath = "prefill16" if eng.prefill_t16 else "prefill"
    toks = [int(t) for t in np.random.default_rng(0).integers(0, ref.hp.n_vocab, 39)]
    got = eng.eval_logits(toks, 0)
    worst = {"ref": 0.0, "emu": 0.0}   # as fractions of 5e-2 and TIGHT

    def judge(what, e_ref, e_emu):
        worst["ref"], worst["emu"] = max(worst["ref"], e_ref / 5e-2), max(worst["emu"], e_emu / TIGHT)
        assert e_ref < 5e-2, (spec, what, e_ref)
        assert e_emu < TIGHT, (spec, what, "emulation", e_emu)

    judge(ppath, rel_err(got, ref.forward(toks, 0).numpy()), rel_err(got, emu.forward(toks, 0, path=ppath).numpy()))
    forced = []
    for i in range(39, 47):   # 8 greedy decode steps on the prefilled cache
        tok = int(np.argmax(got))
        forced.append(tok)
        got = eng.decode_logits(tok, i)
        ref_dec = ref.forward([tok], i).numpy()
        judge(("decode", i), rel_err(got, ref_dec), rel_err(got, emu.forward([tok], i, path="decode").numpy()))
    print("engine", spec, max_batch, ppath, worst)
    assert np.argmax(got) == np.argmax(ref_dec) or \
        ref_dec[np.argmax(got)] > ref_dec.max() - 0.05 * np.abs(ref_dec).max()
    # graph == eager, exactly and on ONE cache: the eager engine loads the graph engine's K / V rows
    # instead of prefilling its own. Two prefills of one file are not bit-equal (the planar prefill GEMM
    # adds its K parts into the residual with atomics; at d = 2048 and max_batch 1 that moves decode
    # logits by up to 8e-3 - the same for a Llama file of this shape), so test_qwen2_gpu.py's two sampled
    # generations part now and then for a reason that is none of the graph's. The decode step has no
    # such sum, so on one cache graph and eager must agree bit for bit:
    #  (a) eight teacher-forced steps through decode_logits, which replays the captured graph (the
    #      norm kernel's device position, the raw-sum buffer);
    #  (b) all 15 decode tokens of a greedy generate() on the graph engine (its own loop, the device
    #      sampler): each is the argmax of the eager engine's logits for the same step on the cache
    #      generate() left. (Token 0 comes from the prompt's prefill, not from the graph.)
    eager = _engine(path, n_slots=max_batch, graph=False)
    n = len(toks)
    eng.eval_logits(toks, 0)
    eager.kv_load(eng.kv_save(n), n)
    for i in range(8):
        a, b = eng.decode_logits(forced[i], n + i), eager.decode_logits(forced[i], n + i)
        assert np.array_equal(np.asarray(a), np.asarray(b)), (spec, "graph vs eager decode step", i, rel_err(a, b))
    g = eng.generate(toks[:9], 0, 16, GREEDY, [], None, None)["tokens"]
    assert len(g) == 16
    eager.kv_load(eng.kv_save(9 + 15), 9 + 15)
    for k in range(1, 16):
        lg = np.asarray(eager.decode_logits(g[k - 1], 9 + k - 1))
        assert int(np.argmax(lg)) == g[k], (spec, "generate() on the graph vs eager decode", k, g)


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


def _check_batch(r, what, split_k):
    """The errors of _batch_case, and the Q|K|V path its engine planned for every (QK-norm) layer:
    split-K with the head norm and the RoPE left to the attention, or - split_k False - bprep + bmm +
    the head-norm kernel: such a layer declines the one-part epilogue and its folded norm."""
    print("batch", what, "vs_ref / 5e-2", max(r["vs_ref"]) / 5e-2, "vs_single / TIGHT", max(r["vs_single"]) / TIGHT)
    assert r["healthy"] and r["picks_ok"], (what, r)
    assert max(r["vs_ref"]) < 5e-2, (what, r)
    assert max(r["vs_single"]) < TIGHT, (what, r)
    want = ("split_k", "none", True) if split_k else ("unfused", "qk_norm_rope_kv", False)
    for l, p in enumerate(r["plan"]):
        assert (p["qkv"], p["finish"], p["qkv_norm_folded"]) == want, (what, l, p)
        assert p["sk_defers_rope"] == split_k, (what, l, p)


def _split_k_capable(path, B=3):
    """Does every layer's Q|K|V type mix take the split-K batched projection at B rows?"""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    rd = GGUFReader(path)
    d = int(rd.metadata["qwen3.embedding_length"])
    n_layer = int(rd.metadata["qwen3.block_count"])
    return all(hip().bmm_qkv_sk_supported(*(int(rd.tensors[f"blk.{l}.attn_{x}.weight"].ggml_type) for x in "qkv"), d, B)
               for l in range(n_layer))


# split-K with the QKNORM attention at hd 128 (G = 2, 8) and hd 64 (G = 4); tiny-qwen3-g5 mixes three
# types per layer, so it takes bprep + bmm + the head-norm kernel under every setting
BATCH_SPECS = [("tiny-qwen3-g2-hd128", True), ("tiny-qwen3-g4-hd64", True), ("tiny-qwen3-g5", False),
               ("tiny-qwen3-g8", True)]


@pytest.mark.parametrize("spec,split_k", BATCH_SPECS)
def test_batch_step_rows_match_single_row_decode(models, spec, split_k, monkeypatch):
    assert _split_k_capable(models[spec]) == split_k, spec
    r = _batch_case(models[spec])       # the default: split-K Q|K|V (where the types allow), norm + RoPE in the attention
    assert r["defers_rope"]
    _check_batch(r, "default", split_k)
    monkeypatch.setenv("LFK_QKV_SK", "0")   # no split-K: a QK-norm layer declines the one-part epilogue too
    _check_batch(_batch_case(models[spec]), "LFK_QKV_SK=0", False)


@pytest.mark.parametrize("spec", ["tiny-qwen3-g2-hd128", "tiny-qwen3-g4-hd64", "tiny-qwen3-g5"])
def test_batch_step_without_deferred_rope_in_a_child(models, spec):
    """LFK_BMM_IL=0 is read once per process: the split-K partials arrive rotated, so a QK-norm layer
    must leave the split-K path (never drop the norm, never throw mid-step)."""
    env = dict(os.environ, LFK_BMM_IL="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), models[spec]], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert not r["defers_rope"]
    _check_batch(r, "LFK_BMM_IL=0", False)


@pytest.mark.parametrize("spec", ["tiny-qwen3-g2-hd128", "tiny-qwen3-g4-hd64"])
def test_joint_admission_matches_sequential(models, spec):
    """slots_begin packs prompts of unequal length into shared prefill chunks: per-row position / KV
    slot in the head-norm kernel, one prompt reusing its slot's resident prefix. First tokens and the
    rows of the following batched steps equal slot-by-slot admission (tests/test_batch_gpu.py's form
    and 1e-3) and sit within 5e-2 of the fp32 reference."""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    kw = dict(n_ctx=256, n_batch=32, device=0, use_graph=False, n_slots=4)
    joint, seq = load_hip().Engine(models[spec], **kw), load_hip().Engine(models[spec], **kw)
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
    path = models["tiny-qwen3-g2-hd128"]
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
    """The norm weights are replicated: heads never straddle ranks."""
    import torch.multiprocessing as mp

    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    path = write_synthetic_gguf("tiny-qwen3-tp", str(tmp_path / "tp.gguf"), seed=4)
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
