"""The non-linear 4-bit pair (IQ4_NL, IQ4_XS) on the GPU: every kernel that reads weights (decode
GEMV and its epilogues, the bf16 prefill GEMM, the embedding gather, the tile16 copy with the
batched MFMA projection and the tile16 prefill GEMM) and the engine end to end, structured as
tests/test_kquants_23_gpu.py with the same per-op bounds."""
from dataclasses import replace

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, write_synthetic_gguf
from gpu_helpers import dev_bytes, hip, make_matrix, q8_emulate, rel_err, rmsnorm, stream, to_planar

pytestmark = pytest.mark.gpu

IQ4_NL, IQ4_XS, Q5_K = GGMLType.IQ4_NL, GGMLType.IQ4_XS, GGMLType.Q5_K
NEW = [IQ4_NL, IQ4_XS]
# 768: odd superblock count, partial row group; 576 (IQ4_NL only): no 256-alignment
GEMV_SHAPES = [(t, R, K) for t in NEW for R, K in [(16, 256), (33, 768), (130, 4096)]] + [(IQ4_NL, 40, 576)]
GEMM_SHAPES = [(t, T, N, K) for t in NEW for T, N, K in [(1, 128, 256), (33, 256, 512), (130, 384, 1024)]] + \
    [(IQ4_NL, 17, 64, 576)]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _swizzle4(x):
    """The batched path's k order inside each 4-group: (0, 2, 1, 3)."""
    return x.reshape(*x.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(x.shape)


# ---------------------------------------------------------------- GEMV
@pytest.mark.parametrize("t,R,K", GEMV_SHAPES)
def test_gemv_types(torch, t, R, K):
    rng = np.random.default_rng(R * K + int(t))
    raw, W = make_matrix(t, R, K, rng)
    x = rng.standard_normal(K).astype(np.float32)
    dw = dev_bytes(to_planar(t, raw, R, K))
    dx = torch.from_numpy(x).cuda()
    out = torch.zeros(R, device="cuda")
    hip().gemv(dw.data_ptr(), int(t), R, K, dx.data_ptr(), 0, 1e-5, out.data_ptr(), R, 0, stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    e_q8 = rel_err(got, W.astype(np.float64) @ q8_emulate(x).astype(np.float64))
    e_ex = rel_err(got, W.astype(np.float64) @ x.astype(np.float64))
    print(f"gemv {t.name} {R}x{K}: q8 {e_q8:.3e} exact {e_ex:.3e}")
    assert e_q8 < 2e-4
    assert e_ex < 2e-2


@pytest.mark.parametrize("t", NEW)
def test_gemv_norm_add_and_resid(torch, t):
    rng = np.random.default_rng(7)
    R, K = 256, 4096
    raw, W = make_matrix(t, R, K, rng)
    x = rng.standard_normal(K).astype(np.float32) * 3
    nw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    dw = dev_bytes(to_planar(t, raw, R, K))
    dx, dn = torch.from_numpy(x).cuda(), torch.from_numpy(nw).cuda()
    y0 = rng.standard_normal(R).astype(np.float32)
    out = torch.from_numpy(y0.copy()).cuda()
    hip().gemv(dw.data_ptr(), int(t), R, K, dx.data_ptr(), dn.data_ptr(), 1e-5, out.data_ptr(), R, 1, stream())
    torch.cuda.synchronize()
    ref = y0 + W @ q8_emulate(rmsnorm(x, nw))
    e = rel_err(out.cpu().numpy() - y0, ref - y0)
    print(f"gemv norm add {t.name}: {e:.3e}")
    assert e < 1e-3
    res = torch.from_numpy(y0.copy()).cuda()
    out2 = torch.zeros(R, device="cuda")
    hip().gemv(dw.data_ptr(), int(t), R, K, dx.data_ptr(), dn.data_ptr(), 1e-5, out2.data_ptr(), R, 0, stream(),
               resid=res.data_ptr())
    torch.cuda.synchronize()
    e = rel_err(out2.cpu().numpy() - y0, ref - y0)
    print(f"gemv norm resid {t.name}: {e:.3e}")
    assert e < 1e-3


@pytest.mark.parametrize("t", NEW)
def test_gemv_swiglu_interleaved(torch, t):
    rng = np.random.default_rng(8)
    F, K = 128, 512
    rg, Wg = make_matrix(t, F, K, rng)
    ru, Wu = make_matrix(t, F, K, rng)
    planar = to_planar(t, rg, F, K, R_dst=2 * F, G=32, off=0) | to_planar(t, ru, F, K, R_dst=2 * F, G=32, off=32)
    dw = dev_bytes(planar)
    x = rng.standard_normal(K).astype(np.float32)
    dx = torch.from_numpy(x).cuda()
    out = torch.zeros(F, device="cuda")
    hip().gemv(dw.data_ptr(), int(t), 2 * F, K, dx.data_ptr(), 0, 1e-5, out.data_ptr(), F, 2, stream())
    torch.cuda.synchronize()
    xq = q8_emulate(x)
    g, u = Wg @ xq, Wu @ xq
    ref = g / (1 + np.exp(-g)) * u
    e = rel_err(out.cpu().numpy(), ref)
    print(f"gemv swiglu {t.name}: {e:.3e}")
    assert e < 1e-3


@pytest.mark.parametrize("tq,tk,tv,bias", [(IQ4_XS, IQ4_XS, Q5_K, False), (IQ4_XS, IQ4_XS, Q5_K, True),
                                           (IQ4_NL, IQ4_NL, IQ4_NL, False), (IQ4_NL, IQ4_NL, IQ4_NL, True)])
def test_gemv_qkv_rope_kvstore(torch, tq, tk, tv, bias):
    """As tests/test_kquants_23_gpu.py::test_gemv_qkv_rope_kvstore, with its bounds: two type runs
    (one launch per segment) and one run, each with and without biases."""
    rng = np.random.default_rng(10)
    K = 512
    hd, nh, nkv, n_ctx, pos = 64, 8, 2, 32, 5
    (rq, Wq), (rk, Wk), (rv, Wv) = make_matrix(tq, nh * hd, K, rng), make_matrix(tk, nkv * hd, K, rng), \
        make_matrix(tv, nkv * hd, K, rng)
    dq, dk, dv = (dev_bytes(to_planar(t, r, R, K)) for t, r, R in ((tq, rq, nh * hd), (tk, rk, nkv * hd), (tv, rv, nkv * hd)))
    x = rng.standard_normal(K).astype(np.float32)
    nw = np.ones(K, np.float32)
    bq, bk, bv = (rng.standard_normal(n).astype(np.float32) * (2 if bias else 0) for n in (nh * hd, nkv * hd, nkv * hd))
    dx, dn, dbq, dbk, dbv = (torch.from_numpy(a).cuda() for a in (x, nw, bq, bk, bv))
    qo = torch.zeros(nh * hd, device="cuda")
    kc = torch.zeros(nkv, n_ctx, hd, dtype=torch.float16, device="cuda")
    vc = torch.zeros_like(kc)
    dpos = torch.tensor([pos], dtype=torch.int32, device="cuda")
    inv = 10000.0 ** (-2 * np.arange(hd // 2) / hd)
    ang = np.arange(n_ctx)[:, None] * inv[None]
    rope = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)).cuda()
    kw = dict(bq=dbq.data_ptr(), bk=dbk.data_ptr(), bv=dbv.data_ptr()) if bias else {}
    hip().gemv_qkv(dq.data_ptr(), int(tq), dk.data_ptr(), int(tk), dv.data_ptr(), int(tv), nh * hd, nkv * hd, K,
                   dx.data_ptr(), dn.data_ptr(), 1e-5, qo.data_ptr(), kc.data_ptr(), vc.data_ptr(), n_ctx, hd,
                   dpos.data_ptr(), rope.data_ptr(), stream(), **kw)
    torch.cuda.synchronize()
    xq = q8_emulate(rmsnorm(x, nw)).astype(np.float64)

    def rot(v):
        v = v.reshape(-1, hd)
        c, s = np.cos(ang[pos]), np.sin(ang[pos])
        o = v.copy()
        o[:, 0::2] = v[:, 0::2] * c - v[:, 1::2] * s
        o[:, 1::2] = v[:, 0::2] * s + v[:, 1::2] * c
        return o
    eq = rel_err(qo.cpu().numpy().reshape(nh, hd), rot(Wq @ xq + bq))
    ek = rel_err(kc[:, pos].float().cpu().numpy(), rot(Wk @ xq + bk))
    ev = rel_err(vc[:, pos].float().cpu().numpy(), (Wv @ xq + bv).reshape(nkv, hd))
    print(f"qkv {tq.name} {tk.name} {tv.name} bias {bias}: q {eq:.3e} k {ek:.3e} v {ev:.3e}")
    assert eq < 1e-3
    assert ek < 2e-3
    assert ev < 2e-3
    assert float(kc[:, pos + 1].abs().sum()) == 0.0 and float(vc[:, pos + 1].abs().sum()) == 0.0
    if bias:  # the biases matter at this bound
        assert rel_err(qo.cpu().numpy().reshape(nh, hd), rot(Wq @ xq)) > 0.1


# ---------------------------------------------------------------- bf16 prefill GEMM
@pytest.mark.parametrize("t,T,N,K", GEMM_SHAPES)
def test_gemm_mfma(torch, t, T, N, K):
    rng = np.random.default_rng(T * N + int(t))
    raw, W = make_matrix(t, N, K, rng)
    dw = dev_bytes(to_planar(t, raw, N, K))
    x = torch.randn(T, K, device="cuda").to(torch.bfloat16)
    out = torch.zeros(T, N, device="cuda")
    hip().gemm(dw.data_ptr(), int(t), N, K, x.data_ptr(), T, out.data_ptr(), 0, N, 0, stream())
    torch.cuda.synchronize()
    Wb = torch.from_numpy(W).to(torch.bfloat16).float()  # the kernel stages weights as bf16
    ref = x.float().cpu() @ Wb.T
    e = rel_err(out.cpu().numpy(), ref.numpy())
    print(f"gemm {t.name} {T}x{N}x{K}: {e:.3e}")
    assert e < 5e-3
    base = torch.randn(T, N, device="cuda")
    acc = base.clone()
    hip().gemm(dw.data_ptr(), int(t), N, K, x.data_ptr(), T, acc.data_ptr(), 0, N, 1, stream())
    torch.cuda.synchronize()
    assert rel_err((acc - base).cpu().numpy(), ref.numpy()) < 5e-3


# ---------------------------------------------------------------- embedding gather
@pytest.mark.parametrize("t", NEW)
def test_embed(torch, t):
    rng = np.random.default_rng(12)
    V, d = 300, 256
    raw, W = make_matrix(t, V, d, rng)
    dw = dev_bytes(to_planar(t, raw, V, d))
    toks = torch.tensor([0, 5, 17, 299], dtype=torch.int32, device="cuda")
    x = torch.zeros(4, d, device="cuda")
    hip().embed(dw.data_ptr(), int(t), V, d, toks.data_ptr(), 4, x.data_ptr(), stream())
    torch.cuda.synchronize()
    np.testing.assert_allclose(x.cpu().numpy(), W[[0, 5, 17, 299]], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- tile16 copy + batched MFMA projection
@pytest.mark.parametrize("t", NEW)
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("R,K", [(16, 256), (130, 4096)])
@pytest.mark.parametrize("tr", [0, 1])   # weights as the MFMA's A operand / as its B operand
def test_bmm_rows_vs_fp32(torch, t, B, R, K, tr):
    """As tests/test_kquants_23_gpu.py::test_bmm_rows_vs_fp32 (the padding columns stay untouched),
    and against the product with the f16-arithmetic weights the tile16 copy stands for: a wrong
    stored scale or codebook entry moves that one far beyond 2e-4. Both operand orientations."""
    rng = np.random.default_rng(B * 1000 + R + int(t))
    raw, W = make_matrix(t, R, K, rng)
    W16 = dequantize(raw, t, R * K, arith="f16").reshape(R, K)
    dw = dev_bytes(to_planar(t, raw, R, K))
    X = rng.standard_normal((B, K)).astype(np.float32)
    Xh = X.astype(np.float16)
    y0 = rng.standard_normal((B, R)).astype(np.float32)
    ldo = R + 6
    out = torch.zeros(B, ldo, device="cuda")
    out[:, :R] = torch.from_numpy(y0).cuda()
    dxh = torch.from_numpy(_swizzle4(Xh)).cuda()
    assert hip().t16_bytes(int(t), R, K) == ((R + 15) // 16) * (K // 256) * 2304   # one step format: 2304 B < Q4_K's 2560
    tw = torch.empty(hip().t16_bytes(int(t), R, K), dtype=torch.uint8, device="cuda")
    hip().t16_repack(dw.data_ptr(), int(t), R, K, tw.data_ptr(), stream())
    hip().bmm(tw.data_ptr(), int(t), R, K, dxh.data_ptr(), K, out.data_ptr(), ldo, B, stream(), tr=tr)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = Xh.astype(np.float64) @ W.astype(np.float64).T
    ref16 = Xh.astype(np.float64) @ W16.astype(np.float64).T
    for b in range(B):
        e, e16 = rel_err(got[b, :R] - y0[b], ref[b]), rel_err(got[b, :R] - y0[b], ref16[b])
        print(f"bmm {t.name} B{B} {R}x{K} tr{tr} row {b}: exact {e:.3e} f16 weights {e16:.3e}")
        assert e < 2e-3, (b, e)
        assert e16 < 2e-4, (b, e16)
        assert np.all(got[b, R:] == 0)


# ---------------------------------------------------------------- tile16 prefill GEMM
@pytest.mark.parametrize("t", NEW)
@pytest.mark.parametrize("T,R,K", [(17, 256, 512), (100, 272, 1024)])
def test_gemm_t16_vs_fp32(torch, t, T, R, K):
    rng = np.random.default_rng(T + R + K + int(t))
    raw, W = make_matrix(t, R, K, rng)
    dw = dev_bytes(to_planar(t, raw, R, K))
    tw = torch.empty(hip().t16_bytes(int(t), R, K), dtype=torch.uint8, device="cuda")
    hip().t16_repack(dw.data_ptr(), int(t), R, K, tw.data_ptr(), stream())
    Xh = rng.standard_normal((T, K)).astype(np.float16)
    dx = torch.from_numpy(_swizzle4(Xh)).cuda()
    ref = Xh.astype(np.float64) @ W.astype(np.float64).T
    ldo = R + 4
    out = torch.full((T, ldo), 3.0, device="cuda")
    hip().gemm_t16(tw.data_ptr(), int(t), R, K, dx.data_ptr(), T, out.data_ptr(), ldo, 0, 0, 0, stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    e = rel_err(got[:, :R], ref)
    print(f"gemm_t16 {t.name} {T}x{R}x{K}: {e:.3e}")
    assert e < 2e-3, e
    assert np.all(got[:, R:] == 3.0)
    res = torch.randn(T, ldo, device="cuda")
    hip().gemm_t16(tw.data_ptr(), int(t), R, K, dx.data_ptr(), T, out.data_ptr(), ldo, 0, 0, 0, stream(),
                   resid=res.data_ptr())
    torch.cuda.synchronize()
    assert rel_err(out.cpu().numpy()[:, :R] - res.cpu().numpy()[:, :R], ref) < 2e-3
    base = torch.randn(T, ldo, device="cuda")
    acc = base.clone()
    hip().gemm_t16(tw.data_ptr(), int(t), R, K, dx.data_ptr(), T, acc.data_ptr(), ldo, 0, 0, 1, stream())
    torch.cuda.synchronize()
    assert rel_err((acc - base).cpu().numpy()[:, :R], ref) < 2e-3
    assert torch.equal(acc[:, R:], base[:, R:])


def test_block_rules(torch):
    for t in NEW:
        assert hip().bmm_supported(int(t), 4096)
        assert not hip().bmm_supported(int(t), 576)   # the tile16 step is 256 k for both
    assert hip().qbytes(int(IQ4_NL), 4, 576) == 4 * 18 * 18
    with pytest.raises(RuntimeError, match="multiple of the type's block size"):
        hip().qbytes(int(IQ4_XS), 4, 288)
    with pytest.raises(RuntimeError):
        hip().repack(int(IQ4_XS), np.zeros(4 * 2 * 136, np.uint8), 288, 0, 4, 0, 288, 4, 0, 0)


# ---------------------------------------------------------------- engine
ENGINE_SPECS = ["tiny-llama3-iq4_xs", "tiny-llama3-iq4_nl", "tiny-iq4-mixed", "tiny-qwen2-iq4_xs", "tiny-iq4_nl-oddff"]


@pytest.fixture(scope="module")
def models(torch, tmp_path_factory):
    d = tmp_path_factory.mktemp("iq4_models")
    return {s: write_synthetic_gguf(s, str(d / f"{s}.gguf"), seed=3) for s in ENGINE_SPECS}


def _engine(path, n_ctx=256, graph=True, **kw):
    return hip().Engine(path, n_ctx=n_ctx, n_batch=128, device=0, use_graph=graph, **kw)


@pytest.mark.parametrize("spec", ENGINE_SPECS)
def test_prefill_and_decode_logits_match_reference(models, spec):
    """Structured as tests/test_kquants_23_gpu.py::test_prefill_and_decode_logits_match_reference:
    < 5e-2 against the exact model, < 1.5e-2 against the rounding-emulating one."""
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    path = models[spec]
    ref = ReferenceLlama(GGUFReader(path), n_ctx=256)
    emu = ReferenceLlama(GGUFReader(path), n_ctx=256)
    eng = _engine(path)
    rng = np.random.default_rng(0)
    toks = [int(t) for t in rng.integers(0, ref.hp.n_vocab, 44)]
    got_pre = eng.eval_logits(toks[:39], 0)
    e_ref = rel_err(got_pre, ref.forward(toks[:39], 0).numpy())
    e = rel_err(got_pre, emu.forward(toks[:39], 0, path="prefill").numpy())
    print(f"{spec} prefill: exact {e_ref:.3e} emulated {e:.3e}")
    assert e_ref < 5e-2, spec
    assert e < 1.5e-2, (spec, "prefill", e)
    for i in range(39, 44):   # graph-replayed decode steps on the prefilled cache
        ref_dec = ref.forward([toks[i]], i).numpy()
        got_dec = eng.decode_logits(toks[i], i)
        e_ref = rel_err(got_dec, ref_dec)
        e = rel_err(got_dec, emu.forward([toks[i]], i, path="decode").numpy())
        print(f"{spec} decode {i}: exact {e_ref:.3e} emulated {e:.3e}")
        assert e_ref < 5e-2, spec
        assert e < 1.5e-2, (spec, "decode", i, e)


def test_graph_replay_equals_eager_logits(models):
    path = models["tiny-iq4-mixed"]
    toks = [int(t) for t in np.random.default_rng(4).integers(3, 300, 16)]
    outs = []
    for graph in (True, False):
        eng = _engine(path, graph=graph)
        eng.eval_logits(toks[:12], 0)
        outs.append([eng.decode_logits(toks[i], i).copy() for i in range(12, 16)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_one_layer_paths_match_emulation(torch, tmp_path):
    """tests/test_kquants_23_gpu.py::test_one_layer_paths_match_emulation on tiny-iq4-mixed-1l
    (IQ4_NL, IQ4_XS, Q4_K and Q6_K in one layer): prefill, decode, a 3-slot engine's tile16 prefill and two
    batched steps, each against the reference that emulates its rounding: all < 3e-3 and at least
    60 % < 1e-4."""
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    spec = "tiny-iq4-mixed-1l"
    path = write_synthetic_gguf(spec, str(tmp_path / f"{spec}.gguf"), seed=6)
    emu = ReferenceLlama(GGUFReader(path), n_ctx=128)
    toks = [int(t) for t in np.random.default_rng(2).integers(3, 500, 30)]
    eng = _engine(path, n_ctx=128)
    errs = [("prefill", rel_err(eng.eval_logits(toks[:20], 0), emu.forward(toks[:20], 0, path="prefill").numpy()))]
    for i in range(20, 25):
        errs.append((f"decode{i}", rel_err(eng.decode_logits(toks[i], i),
                                           emu.forward([toks[i]], i, path="decode").numpy())))
    beng = hip().Engine(path, n_ctx=128, n_batch=64, device=0, use_graph=True, n_slots=3)
    assert beng.prefill_t16
    ppath = "prefill16"
    errs.append((ppath, rel_err(beng.eval_logits(toks[:20], 0),
                                ReferenceLlama(GGUFReader(path), n_ctx=128).forward(toks[:20], 0, path=ppath).numpy())))
    greedy = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
    seqs = {0: toks[:9], 2: toks[:14]}
    for s in seqs:
        seqs[s] = seqs[s] + [beng.slot_begin(s, seqs[s], 0, greedy)]
    for step in range(2):
        out = beng.batch_step([0, 2])
        lg = beng.batch_logits(2)
        for b, s in enumerate((0, 2)):
            n = len(seqs[s])
            em = ReferenceLlama(GGUFReader(path), n_ctx=128)
            em.forward(seqs[s][:n - 1 - step], 0, path=ppath)
            for i in range(n - 1 - step, n - 1):
                em.forward([seqs[s][i]], i, path="batch")
            errs.append((f"batch{step}.{s}", rel_err(lg[b], em.forward([seqs[s][n - 1]], n - 1, path="batch").numpy())))
            seqs[s].append(out[b])
    print("one-layer errors:", [(n, f"{e:.3e}") for n, e in errs])
    exact_bits = sum(e < 1e-4 for _, e in errs)
    assert exact_bits >= 0.6 * len(errs) and all(e < 3e-3 for _, e in errs), errs


def test_batched_step_equals_single_row_decodes(models):
    """A batched step of 3 rows against the same three sequences decoded one row at a time, within
    tests/test_batch_gpu.py::test_batched_and_serial_decode_agree_near_n_ctx's bound (5e-2), and
    both against the fp32 reference."""
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    path = models["tiny-iq4-mixed"]
    bat = hip().Engine(path, n_ctx=128, n_batch=64, device=0, use_graph=True, n_slots=3)
    one = _engine(path, n_ctx=128, graph=False)
    ref = ReferenceLlama(GGUFReader(path), n_ctx=128)
    rng = np.random.default_rng(21)
    greedy = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
    seqs = []
    for s, n in enumerate((7, 20, 13)):
        p = [int(t) for t in rng.integers(3, 300, n)]
        seqs.append(p + [bat.slot_begin(s, p, 0, greedy)])
    toks = bat.batch_step([0, 1, 2])
    lb = bat.batch_logits(3)
    for b, seq in enumerate(seqs):
        one.eval_logits(seq[:-1], 0)
        ls = one.decode_logits(seq[-1], len(seq) - 1)
        want = ref.forward(seq, 0).numpy()
        print(f"row {b}: batched {rel_err(lb[b], want):.3e} serial {rel_err(ls, want):.3e} apart {rel_err(lb[b], ls):.3e}")
        assert rel_err(lb[b], want) < 5e-2 and rel_err(ls, want) < 5e-2
        assert rel_err(lb[b], ls) < 5e-2, (b, rel_err(lb[b], ls))
        assert toks[b] == int(np.argmax(lb[b]))
    assert bat.healthy, bat.last_error


# ---------------------------------------------------------------- hybrid split, MoE refusal, random fill
def test_hybrid_partial_offload_matches_full_gpu(models):
    """CPU layer 0 + GPU layers [1, n) == all-GPU logits (tests/test_engine_gpu.py's bound)."""
    from llama_fastapi_k8s_gpu_amd.runtime import load_cpu
    path = models["tiny-llama3-iq4_xs"]
    full = _engine(path, graph=False)
    toks = [int(t) for t in np.random.default_rng(5).integers(3, 300, 24)]
    want = full.eval_logits(toks, 0)
    want_dec = full.decode_logits(9, 24)
    cpu = load_cpu().CpuEngine(path, n_ctx=256, n_threads=4, n_batch=16, layer_end=1, load_head=False)
    gpu = hip().Engine(path, n_ctx=256, n_batch=128, device=0, use_graph=False, layer_begin=1)
    got = gpu.eval_hidden(cpu.eval_hidden(toks, 0), 0)
    got_dec = gpu.eval_hidden(cpu.eval_hidden([9], 24), 24)
    assert rel_err(got, want) < 3e-2
    assert rel_err(got_dec, want_dec) < 3e-2


def test_iq4_expert_tensors_are_refused(torch, tmp_path):
    spec = replace(SPECS["tiny-mixtral-q4_k_m"], name="tiny-mixtral-iq4_xs", quant="iq4_xs")
    path = write_synthetic_gguf(spec, str(tmp_path / "moe.gguf"))
    with pytest.raises(RuntimeError, match=r"ffn_(gate|up|down)_exps\.weight.*IQ4_XS"):
        _engine(path)


@pytest.mark.parametrize("t", NEW)
def test_fill_random_gives_finite_scales(torch, t):
    """The device-side synthetic fill leaves no random bits in an f16 scale field: every
    decoded weight is finite, centred, and of the requested spread."""
    V, d, std = 64, 768, 0.02
    buf = torch.empty(hip().qbytes(int(t), V, d), dtype=torch.uint8, device="cuda")
    hip().fill_random(buf.data_ptr(), int(t), V, d, std, 11, stream())
    toks = torch.arange(V, dtype=torch.int32, device="cuda")
    x = torch.zeros(V, d, device="cuda")
    hip().embed(buf.data_ptr(), int(t), V, d, toks.data_ptr(), V, x.data_ptr(), stream())
    torch.cuda.synchronize()
    w = x.cpu().numpy()
    assert np.isfinite(w).all()
    # d is jittered by U(0.5, 1.5) per block: the overall spread stays within those factors
    assert 0.5 * std < w.std() < 1.5 * std, w.std()
    assert abs(w.mean()) < 0.25 * std, w.mean()
