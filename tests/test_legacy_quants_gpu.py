"""The legacy 32-weight block formats (Q4_0, Q4_1, Q5_0, Q5_1) on the GPU: every kernel that
reads weights (decode GEMV and its epilogues, the bf16 prefill GEMM, the embedding gather, the
tile16 copy with the batched MFMA projection and the tile16 prefill GEMM) and the engine end
to end, with the tolerances tests/test_kernels_gpu.py and tests/test_engine_gpu.py use for the
same ops."""
import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import write_synthetic_gguf
from gpu_helpers import dev_bytes, hip, make_matrix, q8_emulate, rel_err, rmsnorm, stream, to_planar

pytestmark = pytest.mark.gpu

NEW = [GGMLType.Q4_0, GGMLType.Q4_1, GGMLType.Q5_0, GGMLType.Q5_1]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _swizzle4(x):
    """The batched path's k order inside each 4-group: (0, 2, 1, 3)."""
    return x.reshape(*x.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(x.shape)


# ---------------------------------------------------------------- 7. GEMV
@pytest.mark.parametrize("t", NEW)
@pytest.mark.parametrize("R,K", [(64, 256), (33, 1024), (130, 4096), (40, 576)])   # 576: no 256-alignment
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


@pytest.mark.parametrize("t", [GGMLType.Q4_1, GGMLType.Q5_0])
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


# ---------------------------------------------------------------- 8. GEMV SwiGLU
@pytest.mark.parametrize("t", [GGMLType.Q4_0, GGMLType.Q5_1])
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


# ---------------------------------------------------------------- 9. bf16 prefill GEMM
@pytest.mark.parametrize("t", NEW)
@pytest.mark.parametrize("T,N,K", [(1, 128, 256), (33, 256, 512), (130, 384, 1024), (17, 64, 576)])
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


# ---------------------------------------------------------------- 10. embedding gather
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


# ---------------------------------------------------------------- 11. tile16 copy + batched MFMA projection
@pytest.mark.parametrize("t", NEW)
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("R,K", [(16, 256), (130, 4096)])
def test_bmm_rows_vs_fp32(torch, t, B, R, K):
    """As tests/test_kernels_gpu.py::test_bmm_rows_vs_fp32 (the padding columns stay untouched),
    and against the product with the f16-arithmetic weights the tile16 copy stands for: a wrong
    stored (a, b) pair moves that one far beyond 2e-4."""
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
    tw = torch.empty(hip().t16_bytes(int(t), R, K), dtype=torch.uint8, device="cuda")
    hip().t16_repack(dw.data_ptr(), int(t), R, K, tw.data_ptr(), stream())
    hip().bmm(tw.data_ptr(), int(t), R, K, dxh.data_ptr(), K, out.data_ptr(), ldo, B, stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = Xh.astype(np.float64) @ W.astype(np.float64).T
    ref16 = Xh.astype(np.float64) @ W16.astype(np.float64).T
    for b in range(B):
        e, e16 = rel_err(got[b, :R] - y0[b], ref[b]), rel_err(got[b, :R] - y0[b], ref16[b])
        print(f"bmm {t.name} B{B} {R}x{K} row {b}: exact {e:.3e} f16 weights {e16:.3e}")
        assert e < 2e-3, (b, e)
        assert e16 < 2e-4, (b, e16)
        assert np.all(got[b, R:] == 0)


# ---------------------------------------------------------------- 12. tile16 prefill GEMM
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


def test_unaligned_k_has_no_tile16_copy(torch):
    for t in NEW:
        assert hip().bmm_supported(int(t), 4096)
        assert not hip().bmm_supported(int(t), 576)


# ---------------------------------------------------------------- 13. engine
ENGINE_SPECS = ["tiny-llama3-q4_0", "tiny-llama3-q5_1", "tiny-llama3-legacy-mixed", "tiny-q5_0-oddff"]


@pytest.fixture(scope="module")
def models(torch, tmp_path_factory):
    d = tmp_path_factory.mktemp("legacy_models")
    return {s: write_synthetic_gguf(s, str(d / f"{s}.gguf"), seed=3) for s in ENGINE_SPECS}


def _engine(path, n_ctx=256, graph=True, **kw):
    return hip().Engine(path, n_ctx=n_ctx, n_batch=128, device=0, use_graph=graph, **kw)


@pytest.mark.parametrize("spec", ENGINE_SPECS)
def test_prefill_and_decode_logits_match_reference(models, spec):
    """Structured as tests/test_engine_gpu.py::test_prefill_and_decode_logits_match_reference:
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


def test_oddff_batch_step_takes_the_fallback(models):
    """n_ff = 576: the down projection (K = 576) has no tile16 copy, so a batched step of two
    slots runs its fallback; every row still matches the exact model."""
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    path = models["tiny-q5_0-oddff"]
    eng = _engine(path, n_slots=3)
    ref = ReferenceLlama(GGUFReader(path), n_ctx=256)
    rng = np.random.default_rng(5)
    greedy = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
    seqs = {}
    for s, n in ((0, 9), (2, 14)):
        prompt = [int(t) for t in rng.integers(3, 300, n)]
        seqs[s] = prompt + [eng.slot_begin(s, prompt, 0, greedy)]
    toks = eng.batch_step([0, 2])
    lg = eng.batch_logits(2)
    assert eng.healthy, eng.last_error
    for b, s in enumerate((0, 2)):
        e = rel_err(lg[b], ref.forward(seqs[s], 0).numpy())
        print(f"oddff batch row {b}: exact {e:.3e}")
        assert e < 5e-2, (s, e)
        assert toks[b] == int(np.argmax(lg[b]))


# ---------------------------------------------------------------- 14. one-layer paths
def test_one_layer_paths_match_emulation(torch, tmp_path):
    """tests/test_engine_gpu.py::test_one_layer_paths_match_emulation on tiny-legacy-mixed-1l:
    prefill, decode, a 3-slot engine's tile16 prefill and two batched steps, each against the
    reference that emulates its rounding: all < 3e-3 and at least 60 % < 1e-4."""
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    spec = "tiny-legacy-mixed-1l"
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


# ---------------------------------------------------------------- hybrid split, MoE refusal
def test_hybrid_partial_offload_matches_full_gpu(models):
    """CPU layer 0 + GPU layers [1, n) == all-GPU logits (tests/test_engine_gpu.py's bound)."""
    from llama_fastapi_k8s_gpu_amd.runtime import load_cpu
    path = models["tiny-llama3-legacy-mixed"]
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


def test_legacy_expert_tensors_are_refused(torch, tmp_path):
    from dataclasses import replace
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS
    spec = replace(SPECS["tiny-mixtral-q4_k_m"], name="tiny-mixtral-q4_0", quant="q4_0")
    path = write_synthetic_gguf(spec, str(tmp_path / "moe.gguf"))
    with pytest.raises(RuntimeError, match=r"ffn_(gate|up|down)_exps\.weight.*Q4_0"):
        _engine(path)


@pytest.mark.parametrize("t", NEW)
def test_fill_random_gives_finite_scales(torch, t):
    """The device-side synthetic fill leaves no random bits in an f16 scale field: every
    decoded weight is finite, centred, and of the requested spread."""
    V, d, std = 64, 576, 0.02
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
