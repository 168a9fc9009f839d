"""The batched decode step's dense FFN chains at kernel level against fp64, at the K-part shapes the
other chain tests never run (they compare the chain with the project's own separate launches, on two
shapes whose parts are all of one size):

  * bmm_ffn_chain - one part, two ragged parts, a 1-step last part, 11 parts, the 15 parts the
    counters hold, the folded norm over ragged parts; down Q4_K and Q6_K, the legacy 4-bit types that
    run as Q4_K; both orientations of the down's split-K epilogue; the down's zero side job;
  * bmm_wo_ffn_chain - Wo over K = d and K != d (2 parts) in front of ragged downs;
  * the predicates against the launchers, and the engine on a model whose down plans 16 parts.

Every case runs three launches over re-zeroed counters; h starts as f16 NaN and out as random residual
rows, each with a guard row. Checked per launch: every row of h and of out - resid by itself
(ffn_chain_ref.check_chain), the guard rows bit for bit, the timeout word, and the kernel's own
counters per K part against the plan mirror - so a case advertised as ragged or as 15 parts fails
loudly when the launch rule moves. References and checkers: tests/ffn_chain_ref.py (CPU self-test:
tests/test_ffn_chain_ref.py)."""
import numpy as np
import pytest

from gpu_helpers import dense_ffn_path, dev_bytes, hip, rel_err, stream, to_planar
import ffn_chain_ref as cr
import moe_ref as mr

pytestmark = pytest.mark.gpu

Q4_K = cr.Q4_K
POISON32 = mr.NAN32


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch
    _DEV.clear()   # the module's weights leave the device and the host with it
    _HREF.clear()
    cr.forget_weights()


_DEV, _HREF = {}, {}


def _filled(torch, shape, dtype, pattern):
    it = {2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]
    return torch.full(shape, pattern, dtype=it, device="cuda").view(dtype)


def _bits(torch, t):
    it, ut = {2: (torch.int16, np.uint16), 4: (torch.int32, np.uint32)}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy().view(ut)


def _t16(torch, t, R, C, tag, swiglu=False):
    """The tile16 copy of cr.weights(t, R, C, tag) on the device, and its dequantised values."""
    key = (int(t), R, C, tag)
    if key not in _DEV:
        raw, W = cr.weights(t, R, C, tag)
        dw = dev_bytes(to_planar(t, raw, R, C))
        tw = torch.empty(hip().t16_bytes(int(t), R, C), dtype=torch.uint8, device="cuda")
        hip().t16_repack(dw.data_ptr(), int(t), R, C, tw.data_ptr(), stream(), swiglu=swiglu)
        torch.cuda.synchronize()
        _DEV[key] = (tw, W)
    return _DEV[key]


def _cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _counters(torch, cnt):
    stride, xcds, n_ints = hip().chain_layout()
    assert n_ints == cr.MAX_PARTS * xcds * stride
    return cr.counters_per_part(cnt.cpu().numpy(), stride, xcds)


def _run_chain(torch, tg, td, K, F, norm, B, tr, zero_from=None):
    """zero_from: the first launch (of three) that also carries the down's zero side job."""
    plan = cr.chain_plan(F, K, _cus(torch))
    what = (tg.name, td.name, "K", K, "F", F, "norm", norm, "B", B, "tr", tr, "parts", plan.part_steps)
    assert cr.chain_takes(plan) and hip().bmm_ffn_chain_supported(int(tg), F, K, int(td), B, norm), what
    tgw, Wgu = _t16(torch, tg, 2 * F, K, "gu", swiglu=True)
    tdw, Wd = _t16(torch, td, K, F, "dn")
    X, nw, resid = cr.chain_rows(K, B, norm, 100 * B + F)
    key = (int(tg), K, F, norm, B)
    if key not in _HREF:
        _HREF[key] = cr.h_reference(X, nw, Wgu, norm)
    h_ref = _HREF[key]
    dxh = torch.from_numpy(mr.swizzle4(X.astype(np.float16))).cuda()
    dxf, dnw = torch.from_numpy(X).cuda(), torch.from_numpy(nw).cuda()
    xf_ptr, nw_ptr = (dxf.data_ptr(), dnw.data_ptr()) if norm else (0, 0)
    dres = torch.from_numpy(resid).cuda()
    _, _, n_ints = hip().chain_layout()
    cnt = torch.zeros(n_ints, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    # the side job's float4 count: whole rounds of the down's blocks x 512 threads and a partial one
    zero_n = 4 * (plan.n2 * 512 + 301)
    worst, h_first = [0.0, 0.0], None
    for launch in range(3):
        cnt.zero_()
        err.zero_()
        h = _filled(torch, (B + 1, F), torch.float16, mr.NAN16)
        out = dres.clone()
        zargs, z = {}, None
        if zero_from is not None and launch >= zero_from:
            z = _filled(torch, (zero_n + 64,), torch.float32, POISON32)
            zargs = dict(zero=z.data_ptr(), zero_n=zero_n)
        hip().bmm_ffn_chain(tgw.data_ptr(), int(tg), F, K, dxh.data_ptr(), xf_ptr, nw_ptr, cr.EPS, tdw.data_ptr(), int(td),
                            h.data_ptr(), out.data_ptr(), B, cnt.data_ptr(), stream(), tr=tr, err=err.data_ptr(), **zargs)
        torch.cuda.synchronize()
        w = what + ("launch", launch)
        assert int(err.item()) == 0, (w, "a consumer's wait timed out")
        hb = _bits(torch, h)
        fh, fd = cr.check_chain(hb, out.cpu().numpy(), resid, h_ref, Wd, w)
        worst = [max(worst[0], fh), max(worst[1], fd)]
        cr.check_counters(_counters(torch, cnt), plan, what=w)
        if h_first is None:
            h_first = hb
        assert np.array_equal(hb, h_first), (w, "h differs between launches")   # (one K part, plain stores)
        if z is not None:
            cr.check_zeroed(_bits(torch, z), zero_n, POISON32, w)
    return worst, plan


@pytest.mark.parametrize("tg,td,K,F,norm,B,tr", cr.CHAIN_CASES)
def test_ffn_chain_vs_fp64(torch, tg, td, K, F, norm, B, tr):
    """bmm_ffn_chain against fp64, stage by stage and row by row, with the counters of every K part
    equal to the plan: h within 3e-3 (test_bmm_swiglu_epilogue_vs_fp32's bound), out - resid within
    2e-3 of the fp64 down projection of the h read back (test_bmm_rows_vs_fp32's)."""
    w, plan = _run_chain(torch, tg, td, K, F, norm, B, tr)
    print(f"CHAIN_FRAC ffn_chain {tg.name}/{td.name} K={K} F={F} norm={int(norm)} B={B} tr={tr} "
          f"parts={plan.part_steps} h {w[0]:.3f} down {w[1]:.3f}")


@pytest.mark.parametrize("tg,td,K,F,norm,B,tr", cr.ZERO_CASES)
def test_ffn_chain_zero_side_job(torch, tg, td, K, F, norm, B, tr):
    """The down role re-zeroes the next layer's split-K rows (BmmArgs::zero, as the engine hands it
    to the chain): exactly zero_n floats of a poisoned buffer become 0 - zero_n is no multiple of the
    down's blocks x 512 threads - the 64 behind them keep the poison, and the chain's own results and
    counters are what they are without the side job (the first launch runs without it)."""
    w, plan = _run_chain(torch, tg, td, K, F, norm, B, tr, zero_from=1)
    print(f"CHAIN_FRAC ffn_chain_zero {tg.name}/{td.name} K={K} F={F} B={B} tr={tr} parts={plan.part_steps} "
          f"h {w[0]:.3f} down {w[1]:.3f}")


@pytest.mark.parametrize("K,F", cr.CHAIN_REFUSED)
@pytest.mark.parametrize("B", [1, 8])
def test_ffn_chain_refuses_what_its_counters_do_not_hold(torch, K, F, B):
    """More K parts than counters (K = 512, F = 8192: 16 parts of 2 steps): the predicate says so -
    the engine then takes its separate launches - and the launcher raises before any launch, with
    every buffer untouched."""
    plan = cr.chain_plan(F, K, _cus(torch))
    assert not cr.chain_takes(plan), plan.part_steps
    assert not hip().bmm_ffn_chain_supported(int(Q4_K), F, K, int(Q4_K), B, False)
    tgw = torch.zeros(hip().t16_bytes(int(Q4_K), 2 * F, K), dtype=torch.uint8, device="cuda")
    tdw = torch.zeros(hip().t16_bytes(int(Q4_K), K, F), dtype=torch.uint8, device="cuda")
    dxh = torch.zeros(B, K, dtype=torch.float16, device="cuda")
    h = _filled(torch, (B + 1, F), torch.float16, mr.NAN16)
    out = torch.ones(B + 1, K, device="cuda")
    _, _, n_ints = hip().chain_layout()
    cnt = torch.zeros(n_ints, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="bmm_ffn_chain: unsupported shapes"):
        hip().bmm_ffn_chain(tgw.data_ptr(), int(Q4_K), F, K, dxh.data_ptr(), 0, 0, cr.EPS, tdw.data_ptr(), int(Q4_K),
                            h.data_ptr(), out.data_ptr(), B, cnt.data_ptr(), stream(), err=err.data_ptr())
    torch.cuda.synchronize()
    assert np.all(_bits(torch, h) == mr.NAN16) and bool((out == 1).all())
    assert not bool(cnt.any()) and int(err.item()) == 0


# ---------------------------------------------------------------------------- Wo in front
@pytest.mark.parametrize("td,F,Kwo,B", cr.WO_CASES)
def test_wo_ffn_chain_vs_fp64(torch, td, F, Kwo, B):
    """bmm_wo_ffn_chain (K = 4096, the folded norm): the final rows against resid0 + Wo + down(h read
    back) within 2e-3 (|Wo_b| + |down_b|), h against the fp64 SwiGLU of norm(resid0 + Wo) within 3e-3 +
    2.2 delta_b (ffn_chain_ref's header), the counters of the down's parts, of the gate/up blocks and
    of the Wo blocks equal to the plans. Kwo = 1024: Wo's K != d, two parts."""
    K = 4096
    cus = _cus(torch)
    plan, wplan = cr.chain_plan(F, K, cus), cr.chain_plan(Kwo, K, cus)
    what = (td.name, "F", F, "Kwo", Kwo, "B", B, "parts", plan.part_steps, "wo parts", wplan.part_steps)
    assert cr.wo_chain_takes(wplan, plan), what
    assert hip().bmm_wo_ffn_chain_supported(int(Q4_K), Kwo, int(Q4_K), F, K, int(td), B), what
    tow, Wo = _t16(torch, Q4_K, K, Kwo, "wo")
    tgw, Wgu = _t16(torch, Q4_K, 2 * F, K, "gu", swiglu=True)
    tdw, Wd = _t16(torch, td, K, F, "dn")
    rng = np.random.default_rng(1000 * B + F + Kwo)
    XA = rng.standard_normal((B, Kwo)).astype(np.float16)
    resid0 = (2 * rng.standard_normal((B + 1, K))).astype(np.float32)
    nw = (0.5 + rng.random(K)).astype(np.float32)
    wo_ref = XA.astype(np.float64) @ Wo.astype(np.float64).T
    dxa, dnw, dres = torch.from_numpy(mr.swizzle4(XA)).cuda(), torch.from_numpy(nw).cuda(), torch.from_numpy(resid0).cuda()
    xh = torch.zeros(B, K, dtype=torch.float16, device="cuda")   # (unused: the norm path stages resid)
    _, _, n_ints = hip().chain_layout()
    cnt = torch.zeros(n_ints, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    worst = [0.0, 0.0]
    for launch in range(3):
        cnt.zero_()
        err.zero_()
        h = _filled(torch, (B + 1, F), torch.float16, mr.NAN16)
        r = dres.clone()
        hip().bmm_wo_ffn_chain(tow.data_ptr(), int(Q4_K), Kwo, dxa.data_ptr(), tgw.data_ptr(), int(Q4_K), F, K,
                               dnw.data_ptr(), cr.EPS, tdw.data_ptr(), int(td), xh.data_ptr(), h.data_ptr(), r.data_ptr(),
                               B, cnt.data_ptr(), stream(), err=err.data_ptr())
        torch.cuda.synchronize()
        w = what + ("launch", launch)
        assert int(err.item()) == 0, (w, "a wait timed out")
        fh, ff = cr.check_wo_chain(_bits(torch, h), r.cpu().numpy(), resid0, wo_ref, nw, Wgu, Wd, w)
        worst = [max(worst[0], fh), max(worst[1], ff)]
        cr.check_counters(_counters(torch, cnt), plan, wo_blocks=wplan.n2, what=w)
    print(f"CHAIN_FRAC wo_ffn_chain {td.name} F={F} Kwo={Kwo} B={B} parts={plan.part_steps} wo_parts={wplan.part_steps} "
          f"h {worst[0]:.3f} final {worst[1]:.3f}")


@pytest.mark.parametrize("F,Kwo", cr.WO_REFUSED)
def test_wo_ffn_chain_refuses_a_one_part_down(torch, F, Kwo):
    """F = 512: the down is one K part, which the three-role launch does not take (its down blocks
    wait per part behind Wo's counter): predicate false, the launcher raises before any launch."""
    K, B = 4096, 6
    cus = _cus(torch)
    assert not cr.wo_chain_takes(cr.chain_plan(Kwo, K, cus), cr.chain_plan(F, K, cus))
    assert not hip().bmm_wo_ffn_chain_supported(int(Q4_K), Kwo, int(Q4_K), F, K, int(Q4_K), B)
    tow = torch.zeros(hip().t16_bytes(int(Q4_K), K, Kwo), dtype=torch.uint8, device="cuda")
    tgw = torch.zeros(hip().t16_bytes(int(Q4_K), 2 * F, K), dtype=torch.uint8, device="cuda")
    tdw = torch.zeros(hip().t16_bytes(int(Q4_K), K, F), dtype=torch.uint8, device="cuda")
    dxa = torch.zeros(B, Kwo, dtype=torch.float16, device="cuda")
    xh = torch.zeros(B, K, dtype=torch.float16, device="cuda")
    nw = torch.ones(K, device="cuda")
    h = _filled(torch, (B + 1, F), torch.float16, mr.NAN16)
    r = torch.ones(B + 1, K, device="cuda")
    _, _, n_ints = hip().chain_layout()
    cnt = torch.zeros(n_ints, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="bmm_wo_ffn_chain: unsupported shapes"):
        hip().bmm_wo_ffn_chain(tow.data_ptr(), int(Q4_K), Kwo, dxa.data_ptr(), tgw.data_ptr(), int(Q4_K), F, K,
                               nw.data_ptr(), cr.EPS, tdw.data_ptr(), int(Q4_K), xh.data_ptr(), h.data_ptr(), r.data_ptr(),
                               B, cnt.data_ptr(), stream(), err=err.data_ptr())
    torch.cuda.synchronize()
    assert np.all(_bits(torch, h) == mr.NAN16) and bool((r == 1).all())
    assert not bool(cnt.any()) and int(err.item()) == 0


# ---------------------------------------------------------------------------- the engine
def test_batch_step_16_part_down_takes_the_separate_launches(tmp_path):
    """d = 2048, n_ff = 8192 (Llama-3.2-1B's FFN shape, one layer): the down plans 16 K parts of 2
    steps, one more than the chain's counters hold, so the batched step must take the gate/up and the
    down as separate launches - before the predicate knew the part count, every batched step of such
    a model threw `too many K parts for the counters`. Rows against the fp32 reference and the
    emulation at test_batch_step_d4096_fused_paths' bounds."""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import ModelSpec, write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    spec = ModelSpec("llama-d2048-ff8192-1l", 2048, 1, 16, 4, 8192, 0, 500000.0, "bpe", "q4_k_m", n_ctx_train=1024)
    path = write_synthetic_gguf(spec, str(tmp_path / "ff8192.gguf"))
    eng = load_hip().Engine(path, n_ctx=128, n_batch=64, device=0, use_graph=True, n_slots=4)
    # the engine's plan is the separate launches, and that is the predicate's answer over this layer's
    # own types and shapes on this device (no CU count spelled here)
    for B in (3, 2):
        (p,) = eng.batch_plan(B)
        assert p["ffn"] == "swiglu" and p["ffn"] == dense_ffn_path(path, 0, B), (B, p)
    ref = ReferenceLlama(GGUFReader(path), n_ctx=128)
    emu = ReferenceLlama(GGUFReader(path), n_ctx=128)
    rng = np.random.default_rng(6)
    greedy = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
    seqs, plen, worst = {}, {}, [0.0, 0.0]
    for s, n in zip((2, 0, 3), (6, 11, 9)):
        prompt = [int(t) for t in rng.integers(3, 300, n)]
        seqs[s] = prompt + [eng.slot_begin(s, prompt, 0, greedy)]
        plen[s] = n
    for rows in ([2, 0, 3], [0, 3]):
        toks = eng.batch_step(rows)
        logits = eng.batch_logits(len(rows))
        for b, s in enumerate(rows):
            e32 = rel_err(logits[b], ref.forward(seqs[s], 0).numpy())
            assert e32 < 5e-2, (s, e32)
            out = emu.forward(seqs[s][:plen[s]], 0, path="prefill16" if eng.prefill_t16 else "prefill")
            for i in range(plen[s], len(seqs[s])):
                out = emu.forward([seqs[s][i]], i, path="batch")
            e = rel_err(logits[b], out.numpy())
            assert e < 1.5e-2, (s, e)
            worst = [max(worst[0], e32 / 5e-2), max(worst[1], e / 1.5e-2)]
            assert toks[b] == int(np.argmax(logits[b]))
            seqs[s].append(toks[b])
    assert eng.healthy, eng.last_error
    print(f"CHAIN_FRAC engine d=2048 n_ff=8192 fp32 {worst[0]:.3f} emulation {worst[1]:.3f}")
