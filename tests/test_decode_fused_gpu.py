"""The single-row decode step's two fused launches at kernel level - neither had a binding:

  * attn_wo1 (gemv.hip): the decode attention and the split-K Wo GEMV in one launch; the Wo blocks
    issue their weights, wait for the attention's per-kv-head done counters and quantise x from its
    output. Against fp64 at every done branch (one live split: store and count; more: the
    last-arriving split merges and counts), with one to four K parts, a grid-stride second item, a
    ragged 4-row group, surplus Wo blocks, Q4_K and Q6_K, back to back on one workspace, and
    against the two separate launches.
  * the gate/up GEMV that routes the token itself (GemvArgs::route_w): the picks, weights and logits
    block 0 writes against moe_router_fused (bit for bit) and fp64, the SwiGLU rows against fp64 of
    the picked experts and, bit for bit, against the unrouted launch - one case per configuration
    class of the launcher, the class it has no routed kernel for (gemv_route_fits) included.

And at engine level: a MoE model in that class decodes, and LFK_WO_FUSE=0 / 1 agree past 64 tokens.
References, inputs and checkers: tests/decode_fused_ref.py (CPU self-test: test_decode_fused_ref.py).
Each test prints its worst error (DECODE_FUSED ...)."""
from dataclasses import replace

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize, random_blocks
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, write_synthetic_gguf
from gpu_helpers import dev_bytes, hip, make_matrix, rel_err, stream, to_planar
import decode_fused_ref as fr

pytestmark = pytest.mark.gpu

Q4_K, Q6_K, Q8_0 = fr.Q4_K, fr.Q6_K, fr.Q8_0
HD = fr.HD
SCALE = 1 / np.sqrt(HD)
NAN32 = 0x7FC00ABC   # f32 quiet NaN with a payload: the outputs' sentinel
PAD = 8              # sentinel floats past every slot's F features

_CACHE = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch
    _CACHE.clear()   # the module's weights leave the device with it


def _nan32(torch, n):
    return torch.full((n,), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(torch, t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ attention + Wo
def _wo(t, name):
    """The case's Wo: (planar copy on the device, dequantised [rows][K]). Cases of one K share the
    matrix (the shorter one takes its first rows)."""
    _, H, _, rows, _ = fr.FUSED_CASES[name]
    K = H * HD
    key = ("wo", int(t), K)
    if key not in _CACHE:
        R = max(c[3] for c in fr.FUSED_CASES.values() if c[1] * HD == K)
        _CACHE[key] = make_matrix(t, R, K, np.random.default_rng(int(t) * 10 + K))
    raw, W = _CACHE[key]
    pk = ("wo_planar", int(t), K, rows)
    if pk not in _CACHE:
        rb = raw.size // W.shape[0]
        _CACHE[pk] = dev_bytes(to_planar(t, raw[:rows * rb], rows, K))
    return _CACHE[pk], W[:rows]


def _att_ref(name, L):
    key = ("att", name, L)
    if key not in _CACHE:
        q, _, Kc, Vc = fr.fused_inputs(name, L)
        _CACHE[key] = fr.attn_ref(q, Kc, Vc, L, SCALE)
    return _CACHE[key]


class _Ws:
    """One shape's workspace, kept across launches: split partials and counters, the attention
    output, x_out, the 64 done words (the engine's embedding launch zeroes them) and the error word."""

    def __init__(self, torch, name):
        n_kv, H, n_ctx, rows, _ = fr.FUSED_CASES[name]
        self.part = torch.zeros(hip().attn_decode_workspace_floats(n_ctx, H, HD), device="cuda")
        self.cnt = torch.zeros(64, dtype=torch.int32, device="cuda")
        self.att = torch.zeros(H * HD, device="cuda")
        self.x_out = torch.zeros(rows, device="cuda")
        self.done = torch.zeros(64, dtype=torch.int32, device="cuda")
        self.err = torch.zeros(1, dtype=torch.int32, device="cuda")


def _upload(torch, name, L):
    q, resid, Kc, Vc = fr.fused_inputs(name, L)
    return (torch.from_numpy(q).cuda(), torch.from_numpy(resid).cuda(), torch.from_numpy(fr.poisoned(Kc, L)).cuda(),
            torch.from_numpy(fr.poisoned(Vc, L)).cuda(), torch.tensor([L - 1], dtype=torch.int32, device="cuda"), resid)


def _fused(torch, name, t, L, ws):
    """One attn_wo1 launch over NaN cache rows from L on, a NaN attention buffer, x_out = the residual
    and zeroed done words. Returns (launched, attention output, x_out, residual)."""
    n_kv, H, n_ctx, rows, _ = fr.FUSED_CASES[name]
    dw, _ = _wo(t, name)
    dq, dres, dK, dV, dpos, resid = _upload(torch, name, L)
    ws.att.fill_(float("nan"))
    ws.x_out.copy_(dres)
    ws.done.zero_()
    ok = hip().attn_wo1(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), dpos.data_ptr(), n_ctx, H, n_kv, HD, SCALE,
                        ws.part.data_ptr(), ws.att.data_ptr(), stream(), ws.cnt.data_ptr(), ws.done.data_ptr(),
                        dw.data_ptr(), int(t), rows, H * HD, ws.x_out.data_ptr(), ws.err.data_ptr())
    torch.cuda.synchronize()
    return ok, ws.att.cpu().numpy().reshape(H, HD), ws.x_out.cpu().numpy(), resid


def _check(torch, name, t, L, ws, ok, att, x_out, resid, tag):
    assert ok is True, (tag, "attn_wo1 refused the engine's default shape")
    n_kv = fr.FUSED_CASES[name][0]
    e = fr.check_fused(att, x_out, resid, ws.done.cpu().numpy(), ws.cnt.cpu().numpy(), int(ws.err.item()),
                       _att_ref(name, L), _wo(t, name)[1], n_kv, (tag, name, t.name, "L", L))
    print(f"DECODE_FUSED {tag} {name} {t.name} L={L}: attention {e[0]:.3g} (< {fr.ATTN}) Wo {e[1]:.3g} (< {fr.WO})")


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("name,L", fr.FUSED_PARAMS)
def test_attn_wo1_vs_fp64(torch, name, L, t):
    """(a) - (d): launched; the attention output against fp64 over the keys < L (the rows from L on are
    NaN); x_out - residual against W times the q8 of the attention output read back (the attention
    buffer starts as NaN, so an early, partial or stale x shows); done[h] = 1 for the kv heads and 0
    in the other words, the split counters back at 0, no timed-out wait."""
    ws = _Ws(torch, name)
    _check(torch, name, t, L, ws, *_fused(torch, name, t, L, ws), "fused")


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("name", list(fr.FUSED_CASES))
def test_attn_wo1_back_to_back(torch, name, t):
    """(e): three launches on one workspace, the live splits going many -> one -> two; only the done
    words are zeroed in between (the partials and the split counters are the kernel's to keep)."""
    ws = _Ws(torch, name)
    for L in fr.REPEAT_LENS[name]:
        _check(torch, name, t, L, ws, *_fused(torch, name, t, L, ws), "repeat")


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("name,L", fr.FUSED_PARAMS)
def test_attn_wo1_matches_two_launches(torch, name, L, t):
    """(f): attn_decode then gemv (EPI_ADD) over the same inputs. Both attentions are
    attn_decode_body<128, 4, false> with the same arguments (the done words only change the store
    instructions): equal bit for bit. The Wo sums differ in the order of the split-K atomics."""
    n_kv, H, n_ctx, rows, _ = fr.FUSED_CASES[name]
    ws = _Ws(torch, name)
    ok, att, x_out, resid = _fused(torch, name, t, L, ws)
    assert ok is True
    dw, _ = _wo(t, name)
    dq, dres, dK, dV, dpos, _ = _upload(torch, name, L)
    att2 = torch.full((H * HD,), float("nan"), device="cuda")
    x2 = dres.clone()
    hip().attn_decode(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), dpos.data_ptr(), n_ctx, H, n_kv, HD, SCALE,
                      ws.part.data_ptr(), att2.data_ptr(), stream(), ws.cnt.data_ptr())
    hip().gemv(dw.data_ptr(), int(t), rows, H * HD, att2.data_ptr(), 0, 1e-5, x2.data_ptr(), rows, 1, stream())
    torch.cuda.synchronize()
    a2, y2 = att2.cpu().numpy().reshape(H, HD), x2.cpu().numpy()
    assert np.isfinite(a2).all() and np.isfinite(y2).all() and np.isfinite(x_out).all()
    same = np.array_equal(att.view(np.uint32), a2.view(np.uint32))
    e = rel_err(x_out.astype(np.float64) - resid, y2.astype(np.float64) - resid)
    print(f"DECODE_FUSED two-launch {name} {t.name} L={L}: attention bit-equal {same}, Wo {e:.3g} (< {fr.WO})")
    assert same, ("attention outputs differ", rel_err(att, a2))
    assert e < fr.WO, e
    assert int(ws.cnt.abs().sum()) == 0


# (head_dim, kv heads, heads, Wo type): each one step outside what attn_wo1 takes
REFUSALS = [(64, 8, 32, Q4_K), (128, 2, 16, Q4_K), (128, 4, 16, Q8_0), (128, 2, 8, Q4_K)]


@pytest.mark.parametrize("hd,n_kv,H,t", REFUSALS, ids=["hd64", "G8", "Q8_0", "K1024"])
def test_attn_wo1_refuses_without_launching(torch, hd, n_kv, H, t):
    """head_dim 64, a GQA group of 8, a Q8_0 Wo, K = 1024 (no multiple of 2048): False, and nothing
    ran - x_out holds the residual's bits, the attention buffer is still NaN."""
    n_ctx, rows, K = 64, 64, H * hd
    rng = np.random.default_rng(hd + H)
    dq = torch.from_numpy(rng.standard_normal(K).astype(np.float32)).cuda()
    dK = torch.zeros(n_kv, n_ctx, hd, dtype=torch.float16, device="cuda")
    dV = torch.zeros_like(dK)
    dpos = torch.tensor([9], dtype=torch.int32, device="cuda")
    part = torch.zeros(hip().attn_decode_workspace_floats(n_ctx, H, hd), device="cuda")
    cnt, done = (torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(2))
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    att = torch.full((K,), float("nan"), device="cuda")
    resid = rng.standard_normal(rows).astype(np.float32)
    x_out = torch.from_numpy(resid).cuda()
    dw = dev_bytes(to_planar(t, make_matrix(t, rows, K, rng)[0], rows, K))
    ok = hip().attn_wo1(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), dpos.data_ptr(), n_ctx, H, n_kv, hd,
                        1 / np.sqrt(hd), part.data_ptr(), att.data_ptr(), stream(), cnt.data_ptr(), done.data_ptr(),
                        dw.data_ptr(), int(t), rows, K, x_out.data_ptr(), err.data_ptr())
    torch.cuda.synchronize()
    assert ok is False
    assert np.array_equal(x_out.cpu().numpy().view(np.uint32), resid.view(np.uint32))
    assert bool(torch.isnan(att).all()) and int(done.abs().sum()) == 0 and int(err.item()) == 0


# ------------------------------------------------------------------ routed gate/up
def _experts(t, E, F):
    """E experts' gate and up matrices [F][4096] as ggml blocks on the host and, interleaved in 32-row
    groups and stacked, as one planar buffer on the device: (gate raws, up raws, device bytes, stride)."""
    key = ("gu", int(t), E, F)
    if key not in _CACHE:
        K = fr.ROUTE_K
        rng = np.random.default_rng(int(t) * 100 + E + F)
        g = [random_blocks(t, F * K, rng, std=0.05) for _ in range(E)]
        u = [random_blocks(t, F * K, rng, std=0.05) for _ in range(E)]
        planar = [to_planar(t, g[e], F, K, R_dst=2 * F, G=32, off=0) | to_planar(t, u[e], F, K, R_dst=2 * F, G=32, off=32)
                  for e in range(E)]
        _CACHE[key] = (g, u, dev_bytes(np.concatenate(planar)), planar[0].size)
    return _CACHE[key]


def _route_bufs(torch, E, k, tail=4):
    return (torch.full((k + tail,), -7, dtype=torch.int32, device="cuda"), torch.full((k + tail,), -7.0, device="cuda"),
            torch.full((E + tail,), -7.0, device="cuda"))


def _route_out(bufs, E, k):
    ids, wts, lg = (b.cpu().numpy() for b in bufs)
    assert np.all(ids[k:] == -7) and np.all(wts[k:] == -7.0) and np.all(lg[E:] == -7.0), "written past the end"
    return ids[:k], wts[:k], lg[:E]


@pytest.mark.parametrize("t,E,k,F", fr.ROUTE_CASES)
def test_routed_gate_up(torch, t, E, k, F):
    """K = 4096. The router launch and - where gemv_route_fits says the launcher has the routed kernel
    (not at 8192 <= 2 F k < 16384: there it throws, and the engine falls back to exactly the two
    launches checked here) - the routed gate/up: picks, weights and logits bit-equal and within
    rtol 1e-4 / atol 1e-6 of fp64; every SwiGLU feature of both slots against fp64 of q8(rmsnorm(x))
    through the picked experts; routed bit-equal to unrouted; every float past a slot's F features
    keeps its sentinel."""
    K = fr.ROUTE_K
    x, nw, Wr = fr.route_inputs(t, E, k, F)
    g, u, dw, stride = _experts(t, E, F)
    dx, dnw, dWr = (torch.from_numpy(a).cuda() for a in (x, nw, Wr))
    what = (t.name, "E", E, "k", k, "F", F)
    assert hip().moe_router_fused_ok(int(GGMLType.F32), E, K)
    rb = _route_bufs(torch, E, k)
    hip().moe_router_fused(dx.data_ptr(), dnw.data_ptr(), fr.EPS, dWr.data_ptr(), K, E, k, rb[2].data_ptr(),
                           rb[0].data_ptr(), rb[1].data_ptr(), stream())
    torch.cuda.synchronize()
    r_ids, r_wts, r_lg = _route_out(rb, E, k)
    e_w, e_l = fr.check_router(r_ids, r_wts, r_lg, x, nw, Wr, k, what + ("router",))

    def gate_up(**kw):
        out = _nan32(torch, k * (F + PAD) + PAD)
        hip().gemv(dw.data_ptr(), int(t), 2 * F, K, dx.data_ptr(), dnw.data_ptr(), fr.EPS, out.data_ptr(), F, 2, stream(),
                   n_slots=k, expert_stride=stride, slot_stride=F + PAD, **kw)
        torch.cuda.synchronize()
        b = _bits(torch, out)
        assert np.all(b[k * (F + PAD):] == NAN32) and np.all(b[:k * (F + PAD)].reshape(k, F + PAD)[:, F:] == NAN32), \
            (what, "a store past a slot's features")
        return out[:k * (F + PAD)].view(k, F + PAD)[:, :F].contiguous().cpu().numpy()

    ref = [fr.swiglu_rows_ref(x, nw, dequantize(g[e], t, F * K).reshape(F, K), dequantize(u[e], t, F * K).reshape(F, K))
           for e in r_ids]
    plain = gate_up(ids=rb[0].data_ptr())
    e_plain = fr.check_swiglu(plain, ref, what + ("unrouted",))
    fits = hip().gemv_route_fits(int(t), F, k)
    assert fits == fr.route_fits_expected(F, k), (what, "gemv_route_fits", fits)
    qb = _route_bufs(torch, E, k)
    route = dict(route_w=dWr.data_ptr(), route_E=E, route_k=k, route_ids=qb[0].data_ptr(), route_wts=qb[1].data_ptr(),
                 route_logits=qb[2].data_ptr())
    if not fits:   # the launcher agrees with its predicate (a host-side refusal: nothing is launched)
        with pytest.raises(RuntimeError, match="routing needs"):
            gate_up(**route)
        print(f"DECODE_FUSED routed {t.name} E={E} k={k} F={F}: no routed kernel; router wts {e_w:.3g} logits {e_l:.3g}, "
              f"two-launch SwiGLU {e_plain:.3g} (< {fr.SWIGLU})")
        return
    routed = gate_up(**route)
    q_ids, q_wts, q_lg = _route_out(qb, E, k)

    def ulps(a, b):   # (finite values of one sign pattern: the bit patterns' distance)
        return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())

    same = np.array_equal(routed.view(np.uint32), plain.view(np.uint32))
    e_pair = rel_err(routed, plain)
    print(f"DECODE_FUSED routed {t.name} E={E} k={k} F={F}: picks {q_ids.tolist()} / {r_ids.tolist()}, routed against router "
          f"launch: weights {ulps(q_wts, r_wts)} ulp, logits {ulps(q_lg, r_lg)} ulp; router wts {e_w:.3g} logits {e_l:.3g} "
          f"(abs, against fp64); SwiGLU unrouted {e_plain:.3g} (< {fr.SWIGLU}), routed against unrouted bit-equal {same} "
          f"({e_pair:.3g})")
    assert np.array_equal(q_ids, r_ids), (what, q_ids, r_ids)
    assert np.array_equal(q_wts.view(np.uint32), r_wts.view(np.uint32)), (what, "weights", q_wts, r_wts)
    assert np.array_equal(q_lg.view(np.uint32), r_lg.view(np.uint32)), (what, "logits", q_lg, r_lg)
    fr.check_router(q_ids, q_wts, q_lg, x, nw, Wr, k, what + ("routed",))
    e_routed = fr.check_swiglu(routed, ref, what + ("routed",))
    print(f"DECODE_FUSED routed {t.name} E={E} k={k} F={F}: SwiGLU routed {e_routed:.3g} (< {fr.SWIGLU})")
    assert same, (what, "routed and unrouted outputs differ", e_pair)


# ------------------------------------------------------------------ engine level
def _engine(path, graph):
    return hip().Engine(path, n_ctx=256, n_batch=128, device=0, use_graph=graph)


def test_moe_decode_where_the_routed_launch_does_not_fit(torch, tmp_path):
    """One layer, d = 4096, 2 experts top-2, F = 2048: 8192 gate/up rows, the class the launcher has no
    routed kernel for (as Mixtral-8x7B on 4 ranks, F = 3584). The single-row decode runs - the engine
    asks gemv_route_fits and routes with the router launch - and its logits are within the decode
    emulation's 1.5e-2, eager and graph."""
    from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
    spec = replace(SPECS["tiny-mixtral-d4k"], name="tiny-moe2-d4k-f2k", n_ff=2048, n_expert=2, n_expert_used=2)
    assert not hip().gemv_route_fits(int(Q4_K), spec.n_ff, spec.n_expert_used)
    path = write_synthetic_gguf(spec, str(tmp_path / "moe2.gguf"), seed=6)
    toks = [int(t) for t in np.random.default_rng(8).integers(3, 1000, 26)]
    emu = ReferenceLlama(GGUFReader(path), n_ctx=256)
    emu.forward(toks[:20], 0, path="prefill")
    ref = [emu.forward([toks[i]], i, path="decode").numpy() for i in range(20, 26)]
    for graph in (False, True):
        eng = _engine(path, graph)
        eng.eval_logits(toks[:20], 0)
        for j, i in enumerate(range(20, 26)):
            e = rel_err(eng.decode_logits(toks[i], i), ref[j])
            print(f"DECODE_FUSED moe F=2048 graph={graph} pos {i}: {e:.3g} (< 1.5e-2)")
            assert e < 1.5e-2, (graph, i, e)
        assert eng.healthy
        del eng


def test_wo_fuse_switch_past_one_split(torch, tmp_path, monkeypatch):
    """pd-llama-g4 (d = 4096, 32 / 8 heads: the fused launch's shape) at positions 70 .. 75 - two live
    splits, so the merging block writes the attention output and counts done: LFK_WO_FUSE=1 against 0,
    eager and graph, within the 1e-2 of the other switch comparisons (the split-K atomics' order flips
    q8 roundings downstream); no Wo wait timed out (eng.healthy reads its error word). Which launch
    ran is asserted, not supposed: Engine.wo_fused_enqueued counts the layers enqueued through
    attn_wo1 - none with LFK_WO_FUSE=0, every layer of every eager step (of every capture) with 1.
    The prompt is prefilled once and its KV state loaded into the other engines: the prefill is not
    what is compared, and with a prefill each two engines of ONE configuration already differed by
    7.6e-3 .. 9.8e-3 here (120 samples): this model's own run-to-run spread. From the shared state the
    worst comparison measured 7.3e-3 (profiles/decode_fused_test_figures.txt)."""
    path = write_synthetic_gguf("pd-llama-g4", str(tmp_path / "g4.gguf"), seed=3)
    toks = [int(t) for t in np.random.default_rng(4).integers(3, 1000, 76)]
    out, state, n_layer = {}, None, 4
    for mode, graph in (("0", False), ("0", True), ("1", False), ("1", True)):
        monkeypatch.setenv("LFK_WO_FUSE", mode)
        eng = _engine(path, graph)
        assert eng.hparams["n_layer"] == n_layer
        if state is None:
            eng.eval_logits(toks[:70], 0)
            state = eng.kv_save(70)
        else:
            eng.kv_load(state, 70)
        out[(mode, graph)] = [eng.decode_logits(toks[i], i) for i in range(70, 76)]
        assert eng.healthy, (mode, graph)
        n = eng.wo_fused_enqueued
        print(f"DECODE_FUSED LFK_WO_FUSE={mode} graph={graph}: {n} layers enqueued through attn_wo1")
        if mode == "0":
            assert n == 0, (mode, graph, n)
        else:
            assert n >= (n_layer if graph else 6 * n_layer), (mode, graph, n)
        del eng
    base = out[("0", False)]
    for key, lg in out.items():
        errs = [rel_err(b, a) for a, b in zip(base, lg)]
        print(f"DECODE_FUSED LFK_WO_FUSE={key[0]} graph={key[1]}: worst {max(errs):.3g} (< 1e-2)")
        assert all(np.isfinite(b).all() for b in lg) and max(errs) < 1e-2, (key, errs)
