"""fp64 references, inputs and checkers of the single-row decode's two fused launches: the decode
attention with its split-K Wo GEMV (attn_wo1) and the gate/up GEMV that routes the token itself
(GemvArgs::route_w). Needs no GPU: tests/test_decode_fused_ref.py checks the cases' claims (which
branch a shape reaches, the routing margins) and shows the checkers rejecting planted defects;
tests/test_decode_fused_gpu.py runs the kernels against them."""
import numpy as np

from gpu_helpers import q8_emulate, rel_err, rmsnorm
from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from moe_ref import GW_ATOL, GW_RTOL, MARGIN, route_margin, silu_mul
from test_attn_live_keys_gpu import _attn_ref as attn_ref   # fp64 attention over the keys < L

Q4_K, Q6_K, Q8_0 = GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q8_0

# the bounds the suite already applies to the same kernels and references
ATTN = 3e-3      # test_kernels_gpu.py::test_attn_decode
WO = 1e-3        # test_gemv_norm_add_and_resid (EPI_ADD over q8_emulate(x)); also fused against unfused
SWIGLU = 1e-3    # test_gemv_swiglu_interleaved
Q8REF = 2e-4     # test_gemv_types (the q8 reference): routed against unrouted, were they not bit-equal
EPS = 1e-5

# ---------------------------------------------------------------------------- attention + Wo
HD, GQA = 128, 4
# name -> (kv heads, heads, n_ctx, Wo rows, lengths); K = heads * 128
FUSED_CASES = {
    "k2048": (4, 16, 256, 130, (1, 64, 65, 200, 256)),
    "k4096": (8, 32, 256, 4100, (1, 65, 200)),
    "k4096-ctx2048": (8, 32, 2048, 4096, (1500,)),
    "k8192": (16, 64, 128, 2052, (1, 100)),
}
FUSED_PARAMS = [(name, L) for name, c in FUSED_CASES.items() for L in c[4]]
# three launches on one workspace, the number of live splits changing (the k8192 case holds 128 keys)
REPEAT_LENS = {"k2048": (200, 1, 65), "k4096": (200, 1, 65), "k4096-ctx2048": (200, 1, 65), "k8192": (128, 1, 65)}


def fused_geometry(name):
    """attn_wo1's launch shape for a case, as its host code computes it: Wo items (4 rows x one 64-chunk
    K part), Wo blocks (4 items each, at most 512), K parts, attention blocks per grid plane, Wo planes."""
    n_kv, H, n_ctx, rows, _ = FUSED_CASES[name]
    K = H * HD
    kparts = K // 2048
    items = (rows + 3) // 4 * kparts
    n_wo = min((items + 3) // 4, 512)
    splits = (n_ctx + 63) // 64
    per = n_kv * splits
    return dict(K=K, kparts=kparts, items=items, n_wo=n_wo, splits=splits, per=per, planes=(n_wo + per - 1) // per)


def fused_inputs(name, L):
    """q [H][128], the residual [rows] (one draw per case and length) and the case's K / V caches
    [n_kv][n_ctx][128] f16 (one draw per case)."""
    n_kv, H, n_ctx, rows, _ = FUSED_CASES[name]
    seed = sorted(FUSED_CASES).index(name)
    rng = np.random.default_rng(100 + seed)
    Kc = rng.standard_normal((n_kv, n_ctx, HD)).astype(np.float16)
    Vc = rng.standard_normal((n_kv, n_ctx, HD)).astype(np.float16)
    rng = np.random.default_rng(1000 * (seed + 1) + L)
    q = rng.standard_normal((H, HD)).astype(np.float32)
    resid = rng.standard_normal(rows).astype(np.float32)
    return q, resid, Kc, Vc


def poisoned(cache, L):
    """The cache with every row the result must not depend on (rows >= L) as NaN."""
    c = cache.copy()
    c[:, L:] = np.nan
    return c


def wo_ref(W, att):
    """W [rows][K] (dequantised) times the q8-quantised attention output, fp64."""
    return np.asarray(W, np.float64) @ q8_emulate(np.asarray(att, np.float32).reshape(-1)).astype(np.float64)


def check_fused(att, x_out, resid, done, counters, wait_err, att_ref, W, n_kv, what=""):
    """One fused launch's results: the attention output against fp64, x_out - resid against W times
    the q8 of the attention output THE DEVICE holds (a Wo block that read x early, stale or in part
    shows here), the done counters, the split counters and the wait's error word. Returns the two
    relative errors."""
    att, x_out = np.asarray(att, np.float32), np.asarray(x_out, np.float32)
    assert np.all(np.isfinite(att)), (what, "attention output not finite")
    e_att = rel_err(att, att_ref)
    assert e_att < ATTN, (what, "attention", e_att)
    assert np.all(np.isfinite(x_out)), (what, "x_out not finite: a Wo block read x before it was written")
    e_wo = rel_err(x_out.astype(np.float64) - resid, wo_ref(W, att))
    assert e_wo < WO, (what, "Wo", e_wo)
    done = np.asarray(done)
    assert done.shape == (64,) and np.all(done[:n_kv] == 1) and np.all(done[n_kv:] == 0), (what, "done", done)
    assert np.all(np.asarray(counters) == 0), (what, "split counters", counters)
    assert int(wait_err) == 0, (what, "wait_err", wait_err)
    return e_att, e_wo


# ---------------------------------------------------------------------------- routed gate/up
ROUTE_K = 4096
# (expert type, E, k, F). E = 2, k = 2: rows = 4 F - one case per configuration class of the launcher
# (below 8192, 8192 .. 16383, from 16384), F = 96 a ragged one; Q6_K once; E = 8 is the engine's count
ROUTE_CASES = [(Q4_K, 2, 2, 96), (Q4_K, 2, 2, 2048), (Q4_K, 2, 2, 4096), (Q6_K, 2, 2, 96), (Q4_K, 8, 2, 256)]
# seeds of route_inputs, fixed here from the fp64 conditions of route_conditions alone
ROUTE_SEEDS = {(int(Q4_K), 2, 2, 96): 11, (int(Q4_K), 2, 2, 2048): 12, (int(Q4_K), 2, 2, 4096): 13,
               (int(Q6_K), 2, 2, 96): 14, (int(Q4_K), 8, 2, 256): 16}
# every |logit| is at least this. test_moe_router_rows_vs_fp64's rtol 1e-4 / atol 1e-6 was written for
# the routing WEIGHTS (probabilities); this file applies it to the logits too. A logit is an f32 dot
# product over 4096 terms of sum |n_i w_i| ~ 130, whose absolute rounding (~1e-6 .. 1e-5) does not
# shrink with its value, so near a zero logit the bound would judge that rounding and not the kernel.
# The seeds are therefore chosen (from fp64 alone, before any device result) so that |v| >= 0.25,
# where the bound is 2.6e-5 and relative, as it is for the weights. A condition on the inputs
# beyond what the routing margin asks: it narrows the cases, it does not widen the bound
MIN_LOGIT = 0.25


def route_fits_expected(F, k):
    """The launcher's classes at K = 4096 for the K-quants: the routed kernel exists below 8192 gate/up
    rows ((2, 2) items) and from 16384 ((4, 1)), not between ((4, 2))."""
    rows = 2 * F * k
    return rows < 8192 or rows >= 16384


def route_inputs(t, E, k, F):
    rng = np.random.default_rng(ROUTE_SEEDS[(int(t), E, k, F)])
    x = (3 * rng.standard_normal(ROUTE_K)).astype(np.float32)
    nw = (1 + 0.1 * rng.standard_normal(ROUTE_K)).astype(np.float32)
    Wr = (0.05 * rng.standard_normal((E, ROUTE_K))).astype(np.float32)
    return x, nw, Wr


def router_ref(x, nw, Wr, k, eps=EPS):
    """fp64 of the f32 inputs: logits [E], the k picks in rank order (lowest index on ties) and
    their renormalised weights."""
    xs = np.asarray(x, np.float64)
    n = xs / np.sqrt(np.mean(xs * xs) + eps) * np.asarray(nw, np.float64)
    lg = np.asarray(Wr, np.float64) @ n
    p = np.exp(lg - lg.max())
    p /= p.sum()
    ids = np.argsort(-p, kind="stable")[:k]
    return lg, ids, p[ids] / p[ids].sum()


def route_conditions(x, nw, Wr, k):
    """(relative margin between neighbouring probabilities among the top k + 1, smallest |logit|)."""
    lg, _, _ = router_ref(x, nw, Wr, k)
    return route_margin(lg[None].astype(np.float32), k), float(np.abs(lg).min())


def check_router(ids, wts, logits, x, nw, Wr, k, what=""):
    lg, rid, rw = router_ref(x, nw, Wr, k)
    assert list(np.asarray(ids)) == list(rid), (what, "picks", list(ids), list(rid))
    np.testing.assert_allclose(np.asarray(wts, np.float64), rw, rtol=GW_RTOL, atol=GW_ATOL, err_msg=str(what))
    np.testing.assert_allclose(np.asarray(logits, np.float64), lg, rtol=GW_RTOL, atol=GW_ATOL, err_msg=str(what))
    return float(np.abs(np.asarray(wts) - rw).max()), float(np.abs(np.asarray(logits) - lg).max())


def swiglu_rows_ref(x, nw, Wg, Wu, eps=EPS):
    """silu(Wg xq) * (Wu xq) in fp64 over xq = q8_emulate(rmsnorm(x) * nw); Wg / Wu [F][K]: one
    expert's gate and up matrices (ggml blocks or dequantised)."""
    xq = q8_emulate(rmsnorm(x, nw, eps)).astype(np.float64)
    return silu_mul(np.asarray(Wg, np.float64) @ xq, np.asarray(Wu, np.float64) @ xq)


def check_swiglu(out, ref_slots, what=""):
    """out [k][F] against the fp64 rows of the picked experts, slot by slot (every feature). Returns
    the worst slot's relative error."""
    out = np.asarray(out, np.float32)
    assert np.all(np.isfinite(out)), (what, "non-finite SwiGLU output")
    worst = 0.0
    for s, ref in enumerate(ref_slots):
        e = rel_err(out[s], ref)
        assert e < SWIGLU, (what, "slot", s, e)
        worst = max(worst, e)
    return worst
