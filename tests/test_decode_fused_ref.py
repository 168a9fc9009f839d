"""CPU self-test of tests/decode_fused_ref.py: the cases reach the branches they are there for, every
routed case meets the routing preconditions (none left out), and the checkers reject planted
defects - an early or stale x, a miscounted done word, a tie resolved upwards, a swapped expert."""
import numpy as np
import pytest

import decode_fused_ref as fr
import moe_ref as mr
from gpu_helpers import make_matrix, q8_emulate


def test_fused_cases_reach_their_branches():
    g = {n: fr.fused_geometry(n) for n in fr.FUSED_CASES}
    a, b, c, d = g["k2048"], g["k4096"], g["k4096-ctx2048"], g["k8192"]
    # one K part, a ragged last 4-row group, fewer Wo blocks than one grid plane holds
    assert a["kparts"] == 1 and fr.FUSED_CASES["k2048"][3] % 4 and a["n_wo"] == 9 < a["per"] == 16 and a["planes"] == 1
    # two K parts adding into one row; more items than 512 blocks x 4 waves: a grid-stride second item
    assert b["kparts"] == 2 and b["items"] == 2050 > 4 * b["n_wo"] == 2048
    # 32 launched splits, 24 live ones at L = 1500 (two merge batches of 16), two Wo planes
    assert c["splits"] == 32 and (1500 + 63) // 64 == 24 > 16 and c["planes"] == 2
    assert d["kparts"] == 4 and d["items"] == 2052 and d["planes"] == 16
    for name, (n_kv, H, n_ctx, rows, lens) in fr.FUSED_CASES.items():
        assert H == fr.GQA * n_kv and (H * fr.HD) % 2048 == 0 and n_kv <= 64
        assert rows * H * fr.HD * 210 // 256 <= 14 << 20           # Q6_K bytes
        assert all(1 <= L <= n_ctx for L in lens + fr.REPEAT_LENS[name])
    # both done branches (one live split: store and count; more: the last arriver merges), L = n_ctx
    lens = fr.FUSED_CASES["k2048"][4]
    assert min(lens) <= 64 < max(lens) and 65 in lens and max(lens) == fr.FUSED_CASES["k2048"][2]
    for name in ("k4096", "k8192"):
        assert min(fr.FUSED_CASES[name][4]) <= 64 < max(fr.FUSED_CASES[name][4])


def test_route_cases_cover_the_launcher_classes():
    e2 = [(F, fr.route_fits_expected(F, k)) for t, E, k, F in fr.ROUTE_CASES if E == 2 and t == fr.Q4_K]
    assert e2 == [(96, True), (2048, False), (4096, True)]
    assert [4 * F for F, _ in e2] == [384, 8192, 16384]            # the class edges themselves
    assert fr.route_fits_expected(3584, 2) is False                # Mixtral-8x7B's F on 4 ranks
    assert any(t == fr.Q6_K for t, *_ in fr.ROUTE_CASES) and (fr.Q4_K, 8, 2, 256) in fr.ROUTE_CASES
    for t, E, k, F in fr.ROUTE_CASES:
        assert F % 32 == 0 and E * 2 * F * fr.ROUTE_K <= 70e6 and (int(t), E, k, F) in fr.ROUTE_SEEDS


@pytest.mark.parametrize("t,E,k,F", fr.ROUTE_CASES)
def test_route_case_preconditions(t, E, k, F):
    """No f32 rounding flips a pick (or the picks' order), and no logit is so small that the router
    bound's absolute term would be judging an f32 dot product's rounding."""
    margin, min_logit = fr.route_conditions(*fr.route_inputs(t, E, k, F), k)
    print(f"DECODE_FUSED route E={E} k={k} F={F} {t.name}: margin {margin:.3g} min |logit| {min_logit:.3g}")
    assert margin >= mr.MARGIN and min_logit >= fr.MIN_LOGIT


def test_router_ref_ties_and_check():
    rng = np.random.default_rng(0)
    x, nw = rng.standard_normal(fr.ROUTE_K).astype(np.float32), np.ones(fr.ROUTE_K, np.float32)
    row = (0.01 * x).astype(np.float32)
    Wr = np.stack([row * 0.5, row, row, -row])                     # experts 1 and 2 tie at the top
    lg, ids, w = fr.router_ref(x, nw, Wr, 2)
    assert lg[1] == lg[2] > lg[0] > lg[3] and list(ids) == [1, 2]
    x, nw, Wr = fr.route_inputs(fr.Q4_K, 8, 2, 256)
    lg, ids, w = fr.router_ref(x, nw, Wr, 2)
    assert abs(w.sum() - 1) < 1e-12 and w[0] > w[1]
    fr.check_router(ids, w.astype(np.float32), lg.astype(np.float32), x, nw, Wr, 2)
    with pytest.raises(AssertionError):                            # the picks in the wrong order
        fr.check_router(ids[::-1], w[::-1], lg, x, nw, Wr, 2)
    with pytest.raises(AssertionError):                            # weights not renormalised
        fr.check_router(ids, w * 0.999, lg, x, nw, Wr, 2)
    with pytest.raises(AssertionError):                            # a logit of the unnormalised x
        fr.check_router(ids, w, lg * 1.001, x, nw, Wr, 2)


def test_swiglu_rows_ref_and_subset():
    rng = np.random.default_rng(1)
    F, K = 64, 512
    (rg, Wg), (ru, Wu) = make_matrix(fr.Q4_K, F, K, rng), make_matrix(fr.Q4_K, F, K, rng)
    x = (3 * rng.standard_normal(K)).astype(np.float32)
    nw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    ref = fr.swiglu_rows_ref(x, nw, Wg, Wu)
    # the same through moe_ref's reference over the interleaved (32-row groups) matrix
    inter = np.concatenate([np.concatenate([Wg[i:i + 32], Wu[i:i + 32]]) for i in range(0, F, 32)])
    from gpu_helpers import rmsnorm
    assert np.allclose(ref, mr.swiglu_ref(q8_emulate(rmsnorm(x, nw))[None], inter)[0], rtol=1e-12, atol=0)
    out = np.stack([ref, ref]).astype(np.float32)
    fr.check_swiglu(out, [ref, ref])
    bad = out.copy()
    bad[1] = fr.swiglu_rows_ref(x, nw, Wu, Wg)                       # gate and up swapped in one slot
    with pytest.raises(AssertionError):
        fr.check_swiglu(bad, [ref, ref])
    bad = out.copy()
    bad[0, 33] = ref[34]                                             # one feature from its neighbour's rows
    with pytest.raises(AssertionError):
        fr.check_swiglu(bad, [ref, ref])


def _fused_ok(name="k2048", L=65):
    n_kv, H, n_ctx, rows, _ = fr.FUSED_CASES[name]
    q, resid, Kc, Vc = fr.fused_inputs(name, L)
    _, W = make_matrix(fr.Q4_K, rows, H * fr.HD, np.random.default_rng(3))
    ref = fr.attn_ref(q, Kc, Vc, L, 1 / np.sqrt(fr.HD))
    att = ref.astype(np.float32)
    x_out = (resid + fr.wo_ref(W, att)).astype(np.float32)
    done = np.zeros(64, np.int32)
    done[:n_kv] = 1
    return dict(att=att, x_out=x_out, resid=resid, done=done, counters=np.zeros(64, np.int32), wait_err=0,
                att_ref=ref, W=W, n_kv=n_kv), (q, Kc, Vc, L)


def test_check_fused_rejects_planted_defects():
    ok, (q, Kc, Vc, L) = _fused_ok()
    fr.check_fused(**ok)
    # the reference ignores what lies at and beyond L
    assert np.array_equal(fr.attn_ref(q, fr.poisoned(Kc, L), fr.poisoned(Vc, L), L, 1 / np.sqrt(fr.HD)), ok["att_ref"])
    W, att, resid = ok["W"], ok["att"], ok["resid"]

    def bad(**kw):
        with pytest.raises(AssertionError):
            fr.check_fused(**{**ok, **kw})

    early = att.copy()
    early[4:8] = np.nan                                            # Wo read kv head 1 before it was written
    bad(x_out=(resid + fr.wo_ref(W, early)).astype(np.float32))
    stale = att.copy()
    stale[4:8] = fr.attn_ref(q, Kc, Vc, 1, 1 / np.sqrt(fr.HD))[4:8]  # ... or its outputs of an earlier launch
    bad(x_out=(resid + fr.wo_ref(W, stale)).astype(np.float32))
    part = (resid + fr.wo_ref(W[:, :1024], att.reshape(-1)[:1024])).astype(np.float32)
    bad(x_out=part)                                                # half of the one K part
    lost = ok["x_out"].copy()
    lost[128:] = resid[128:]                                       # the ragged last group not written
    bad(x_out=lost)
    bad(att=(att * 1.01).astype(np.float32))                       # a wrong attention, Wo consistent with it or not
    twice = ok["done"].copy()
    twice[0] = 2
    bad(done=twice)
    spill = ok["done"].copy()
    spill[ok["n_kv"]] = 1
    bad(done=spill)
    left = np.zeros(64, np.int32)
    left[1] = 3
    bad(counters=left)
    bad(wait_err=1)
