"""CPU self-test of tests/moe_ref.py: the checkers accept the fp64 reference plus noise at a tenth of
each bound and reject single planted defects of the kinds the MoE kernels could have, and every
routing input of the GPU tests satisfies the margin precondition."""
import numpy as np
import pytest

import moe_ref as mr


def _noisy(ref, bound, rng, frac=0.1):
    """ref plus noise whose norm is frac * bound of every row's."""
    n = rng.standard_normal(ref.shape)
    n *= (frac * bound * np.linalg.norm(ref, axis=-1, keepdims=True)) / np.linalg.norm(n, axis=-1, keepdims=True)
    return ref + n


@pytest.fixture(scope="module")
def grouped():
    """One grouped case in fp64: T = 300 tokens, E = 4, k = 2, the (65, 128, 107, 300) pattern."""
    rng = np.random.default_rng(1)
    T, counts = mr.GROUP_PATTERNS[3]
    d, F, E = 64, 64, 4
    lg = mr.logits_for_counts(T, counts, 5)
    rt = mr.route_reference(lg, 2)
    assert tuple(np.diff(rt.cnt_off)) == counts
    x = rng.standard_normal((T, d))
    Wgu = [0.1 * rng.standard_normal((2 * F, d)) for _ in range(E)]
    Wd = [0.1 * rng.standard_normal((d, F)) for _ in range(E)]
    xg = x[rt.tok]
    h = np.zeros((2 * T, F))
    for e in range(E):
        r0, r1 = rt.cnt_off[e], rt.cnt_off[e + 1]
        h[r0:r1] = mr.swiglu_ref(xg[r0:r1], Wgu[e])
    return dict(T=T, E=E, d=d, F=F, rt=rt, x=x, xg=xg, Wgu=Wgu, Wd=Wd, h=h)


@pytest.mark.parametrize("bound", [mr.T16_GU, mr.T16_DN, mr.DQ_GU, mr.DQ_DN, mr.BMM_GU, mr.BMM_DN])
def test_check_rows_accepts_noise_at_a_tenth(grouped, bound):
    rng = np.random.default_rng(2)
    frac = mr.check_rows(_noisy(grouped["h"], bound, rng), grouped["h"], bound)
    assert 0.09 < frac < 0.11


def test_check_rows_rejects_one_wrong_row_among_300(grouped):
    """A single row at twice the bound fails although the whole array's norm error is ~bound / 12."""
    rng = np.random.default_rng(3)
    h = grouped["h"]
    got = _noisy(h, mr.T16_GU, rng)
    got[417] = _noisy(h[417:418], mr.T16_GU, rng, frac=2.0)[0]
    assert np.linalg.norm(got - h) / np.linalg.norm(h) < mr.T16_GU
    with pytest.raises(AssertionError, match="417"):
        mr.check_rows(got, h, mr.T16_GU)


def test_rejects_neighbouring_group_row_overwritten(grouped):
    """Expert 1's launch also stores the row past its group: the first row of expert 2's."""
    rt, h, F = grouped["rt"], grouped["h"], grouped["F"]
    rows, ld = 2 * grouped["T"] + 16, F + 8
    sent = np.full((rows, ld), mr.NAN16, np.uint16).view(np.float16)
    r0, r1 = rt.cnt_off[1], rt.cnt_off[2]
    got = sent.copy()
    got[r0:r1, :F] = h[r0:r1]
    mr.check_group_untouched(got, sent, r0, r1, F)
    got[r1, :F] = h[r1 - 1]
    with pytest.raises(AssertionError, match=rf"\({r1}, 0\)"):
        mr.check_group_untouched(got, sent, r0, r1, F)
    # ... the slack row past the last group, and a pad column inside the group
    r0, r1 = rt.cnt_off[3], rt.cnt_off[4]
    got = sent.copy()
    got[r0:r1, :F] = h[r0:r1]
    got[r1, 3] = 1.0
    with pytest.raises(AssertionError, match=rf"\({r1}, 3\)"):
        mr.check_group_untouched(got, sent, r0, r1, F)
    got[r1, 3] = sent[r1, 3]
    got[r0 + 2, F + 1] = 0.0
    with pytest.raises(AssertionError, match=rf"\({r0 + 2}, {F + 1}\)"):
        mr.check_group_untouched(got, sent, r0, r1, F)
    # the zero sentinel of the pre-zeroed split-K output: a -0.0 is a touch too
    z = np.zeros((8, 8), np.float32)
    g = z.copy()
    g[5, 1] = -0.0
    with pytest.raises(AssertionError, match=r"\(5, 1\)"):
        mr.check_group_untouched(g, z, 0, 4, 8)


def test_rejects_group_shifted_by_a_row(grouped):
    rt, h = grouped["rt"], grouped["h"]
    r0, r1 = rt.cnt_off[2], rt.cnt_off[3]
    mr.check_rows(h[r0:r1], h[r0:r1], mr.DQ_GU)
    with pytest.raises(AssertionError):
        mr.check_rows(h[r0 + 1:r1 + 1], h[r0:r1], mr.DQ_GU)   # the loosest bound


def test_rejects_routing_weight_dropped_from_one_row(grouped):
    rt, T = grouped["rt"], grouped["T"]
    rng = np.random.default_rng(4)
    d = grouped["d"]
    y = np.concatenate([mr.down_ref(grouped["h"][rt.cnt_off[e]:rt.cnt_off[e + 1]], grouped["Wd"][e]) for e in range(4)])
    acc0 = rng.standard_normal((T, d))
    terms = np.stack([rt.gw[rt.pos.reshape(T, 2)[:, j]][:, None] * y[rt.pos.reshape(T, 2)[:, j]] for j in range(2)])
    ref = acc0 + terms.sum(0)
    bound = mr.scatter_bound(acc0, terms)
    got = (acc0.astype(np.float32) + terms[0].astype(np.float32) + terms[1].astype(np.float32)).astype(np.float64)
    # (the fp32 rounding of the inputs themselves is not the kernel's: compare like with like)
    ref32 = acc0.astype(np.float32).astype(np.float64) + terms[0].astype(np.float32).astype(np.float64) \
        + terms[1].astype(np.float32).astype(np.float64)
    assert np.all(np.abs(got - ref32) <= bound)
    bad = got.copy()
    bad[123] = acc0[123] + y[rt.pos[2 * 123]] * 1.0 + terms[1][123]   # slot 0's weight dropped
    assert np.any(np.abs(bad - ref) > bound)
    # and through the whole FFN's per-row check
    full = mr.moe_ffn_ref(grouped["x"], grouped["Wgu"], grouped["Wd"], rt, 2)
    np.testing.assert_allclose(full, terms.sum(0), rtol=1e-9, atol=1e-12)
    bad = full.copy()
    bad[123] = y[rt.pos[2 * 123]] + terms[1][123]
    with pytest.raises(AssertionError, match="123"):
        mr.check_rows(bad, full, mr.DQ_GU + mr.DQ_DN)


def test_rejects_tie_resolved_to_the_higher_index():
    hit = 0
    for T, E, k, kind in mr.ROUTE_CASES:
        lg = mr.routing_logits(T, E, k, kind, mr.route_seed(T, E, k, kind))
        ref = mr.route_reference(lg, k)
        good = dict(sel=ref.sel.astype(np.int32), selw=ref.selw.astype(np.float32), cnt_off=ref.cnt_off.astype(np.int32),
                    tok=ref.tok.astype(np.int32), gw=ref.gw.astype(np.float32), pos=ref.pos.astype(np.int32))
        mr.check_routing(good, ref, T, E, k)
        hi = mr.route_reference(lg, k, tie_high=True)
        if kind == "random" and T > 3:
            assert list(ref.sel[3]) == list(range(k))     # the all-equal row: experts 0 .. k - 1
            bad = dict(good, sel=hi.sel.astype(np.int32), cnt_off=hi.cnt_off.astype(np.int32),
                       tok=hi.tok.astype(np.int32), pos=hi.pos.astype(np.int32))
            with pytest.raises(AssertionError):
                mr.check_routing(bad, ref, T, E, k)
            hit += 1
    assert hit == 5


def test_routing_weights_at_a_tenth_of_the_router_bound_pass_and_ten_times_fail():
    T, E, k = 40, 4, 2
    lg = mr.routing_logits(T, E, k, "random", mr.route_seed(T, E, k, "random"))
    ref = mr.route_reference(lg, k)
    good = dict(sel=ref.sel, selw=ref.selw * (1 + 0.1 * mr.GW_RTOL), cnt_off=ref.cnt_off, tok=ref.tok,
                gw=ref.gw * (1 - 0.1 * mr.GW_RTOL), pos=ref.pos)
    mr.check_routing(good, ref, T, E, k)
    gw = ref.gw.copy()
    gw[17] *= 1 + 10 * mr.GW_RTOL
    with pytest.raises(AssertionError):
        mr.check_routing(dict(good, gw=gw), ref, T, E, k)
    tok = ref.tok.copy()
    tok[[4, 5]] = tok[[5, 4]]     # two rows of a group out of token order
    with pytest.raises(AssertionError, match="tok"):
        mr.check_routing(dict(good, tok=tok), ref, T, E, k)


def test_routing_inputs_meet_the_margin_precondition():
    for T, E, k, kind in mr.ROUTE_CASES:
        lg = mr.routing_logits(T, E, k, kind, mr.route_seed(T, E, k, kind))
        assert lg.dtype == np.float32 and lg.shape == (T, E)
        assert mr.route_margin(lg, k) >= mr.MARGIN, (T, E, k, kind)
        cnt = np.diff(mr.route_reference(lg, k).cnt_off)
        if kind == "empty":
            assert cnt[1] == 0
        if kind == "one":
            assert cnt[E - 2] == T
    for i, (T, counts) in enumerate(mr.GROUP_PATTERNS):
        lg = mr.logits_for_counts(T, counts, 50 + i)
        assert mr.route_margin(lg, 2) >= mr.MARGIN
        assert tuple(np.diff(mr.route_reference(lg, 2).cnt_off)) == counts


@pytest.fixture(scope="module")
def batched():
    rng = np.random.default_rng(6)
    B, E, d, F = 6, 8, 32, 64
    x = rng.standard_normal((B, d))
    Wgu = [0.2 * rng.standard_normal((2 * F, d)) for _ in range(E)]
    Wd = [0.2 * rng.standard_normal((d, F)) for _ in range(E)]
    return dict(B=B, E=E, d=d, F=F, x=x, Wgu=Wgu, Wd=Wd)


def _gu_bits(h, sent_bits, E, F):
    """The kernel's h_out for reference h: f16, 4-group order, NaN columns left as the sentinel."""
    got = sent_bits.copy()
    hs = mr.swizzle4(np.where(np.isnan(h), 0, h)).astype(np.float16).view(np.uint16)
    keep = ~np.isnan(h)
    got[:, :E * F][keep] = hs[keep]
    return got


def test_batched_checkers_accept_and_reject(batched):
    B, E, d, F = (batched[k] for k in ("B", "E", "d", "F"))
    rng = np.random.default_rng(7)
    for name, ew in mr.ew_patterns(B, E, 11):
        h = mr.bmm_gu_ref(batched["x"], batched["Wgu"], ew)
        sent = np.full((B, E * F + 8), mr.NAN16, np.uint16)
        active = [e for e in range(E) if np.any(ew[:, e] != 0)]
        got = _gu_bits(h, sent, E, F)
        mr.check_bmm_gu(got, sent, h, ew, F, name)          # f16 rounding alone: far inside the bound
        # the routing weight replaced by 1 in one routed block
        b, e = [(b, e) for e in active for b in range(B) if ew[b, e] not in (0.0, 1.0)][:1][0] if name != "first" else (0, 0)
        if ew[b, e] != 1.0:
            bad = got.copy()
            blk = mr.swizzle4(h[b, e * F:(e + 1) * F] / ew[b, e]).astype(np.float16).view(np.uint16)
            bad[b, e * F:(e + 1) * F] = blk
            with pytest.raises(AssertionError):
                mr.check_bmm_gu(bad, sent, h, ew, F, name)
        # an unrouted row's block under an active expert not zeroed
        zero = [(b, e) for e in active for b in range(B) if ew[b, e] == 0]
        if zero:
            b, e = zero[0]
            bad = got.copy()
            bad[b, e * F + 5] = np.float16(1e-3).view(np.uint16)
            with pytest.raises(AssertionError, match="not zero"):
                mr.check_bmm_gu(bad, sent, h, ew, F, name)
        # a skipped expert's columns written
        idle = [e for e in range(E) if e not in active]
        if idle:
            bad = got.copy()
            bad[0, idle[0] * F + 2] = 0
            with pytest.raises(AssertionError, match="touched"):
                mr.check_bmm_gu(bad, sent, h, ew, F, name)
        # the down projection over the device's h: reference plus noise at a tenth of the bound
        hd = mr.swizzle4(got[:, :E * F].view(np.float16).astype(np.float64))
        ref = mr.bmm_down_ref(hd, batched["Wd"], ew)
        live = np.linalg.norm(ref, axis=1) > 0
        mr.check_rows(_noisy(ref[live], mr.BMM_DN, rng), ref[live], mr.BMM_DN)
        # an unrouted expert's columns fed to the down projection (finite garbage in place of the
        # poison: with the NaN pattern itself the output is non-finite, rejected as such)
        if idle:
            e = idle[0]
            leak = ref + 0.05 * rng.standard_normal((B, F)) @ batched["Wd"][e].T
            with pytest.raises(AssertionError):
                mr.check_rows(leak[live], ref[live], mr.BMM_DN)
            with pytest.raises(AssertionError, match="non-finite"):
                mr.check_rows(ref[live] + np.nan, ref[live], mr.BMM_DN)
        # one K part of the down attributed to the next expert
        e = active[0]
        wrong = mr.bmm_down_ref(hd, batched["Wd"], ew, part=(e, F // 2, F))
        with pytest.raises(AssertionError):
            mr.check_rows(wrong[live], ref[live], mr.BMM_DN)


def test_scatter_bound_holds_for_fp32_sums_and_is_tight():
    rng = np.random.default_rng(8)
    for k in (1, 2, 8):
        acc0 = rng.standard_normal((50, 33)).astype(np.float32)
        terms = rng.standard_normal((k, 50, 33)).astype(np.float32)
        v = np.zeros_like(acc0)
        for j in range(k):
            v = v + terms[j]
        got = (acc0 + v).astype(np.float64)
        ref = acc0.astype(np.float64) + terms.astype(np.float64).sum(0)
        bound = mr.scatter_bound(acc0.astype(np.float64), terms.astype(np.float64))
        assert np.all(np.abs(got - ref) <= bound)
        assert np.all(bound < 1e-5 * (1 + np.abs(ref)) * (k + 1))   # tight: a dropped term is ~1
