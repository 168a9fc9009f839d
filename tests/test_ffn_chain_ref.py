"""CPU self-test of tests/ffn_chain_ref.py: the plan mirror gives the part counts the suite already
records and those of the GPU cases' table, the checkers accept the clean reference and the kernels'
number formats emulated on the CPU (under half of each bound), and reject single planted defects
of the kinds the chains' hand-off could have. The defects are planted at F = 7936, K = 512 (ten parts
of 3 steps and a 1-step last part): the longest row of the GPU cases, where one part, one tile or one
element is smallest relative to the row."""
import numpy as np
import pytest

import ffn_chain_ref as cr
import moe_ref as mr

CUS = 256   # the part counts written down in the suite and the issue's table are the MI355X's


# ---------------------------------------------------------------------------- chain_plan
def test_plan_matches_the_recorded_counts():
    """test_bmm_ffn_chain_matches_two_launches asserts 8 parts x 224 tiles on the 8B shape; the
    quarter shape F = K = 4096 of the transposed tests runs 8 parts of 2 steps."""
    p = cr.chain_plan(14336, 4096, CUS)
    assert (p.kparts, p.spp, p.part_tiles, p.n1, p.n2) == (8, 7, [224] * 8, 256, 256) and not p.ragged
    p = cr.chain_plan(4096, 4096, CUS)
    assert (p.kparts, p.part_steps) == (8, [2] * 8)


@pytest.mark.parametrize("d,F,parts", [
    (512, 512, [2]), (512, 1280, [3, 2]), (512, 3328, [3, 3, 3, 3, 1]), (512, 7936, [3] * 10 + [1]),
    (512, 7680, [2] * 15), (4096, 1280, [3, 2]), (4096, 2816, [3, 3, 3, 2]), (512, 8192, [2] * 16),
    (4096, 512, [2]), (4096, 1024, [2, 2]), (4096, 4096, [2] * 8),
    # the real models of the issue: Llama-2-7B, Qwen2.5-7B, Llama-3.2-3B, Qwen3-4B, Qwen2.5-3B, Llama-3.2-1B
    (4096, 11008, [6] * 7 + [1]), (3584, 18944, [9] * 8 + [2]), (3072, 8192, [3] * 10 + [2]),
    (2560, 9728, [3] * 12 + [2]), (2048, 11008, [3] * 14 + [1]), (2048, 8192, [2] * 16)])
def test_plan_of_the_case_table(d, F, parts):
    p = cr.chain_plan(F, d, CUS)
    assert p.part_steps == parts and p.kparts == len(parts) and sum(p.part_tiles) == F // 8
    assert p.ragged == (parts[-1] != parts[0])
    assert p.n1 == min(CUS, F // 8) and p.n2 % p.kparts == 0 and p.n2 <= max(CUS, p.kparts)


def test_case_lists_are_what_they_claim():
    plans = {(K, F): cr.chain_plan(F, K, CUS) for K, F, _ in cr.CHAIN_SHAPES}
    assert all(cr.chain_takes(p) for p in plans.values())
    assert max(p.kparts for p in plans.values()) == cr.STAGED_PART
    assert all(plans[K, F].ragged for K, F, _ in cr.TR_SHAPES)
    assert sum(p.part_steps[-1] == 1 and p.kparts > 1 for p in plans.values()) >= 2    # 1-step tails
    assert not any(cr.chain_takes(cr.chain_plan(F, K, CUS)) for K, F in cr.CHAIN_REFUSED)
    assert 60 <= len(cr.CHAIN_CASES) <= 80 and len(set(cr.CHAIN_CASES)) == len(cr.CHAIN_CASES)
    for td, F, Kwo, B in cr.WO_CASES:
        assert cr.wo_chain_takes(cr.chain_plan(Kwo, 4096, CUS), cr.chain_plan(F, 4096, CUS))
    assert cr.chain_plan(1024, 4096, CUS).kparts == 2
    for F, Kwo in cr.WO_REFUSED:
        assert not cr.wo_chain_takes(cr.chain_plan(Kwo, 4096, CUS), cr.chain_plan(F, 4096, CUS))


def test_check_counters():
    p = cr.chain_plan(3328, 512, CUS)
    good = np.zeros((cr.MAX_PARTS, 8, 32), np.int32)
    for kp, t in enumerate(p.part_tiles):
        good[kp, :, 0] = [t // 8 + (i < t % 8) for i in range(8)]
    good[cr.STAGED_PART, 3, 0] = p.n1
    cr.check_counters(cr.counters_per_part(good, 32, 8), p)
    for part, shard, delta in ((4, 0, -1), (4, 7, 1), (5, 2, 1), (cr.STAGED_PART, 0, -1), (cr.WO_PART, 0, 1)):
        bad = good.copy()
        bad[part, shard, 0] += delta
        with pytest.raises(AssertionError, match="counters"):
            cr.check_counters(cr.counters_per_part(bad, 32, 8), p)
    bad = good.copy()
    bad[0, 0, 5] = 1
    with pytest.raises(AssertionError, match="padding"):
        cr.counters_per_part(bad, 32, 8)
    wo = good.copy()
    wo[cr.WO_PART, 1, 0] = 64
    cr.check_counters(cr.counters_per_part(wo, 32, 8), p, wo_blocks=64)


# ---------------------------------------------------------------------------- planted defects
F, K, B = 7936, 512, 5


class _Case:
    """The chain of one case in fp64, part by part, so that single defects can be planted: h = the
    f16 of the reference rows, out = resid + the parts' partial sums over that h."""

    def __init__(self, norm=False):
        rng = np.random.default_rng(11)
        self.norm = norm
        self.plan = cr.chain_plan(F, K, CUS)
        assert self.plan.part_steps == [3] * 10 + [1]
        self.Wgu = 0.05 * rng.standard_normal((2 * F, K))
        self.Wd = 0.05 * rng.standard_normal((K, F))
        self.X, self.nw, self.resid = cr.chain_rows(K, B, norm, 12)
        self.h_ref = cr.h_reference(self.X, self.nw, self.Wgu, norm)

    def pre(self):
        """Gate and up pre-activations [B][F] each, natural feature order."""
        x = cr.staged_x(self.X, self.nw, cr.EPS, "folded" if self.norm else "xh")
        p = (x @ self.Wgu.T).reshape(B, F // 32, 2, 32)
        return p[:, :, 0].reshape(B, F), p[:, :, 1].reshape(B, F)

    def run(self, h=None, parts=None, twice=None, h_of_part=None, store=False):
        """h: the rows the producer wrote (default: the reference); parts: the K parts summed
        (default: all); twice: a part added a second time; h_of_part {kp: rows}: what that part's
        consumer read instead of h; store: the result overwrites the residual."""
        h = self.h_ref if h is None else h
        hb = np.full((B + 1, F), mr.NAN16, np.uint16)
        hb[:B] = cr.h_bits_of(h)
        hv = cr.h_values(hb[:B])
        out = self.resid.astype(np.float64)
        if store:
            out[:B] = 0
        todo = list(range(self.plan.kparts) if parts is None else parts) + ([twice] if twice is not None else [])
        for kp in todo:
            c = slice(256 * 3 * kp, 256 * (3 * kp + self.plan.part_steps[kp]))
            src = hv if not (h_of_part and kp in h_of_part) else h_of_part[kp]
            out[:B] += src[:, c] @ self.Wd[:, c].T
        return hb, out.astype(np.float32)

    def check(self, hb, out):
        return cr.check_chain(hb, out, self.resid, self.h_ref, self.Wd, "case")


@pytest.fixture(scope="module")
def case():
    return _Case()


def test_clean_reference_passes(case):
    fh, fd = case.check(*case.run())
    assert fh < 0.15 and fd < 0.01, (fh, fd)    # the f16 rounding of h; the fp32 rounding of out


def test_rejects_last_part_dropped(case):
    """The 1-step last part (256 of 7936 features) never summed - a consumer that took need = 0."""
    with pytest.raises(AssertionError, match="down"):
        case.check(*case.run(parts=range(case.plan.kparts - 1)))


def test_rejects_part_summed_from_the_sentinel(case):
    """One part's consumer staged h before its producer tiles landed: the buffer's NaN prefill."""
    stale = np.full((B, F), np.nan)
    with pytest.raises(AssertionError, match="non-finite"):
        case.check(*case.run(h_of_part={10: stale}))
    # ... and a stale but finite buffer (the previous step's rows): the part's sum is another row's
    with pytest.raises(AssertionError, match="down"):
        case.check(*case.run(h_of_part={10: case.h_ref[::-1]}))


def test_rejects_tile_taken_from_its_neighbour(case):
    h = case.h_ref.copy()
    h[:, 8 * 500:8 * 501] = case.h_ref[:, 8 * 501:8 * 502]
    with pytest.raises(AssertionError, match="'h'"):
        case.check(*case.run(h=h))


def test_rejects_gate_and_up_swapped_in_one_tile(case):
    g, u = case.pre()
    h = case.h_ref.copy()
    t = slice(8 * 77, 8 * 78)
    h[:, t] = mr.silu_mul(u[:, t], g[:, t])
    with pytest.raises(AssertionError, match="'h'"):
        case.check(*case.run(h=h))


def test_rejects_partial_added_twice(case):
    with pytest.raises(AssertionError, match="down"):
        case.check(*case.run(twice=10))   # (the smallest one)


def test_rejects_norm_scale_dropped_in_one_row():
    c = _Case(norm=True)
    c.check(*c.run())
    h = c.h_ref.copy()
    x = (c.X * c.nw).astype(np.float16).astype(np.float64)     # row 3 without rsqrt(mean(x^2) + eps)
    h[3] = mr.swiglu_ref(x[3:4], c.Wgu)[0]
    with pytest.raises(AssertionError, match="row', 3"):
        c.check(*c.run(h=h))


def test_rejects_residual_overwritten(case):
    with pytest.raises(AssertionError, match="down"):
        case.check(*case.run(store=True))


def test_rejects_one_h_element_off_by_its_magnitude(case):
    """One element of 7936 doubled - an element of the row's rms magnitude, 1 / 89 of the row's norm."""
    h = case.h_ref.copy()
    rms = np.sqrt(np.mean(h[2] ** 2))
    j = int(np.argmin(np.abs(np.abs(h[2]) - rms)))
    h[2, j] *= 2
    with pytest.raises(AssertionError, match="row', 2"):
        case.check(*case.run(h=h))


def test_rejects_nan_and_touched_guard_rows(case):
    hb, out = case.run()
    bad = hb.copy()
    bad[1, 100] = mr.NAN16
    with pytest.raises(AssertionError, match="non-finite"):
        case.check(bad, out)
    bad = hb.copy()
    bad[B, 7] = 0
    with pytest.raises(AssertionError, match="h guard"):
        case.check(bad, out)
    bad = out.copy()
    bad[B, K - 1] += 1
    with pytest.raises(AssertionError, match="out guard"):
        case.check(hb, bad)


def test_check_zeroed():
    poison = 0x7FC00ABC
    z = np.full(1000 + 64, poison, np.uint32)
    z[:1000] = 0
    cr.check_zeroed(z, 1000, poison)
    for i, v in ((999, poison), (5, 0x80000000), (1000, 0), (1063, 0)):
        bad = z.copy()
        bad[i] = v
        with pytest.raises(AssertionError, match="zero side job"):
            cr.check_zeroed(bad, 1000, poison)


# ---------------------------------------------------------------------------- the formats' own error
@pytest.mark.parametrize("tg,td,K,F,norm", [(cr.Q4_K, cr.Q4_K, 512, 3328, False), (cr.Q4_K, cr.Q6_K, 512, 7936, False),
                                            (cr.Q4_0, cr.Q4_1, 512, 3328, False), (cr.Q4_K, cr.Q6_K, 4096, 1280, True)])
def test_emulated_formats_stay_under_half_the_bounds(tg, td, K, F, norm):
    """The GPU cases' own inputs through the kernels' number formats on the CPU (f16 rows and weights,
    fp32 sums, f16 h, the partial sums added part by part): under half of each bound, so the bounds
    leave the kernels their rounding and nothing of the size of a defect."""
    Bq = 8
    Wgu, Wd = cr.weights(tg, 2 * F, K, "gu")[1], cr.weights(td, K, F, "dn")[1]
    X, nw, resid = cr.chain_rows(K, Bq, norm, 100 * Bq + F)
    hb, out = cr.emulate_chain(X, nw, Wgu, Wd, resid, norm, cr.chain_plan(F, K, CUS))
    fh, fd = cr.check_chain(hb, out, resid, cr.h_reference(X, nw, Wgu, norm), Wd, "emulated")
    assert fh < 0.5 and fd < 0.5, (fh, fd)
    cr.forget_weights()


# ---------------------------------------------------------------------------- the Wo chain
def _wo_case(F=1280, K=4096, Kwo=1024, Bq=6):
    rng = np.random.default_rng(21)
    Wo = 0.05 * rng.standard_normal((K, Kwo))
    Wgu = 0.05 * rng.standard_normal((2 * F, K))
    Wd = 0.05 * rng.standard_normal((K, F))
    xa = rng.standard_normal((Bq, Kwo)).astype(np.float16).astype(np.float64)
    resid0 = (2 * rng.standard_normal((Bq + 1, K))).astype(np.float32)
    nw = (0.5 + rng.random(K)).astype(np.float32)
    return dict(Wgu=Wgu, Wd=Wd, wo=xa @ Wo.T, resid0=resid0, nw=nw, B=Bq, F=F, rng=rng)


def _wo_run(c, wo=None, drop_wo_row=None):
    """The Wo chain in fp64 over Wo rows `wo` (default: the reference's)."""
    wo = c["wo"] if wo is None else wo
    Bq = c["B"]
    h = cr.wo_h_reference(c["resid0"][:Bq], wo, c["nw"], c["Wgu"])
    hb = np.full((Bq + 1, c["F"]), mr.NAN16, np.uint16)
    hb[:Bq] = cr.h_bits_of(h)
    r = c["resid0"].astype(np.float64)
    r[:Bq] += wo + mr.down_ref(cr.h_values(hb[:Bq]), c["Wd"])
    if drop_wo_row is not None:
        r[drop_wo_row] -= wo[drop_wo_row]
    return hb, r.astype(np.float32)


def test_wo_chain_checker_accepts_clean_and_rejects_defects():
    c = _wo_case()
    fh, ff = cr.check_wo_chain(*_wo_run(c), c["resid0"], c["wo"], c["nw"], c["Wgu"], c["Wd"])
    assert fh < 0.15 and ff < 0.05, (fh, ff)
    # the gate/up staged the rows before Wo's last K part had landed (half of Wo missing in x)
    hb, r = _wo_run(c)
    hb_early, _ = _wo_run(c, wo=0.5 * c["wo"])
    with pytest.raises(AssertionError, match="h row"):
        cr.check_wo_chain(hb_early, r, c["resid0"], c["wo"], c["nw"], c["Wgu"], c["Wd"])
    # Wo's sum missing from one final row
    with pytest.raises(AssertionError, match="final row', 4"):
        cr.check_wo_chain(*_wo_run(c, drop_wo_row=4), c["resid0"], c["wo"], c["nw"], c["Wgu"], c["Wd"])


@pytest.mark.parametrize("scale", [2.0, 0.25])
def test_wo_error_moves_h_by_less_than_half_its_bound(scale):
    """Nobody measured H_BOUND + 2.2 delta_b: Wo's rows perturbed by random noise of DN_BOUND of each
    row's norm (the size of error its bound allows) move the fp64 h by less than half of the bound -
    with the residual twice as large as Wo's rows (the GPU cases) and a quarter of them."""
    c = _wo_case()
    c["resid0"] = (c["resid0"] * (scale / 2)).astype(np.float32)
    Bq, rng = c["B"], np.random.default_rng(22)
    n = rng.standard_normal(c["wo"].shape)
    n *= cr.DN_BOUND * np.linalg.norm(c["wo"], axis=1, keepdims=True) / np.linalg.norm(n, axis=1, keepdims=True)
    h0 = cr.wo_h_reference(c["resid0"][:Bq], c["wo"], c["nw"], c["Wgu"])
    h1 = cr.wo_h_reference(c["resid0"][:Bq], c["wo"] + n, c["nw"], c["Wgu"])
    frac = mr.row_errors(h1, h0) / cr.wo_h_bounds(c["resid0"][:Bq], c["wo"])
    print("WO_H perturbation / bound per row", np.round(frac, 3))
    assert frac.max() < 0.5, frac
