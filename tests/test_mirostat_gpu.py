"""Kernel-level tests of mirostat v1 / v2 on the device sampler (sampler.hip stage 1's scratch store and
stage 2's mirostat path) against the fp64 reference and bounds of tests/mirostat_ref.py. Every case is
launched twice (bit-equal), with the state, candidate blocks and scratch between sentinel words and
+200 behind each logits row; the reference asserts one acceptable token per case before the launch."""
import numpy as np
import pytest

from gpu_helpers import hip, stream
from llama_fastapi_k8s_gpu_amd.engine.sampling import SamplingParams
from mirostat_ref import reference

SENT, GUARD, PAD, STEP = 0x5A5A5A5A, 16, 37, 3


def make_case(mode, V, mu, eta, tie="", seed=0):
    """Logits around +91 (exp overflows fp32) with every third around -92; v2 rows carry a bias and
    penalties that move tokens across the threshold, v1 rows none (mirostat_ref: k is then exact)."""
    rng = np.random.default_rng(1000 * V + 10 * mode + seed)
    x = rng.normal(91.0, 2.0, V).astype(np.float32)
    x[1::3] = rng.normal(-92.0, 1.0, len(x[1::3])).astype(np.float32)
    order = np.argsort(-x, kind="stable")
    if tie == "top":        # the best value three times: mu below its surprise keeps the lowest id alone
        x[[5, 3, 6]] = x.max() + 1
    if tie == "plateau":    # ranks 20 .. 400 equal: v1's count cut ends inside the run
        x[order[20:400]] = x[order[20]]
    if mode == 1:
        p = SamplingParams(temperature=1.0, repeat_penalty=1.0, seed=77 + seed, mirostat_mode=1, mirostat_tau=4.0,
                           mirostat_eta=eta)
        return x, p, [], mu
    p = SamplingParams(temperature=0.9, repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1, seed=77 + seed,
                       logit_bias={1: 183.5, int(order[1]): -3.0}, mirostat_mode=2, mirostat_tau=4.0, mirostat_eta=eta)
    return x, p, [int(order[0]), int(order[2]), int(order[0]), 8 % V], mu


def params_bytes(p):
    return np.frombuffer(hip().sampler_params_bytes(
        p.top_k, p.top_p, p.min_p, p.temperature, p.repeat_penalty, p.frequency_penalty, p.presence_penalty, p.last_n,
        p.seed, 0, 1.0, 1.0, p.logit_bias, p.mirostat_mode, p.mirostat_tau, p.mirostat_eta), np.uint8)


def _guarded(torch, data):
    g = torch.full((2 * GUARD + data.size,), SENT, dtype=torch.int32, device="cuda")
    g[GUARD:-GUARD] = torch.from_numpy(data.view(np.int32).ravel())
    return g


def launch(torch, rows, V, slots=None):
    """rows: (x, params, window, mu); single row on slot 0, or batched on `slots`. -> (state [4][8], raw)"""
    h, B = hip(), len(rows)
    logits = np.full((B, V + PAD), 200.0, np.float32)
    pb = [params_bytes(r[1]) for r in rows]
    params, state, ring = np.zeros((4, pb[0].size), np.uint8), np.zeros((4, 8), np.int32), np.zeros((4, 64), np.int32)
    for b, (x, p, window, mu) in enumerate(rows):
        s = slots[b] if slots else 0
        logits[b, :V], params[s], ring[s, :len(window)] = x, pb[b], window
        state[s, 2:5] = STEP, len(window), len(window)
        state[s, 6] = np.float32(mu).view(np.int32)
    dl, dp, dr = (torch.from_numpy(a).cuda() for a in (logits, params, ring))
    ds = _guarded(torch, state)
    cand = _guarded(torch, np.zeros(B * h.sampler_cand_words(V), np.int32))
    scr = _guarded(torch, np.zeros(B * V, np.int32))
    ptr = lambda g: g.data_ptr() + 4 * GUARD  # noqa: E731
    kw = {}
    if slots:
        dslots, dout = torch.tensor(slots, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        kw = dict(batch=B, slots=dslots.data_ptr(), logits_ld=V + PAD, batch_out=dout.data_ptr())
    h.sample(dl.data_ptr(), V, dp.data_ptr(), dr.data_ptr(), ptr(ds), ptr(cand), 0, 0, 1, stream(), mscratch=ptr(scr), **kw)
    torch.cuda.synchronize()
    raw = [g.cpu().numpy() for g in (ds, cand, scr)]
    for w in raw:
        assert (w[:GUARD] == SENT).all() and (w[-GUARD:] == SENT).all(), "guard words overwritten"
    assert np.array_equal(dl.cpu().numpy().view(np.int32), logits.view(np.int32)), "a logits row was written"
    st = raw[0][GUARD:-GUARD].reshape(4, 8)
    if slots:
        assert dout.cpu().tolist() == [int(st[s, 0]) for s in slots]
    return st, raw


def check(torch, rows, V, slots=None):
    refs = [reference(x, p, w, mu, STEP) if p.mirostat_mode else None for x, p, w, mu in rows]
    for r in refs:
        assert r is None or r["margin"] > 1.0, f"the case is within a bound of a decision: {r}"
    st, raw = launch(torch, rows, V, slots)
    st2, raw2 = launch(torch, rows, V, slots)
    assert all(np.array_equal(a, b) for a, b in zip(raw, raw2)), "two runs differ"
    worst = 0.0
    for b, r in enumerate(refs):
        s = slots[b] if slots else 0
        assert st[s, 2] == STEP + 1 and st[s, 5] == 1 and st[s, 3] == len(rows[b][2]) + 1
        if r is not None:
            assert int(st[s, 0]) == r["token"], (b, r)
            err = abs(float(st[s, 6:7].view(np.float32)[0]) - r["mu"])
            assert err <= r["d_mu"], (b, err, r)
            worst = max(worst, err / r["d_mu"])
    print(f"mirostat V={V}: worst mu error / bound = {worst:.3f}; smallest margin = "
          f"{min(r['margin'] for r in refs if r):.1f}")
    return st, refs


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# mu 0.05: below the best token's surprise, one token kept; 400: everything kept, past the 4096-entry
# LDS window at V = 4112, so the bisection draws
CASES = [(2, V, mu, eta, "") for V in (8, 1000, 1024, 1025, 4112) for mu, eta in ((0.05, 0.1), (5.0, 0.0), (400.0, 0.1))]
CASES += [(2, 1000, 0.05, 0.1, "top"), (1, 8, 3.0, 0.1, ""), (1, 1000, 8.0, 0.0, ""), (1, 1000, 8.0, 0.1, "plateau"),
          (1, 4112, 400.0, 0.1, "")]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,V,mu,eta,tie", CASES)
def test_single_row(torch, mode, V, mu, eta, tie):
    _, (r,) = check(torch, [make_case(mode, V, mu, eta, tie)], V)
    if mu == 0.05:
        assert r["k"] == 1
    if mode == 2 and mu == 5.0:   # the bias and the penalties move tokens across the threshold
        x, p, _, _ = make_case(mode, V, mu, eta, tie)
        raw = SamplingParams(temperature=p.temperature, repeat_penalty=1.0, mirostat_mode=2, seed=p.seed)
        assert reference(x, raw, [], mu, STEP)["kept"] != r["kept"]
    if mu == 400.0:
        assert r["k"] == V
    if tie == "plateau":
        assert r["cut_in_tie"]


@pytest.mark.gpu
@pytest.mark.parametrize("V,mu", [(1000, 5.0), (4112, 400.0)])
def test_batched_rows_mixed(torch, V, mu):
    """Slots [2, 0, 3], pitch V + 37: a v2 row, a plain top-k row and a v1 row in one launch. The plain
    row draws what it draws alone, and its mu word stays."""
    x, _, w, _ = make_case(2, V, mu, 0.1, seed=5)
    plain = (x, SamplingParams(seed=9), w, 123.0)
    rows = [make_case(2, V, mu, 0.1, seed=3), plain, make_case(1, V, mu + 3.0, 0.1, seed=4)]
    st, _ = check(torch, rows, V, [2, 0, 3])
    alone, _ = launch(torch, [plain], V)
    assert st[0, 0] == alone[0, 0] and np.array_equal(st[0], alone[0])
    assert st[0, 6:7].view(np.float32)[0] == np.float32(123.0)


def test_routing():
    """Mirostat takes the device route only where the backend says it samples it there."""
    p = SamplingParams(temperature=0.8, mirostat_mode=2)
    assert p.gpu_compatible(32000, mirostat=True) and not p.gpu_compatible(32000)
    assert SamplingParams(temperature=0.8, mirostat_mode=1, top_k=0).gpu_compatible(32000, 20, mirostat=True)
    assert not SamplingParams(temperature=0.8, mirostat_mode=2, n_probs=21).gpu_compatible(32000, 20, mirostat=True)
    assert not SamplingParams(temperature=0.8, mirostat_mode=2, grammar=object()).gpu_compatible(32000, mirostat=True)
