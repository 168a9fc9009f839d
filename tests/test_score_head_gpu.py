"""The scoring head (csrc/kernels/score.hip) against fp64: per row the log-probability of a target
token, the log-sum-exp and the most probable token, computed without storing the logits.

Reference: the weights dequantised in the tile16 arithmetic (``arith="f16"``), x rounded to f16,
logits and log_softmax in fp64, argmax = lowest id on ties. The operands are the kernel's own, so
what remains is (a) the fp32 accumulation of a dot of length K - at most K roundings of relative
size u = 2^-24 on partial sums bounded by A = sum_k |w_k x_k|, i.e. K u A per logit; a
log-probability l - lse carries it twice (lse is a softmax-weighted mean of the logits' errors, at
most the largest of them) - and (b) the exp / log-sum-exp / subtraction roundings, for which
``logprobs_ref.lp_bound`` already holds the sampler's log-probabilities. Hence per row, with
A = max_j sum_k |W_jk x_k| over the real vocabulary:

    |lp - lp_fp64| <= 2 K u A + lp_bound        |lse - lse_fp64| <= K u A + lp_bound

Ids are exact: every case asserts first that its fp64 top two logits are further apart than
2 K u A in every row (the seeds below were chosen so), except the planted tie - one weight row
copied into another range, bit-equal logits, the lower id must win.

Measured on the MI355X (profiles/score_test_figures.txt): the worst error is 0.0046 of the bound -
K u A is the worst case of K same-signed roundings, nowhere near met."""
import functools

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize, random_blocks
from gpu_helpers import dev_bytes, hip, stream, to_planar
from logprobs_ref import lp_bound

pytestmark = pytest.mark.gpu

Q4, Q6, Q8 = GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q8_0
U32 = 2.0 ** -24
GUARD = 8            # sentinel words on either side of the records and the partials
SENTINEL = np.float32(-1234.5)

# (type, K, V, T, groups per range (0: the launcher's rule), x scale, planted tie)
#   V: 1000 = padding rows inside the last tile; 1024 = four groups (four ranges by the rule);
#   4112 = 17 groups: in pairs a ragged last range of ONE tile, in eights three ranges (8, 8, 1)
#   T: 63 | 64 | 65 = the 64 -> 128 token block border, 130 = two blocks and a ragged one
#   scale 30 | 45: every row's largest logit is above 89 and its smallest below -89 (asserted in case_ref):
#   expf overflows fp32 above 88.72, so a sum of exp(l) without the maximum subtracted is inf in every row
#   tie: the two equal maxima lie in different ranges (asserted in case_ref)
CASES = [
    (Q6, 256, 1000, 1, 0, 1.0, False),
    (Q8, 512, 1024, 63, 0, 1.0, False),
    (Q4, 256, 4112, 64, 2, 1.0, False),
    (Q6, 512, 4112, 65, 8, 30.0, False),
    (Q8, 256, 1000, 130, 1, 1.0, True),
    (Q4, 512, 1024, 130, 2, 45.0, True),
    (Q6, 256, 4112, 130, 0, 1.0, False),
]


def _swizzle4(x):
    """bmm's k order inside each 4-group: (0, 2, 1, 3)."""
    return x.reshape(*x.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(x.shape)


@functools.lru_cache(maxsize=None)
def case_ref(t, K, V, T, gpr, scale, tie):
    """(raw ggml rows [R], x f16 [T][K], targets, fp64 logits [T][V], A [T]) - CPU only, built once."""
    rng = np.random.default_rng(7 + 1000 * int(t) + K + 13 * V + T)
    R = (V + 15) // 16 * 16
    raw = random_blocks(t, V * K, rng, std=0.05)
    if R > V:   # tile padding rows with large weights: an unmasked row >= V wins every maximum
        raw = np.concatenate([raw, random_blocks(t, (R - V) * K, rng, std=20.0)])
    rb = len(raw) // R
    x = (rng.standard_normal((T, K)) * scale).astype(np.float32).astype(np.float16)
    deq = lambda: dequantize(raw, t, R * K, arith="f16").reshape(R, K)[:V].astype(np.float64)
    if tie:     # row 0's best weight row copied half the vocabulary away: equal logits in two ranges
        a = int(np.argmax(x[0].astype(np.float64) @ deq().T))
        b = (a + V // 2) % V
        assert gpr > 0 and a // (256 * gpr) != b // (256 * gpr), "the tie must span two ranges"
        raw = raw.copy()
        raw[b * rb:(b + 1) * rb] = raw[a * rb:(a + 1) * rb]
    W = deq()
    xd = x.astype(np.float64)
    logits = xd @ W.T
    A = (np.abs(xd) @ np.abs(W).T).max(1)
    # first range, last real row, none, last range, then anywhere
    tg = np.where(np.arange(T) % 4 == 0, V - 1, rng.integers(0, V, T))
    tg[1::4] = 5
    tg[2::4] = -1
    tg[3::4] = V - 3
    top2 = np.sort(logits, 1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    planted = np.zeros(T, bool)
    planted[0] = tie
    assert (gap[~planted] > 2 * K * U32 * A[~planted]).all(), "the seed gives a near-tie: choose another"
    assert not tie or gap[0] == 0.0
    assert scale == 1.0 or (logits.max(1).min() > 89 and logits.min(1).max() < -89), "exp(l) must overflow in every row"
    return raw, x, tg.astype(np.int32), logits, A


def _buffers(torch, T, words):
    rec = torch.full((2 * GUARD + 4 * T,), float(SENTINEL), device="cuda")
    part = torch.full((2 * GUARD + words,), float("nan"), device="cuda")
    part[:GUARD] = float(SENTINEL)
    part[GUARD + words:] = float(SENTINEL)
    return rec, part


def _launch(torch, t, K, V, T, gpr, scale, tie):
    raw, x, tg, _, _ = case_ref(t, K, V, T, gpr, scale, tie)
    R = (V + 15) // 16 * 16
    tw = torch.empty(hip().t16_bytes(int(t), R, K), dtype=torch.uint8, device="cuda")
    hip().t16_repack(dev_bytes(to_planar(t, raw, R, K)).data_ptr(), int(t), R, K, tw.data_ptr(), stream(), False)
    xs = np.full((T + 1, K), np.nan, np.float16)   # a NaN row behind row T - 1
    xs[:T] = _swizzle4(x)
    dx, dt = torch.from_numpy(xs).cuda(), torch.from_numpy(tg).cuda()
    words = hip().score_head_workspace_words(T, V, gpr)
    rec, part = _buffers(torch, T, words)
    hip().score_head(tw.data_ptr(), int(t), R, K, V, dx.data_ptr(), T, dt.data_ptr(), tg.tolist(),
                     part.data_ptr() + 4 * GUARD, words, rec.data_ptr() + 4 * GUARD, stream(), gpr=gpr)
    torch.cuda.synchronize()
    rec, part = rec.cpu().numpy(), part.cpu().numpy()
    for buf in (rec, part):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard words"
    return rec[GUARD:-GUARD].reshape(T, 4)


@pytest.mark.parametrize("t,K,V,T,gpr,scale,tie", CASES)
def test_score_head_vs_fp64(t, K, V, T, gpr, scale, tie):
    import torch
    _, _, tg, logits, A = case_ref(t, K, V, T, gpr, scale, tie)
    rec = _launch(torch, t, K, V, T, gpr, scale, tie)
    again = _launch(torch, t, K, V, T, gpr, scale, tie)
    assert np.array_equal(rec.view(np.uint32), again.view(np.uint32)), "two runs are bit-equal"
    M = logits.max(1)
    lse = M + np.log(np.exp(logits - M[:, None]).sum(1))
    best = logits.argmax(1)   # lowest id on ties
    assert np.array_equal(rec[:, 2].copy().view(np.int32), best.astype(np.int32))
    worst = 0.0
    for r in range(T):
        dot, b = K * U32 * A[r], lp_bound(logits[r], M[r])
        errs = [(abs(rec[r, 1] - lse[r]), dot + b), (abs(rec[r, 3] - (M[r] - lse[r])), 2 * dot + b)]
        if tg[r] < 0:
            assert np.isnan(rec[r, 0]), (r, rec[r])
        else:
            errs.append((abs(rec[r, 0] - (logits[r, tg[r]] - lse[r])), 2 * dot + lp_bound(logits[r], logits[r, tg[r]])))
        for e, bound in errs:
            assert np.isfinite(e) and e <= bound, (r, rec[r], e, bound)
            worst = max(worst, e / bound)
    print(f"score_head {t.name} K={K} V={V} T={T} gpr={gpr} scale={scale:g}: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("what", ["K128", "target", "workspace"])
def test_score_head_refuses(what):
    """Refused arguments raise before anything is queued: records and partials keep every word."""
    import torch
    t, K, V, T = Q8, 256, 1000, 3
    R = 1008
    tw = torch.zeros(hip().t16_bytes(int(t), R, K), dtype=torch.uint8, device="cuda")
    dx = torch.zeros((T, K), dtype=torch.float16, device="cuda")
    tg = [V if what == "target" else 1] * T
    dt = torch.tensor(tg, dtype=torch.int32, device="cuda")
    words = hip().score_head_workspace_words(T, V)
    rec, part = _buffers(torch, T, words)
    rec0, part0 = rec.clone(), part.clone()
    with pytest.raises(RuntimeError):
        hip().score_head(tw.data_ptr(), int(t), R, 128 if what == "K128" else K, V, dx.data_ptr(), T, dt.data_ptr(), tg,
                         part.data_ptr() + 4 * GUARD, words - (what == "workspace"), rec.data_ptr() + 4 * GUARD, stream())
    torch.cuda.synchronize()
    assert torch.equal(rec.view(torch.int32), rec0.view(torch.int32))
    assert torch.equal(part.view(torch.int32), part0.view(torch.int32))
