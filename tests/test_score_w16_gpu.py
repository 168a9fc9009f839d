"""score_head_w16 (csrc/kernels/score_w16.hip: a row-major BF16 / F16 lm_head) against fp64 logits of
the stored 16-bit weights and x, fp64 log_softmax, argmax = lowest id on ties. Products of two bf16 or
two f16 values are exact in fp32, so the bound is test_score_head_gpu.py's header's: |lp - lp64| <=
2 K u A + lp_bound, |lse - lse64| <= K u A + lp_bound, u = 2^-24, A = max_j sum_k |W_jk x_k|; ids exact.
Measured (profiles/score_w16_test_figures.txt): the worst error is 0.067 of the bound, at K = 64."""
import functools

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from gpu_helpers import hip, stream
from logprobs_ref import lp_bound
from test_score_head_gpu import GUARD, SENTINEL, U32, _buffers

pytestmark = pytest.mark.gpu

BF16, F16, F32 = GGMLType.BF16, GGMLType.F16, GGMLType.F32

# (type, K, V, T, groups per range (0: the launcher's rule), x scale, planted tie)
#   K: 64 = one step (fewer than the 3-deep ring), 192 = the ring, 256 = ring + 1; V: 100 < one 128-row group,
#   129 = a last group of one row, 1000 = 8 groups (gpr 7: a last range of ONE group; the rule: 8 ranges); T: 33 =
#   a 32-token tile border, 63 | 64 | 65 = the 64 -> 128 token block border; scale 45 | 60: exp(l) overflows fp32
CASES = [
    (BF16, 64, 100, 1, 0, 1.0, False),
    (F16, 192, 128, 33, 0, 1.0, False),
    (BF16, 256, 129, 63, 0, 1.0, False),
    (F16, 512, 1000, 64, 3, 1.0, False),
    (BF16, 512, 1000, 65, 7, 45.0, False),
    (F16, 256, 1000, 130, 0, 1.0, False),
    (BF16, 64, 1000, 130, 2, 1.0, True),
    (F16, 256, 1000, 130, 2, 60.0, True),
    (BF16, 192, 129, 130, 1, 1.0, False),
    (F16, 64, 100, 65, 0, 1.0, False),
]


def to16(t, a):
    """f32 -> the type's 16-bit words (round to nearest even) and their exact fp64 values."""
    a = np.ascontiguousarray(a, np.float32)
    if t == F16:
        return a.astype(np.float16).view(np.uint16), a.astype(np.float16).astype(np.float64)
    u = a.view(np.uint32)
    w = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return w, (w.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case_ref(t, K, V, T, gpr, scale, tie):
    """(W words [V][K], x words [T][K], targets, fp64 logits [T][V], A [T]) - CPU only, built once."""
    rng = np.random.default_rng(11 + 1000 * int(t) + K + 13 * V + T)
    w16, W = to16(t, rng.standard_normal((V, K)) * 0.05)
    x16, xd = to16(t, rng.standard_normal((T, K)) * scale)
    if tie:     # row 0's best weight row copied half the vocabulary away: equal logits in two ranges
        a = int(np.argmax(xd[0] @ W.T))
        b = (a + V // 2) % V
        assert gpr > 0 and a // (128 * gpr) != b // (128 * gpr), "the tie must span two ranges"
        w16[b], W[b] = w16[a], W[a]
    logits = xd @ W.T
    A = (np.abs(xd) @ np.abs(W).T).max(1)
    tg = np.where(np.arange(T) % 4 == 0, V - 1, rng.integers(0, V, T))   # last real row, ..., anywhere
    tg[1::4], tg[2::4], tg[3::4] = 5, -1, V - 3                          # first range, none, last range
    top2 = np.sort(logits, 1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    assert (gap[int(tie):] > 2 * K * U32 * A[int(tie):]).all(), "the seed gives a near-tie: choose another"
    assert not tie or gap[0] == 0.0
    assert scale == 1.0 or (logits.max(1).min() > 89 and logits.min(1).max() < -89), "exp(l) must overflow in every row"
    return w16, x16, tg.astype(np.int32), logits, A


def _launch(torch, case):
    t, K, V, T, gpr = case[:5]
    w16, x16, tg, _, _ = case_ref(*case)
    xs = np.full((T + 1, K), 0x7E00 if t == F16 else 0x7FC0, np.uint16)   # a NaN row behind row T - 1
    xs[:T] = x16
    dw = torch.from_numpy(w16.view(np.int16)).cuda()
    dx, dt = torch.from_numpy(xs.view(np.int16)).cuda(), torch.from_numpy(tg).cuda()
    words = hip().score_head_w16_workspace_words(T, V, gpr)
    rec, part = _buffers(torch, T, words)
    hip().score_head_w16(dw.data_ptr(), int(t), V, K, V, dx.data_ptr(), T, dt.data_ptr(), tg.tolist(),
                         part.data_ptr() + 4 * GUARD, words, rec.data_ptr() + 4 * GUARD, stream(), gpr=gpr)
    torch.cuda.synchronize()
    rec, part = rec.cpu().numpy(), part.cpu().numpy()
    assert all((b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all() for b in (rec, part)), "guard words"
    return rec[GUARD:-GUARD].reshape(T, 4)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0].name}-K{c[1]}-V{c[2]}-T{c[3]}-g{c[4]}")
def test_score_head_w16_vs_fp64(case):
    import torch
    t, K, V, T, gpr, scale = case[:6]
    _, _, tg, logits, A = case_ref(*case)
    rec = _launch(torch, case)
    assert np.array_equal(rec.view(np.uint32), _launch(torch, case).view(np.uint32)), "two runs are bit-equal"
    M = logits.max(1)
    lse = M + np.log(np.exp(logits - M[:, None]).sum(1))
    assert np.array_equal(rec[:, 2].copy().view(np.int32), logits.argmax(1).astype(np.int32))   # lowest id on ties
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
    print(f"score_head_w16 {t.name} K={K} V={V} T={T} gpr={gpr} scale={scale:g}: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("what", ["K96", "target", "workspace", "F32"])
def test_score_head_w16_refuses(what):
    """Refused arguments raise before anything is queued: records and partials keep every word."""
    import torch
    K, V, T = 128, 300, 3
    dw = dx = torch.zeros((V, K), dtype=torch.float32, device="cuda")   # (large enough for every case's type)
    tg = [V if what == "target" else 1] * T
    dt = torch.tensor(tg, dtype=torch.int32, device="cuda")
    words = hip().score_head_w16_workspace_words(T, V)
    rec, part = _buffers(torch, T, words)
    rec0, part0 = rec.clone(), part.clone()
    with pytest.raises(RuntimeError):
        hip().score_head_w16(dw.data_ptr(), int(F32 if what == "F32" else BF16), V, 96 if what == "K96" else K, V,
                             dx.data_ptr(), T, dt.data_ptr(), tg, part.data_ptr() + 4 * GUARD,
                             words - (what == "workspace"), rec.data_ptr() + 4 * GUARD, stream())
    torch.cuda.synchronize()
    assert torch.equal(rec.view(torch.int32), rec0.view(torch.int32))
    assert torch.equal(part.view(torch.int32), part0.view(torch.int32))
