"""Reference, checker and kernel emulation for the device token log-probabilities
(csrc/kernels/sampler.hip: logprobs_stage1 / logprobs_stage2).

  * ``ref_logprobs``      - the fp64 reference: ``engine.sampling.token_logprobs`` with the ties at the
                            end of the list settled the way the contract says (ascending token id).
  * ``check_logprobs``    - one record against that reference: ids and order exact, values within
                            ``lp_bound``.
  * ``emulate_logprobs``  - the kernel's slice-wise reduction in fp32 (slice maximum, slice sum of
                            exp, rescale to the global maximum, log), with single defects that can be
                            planted to show the checker rejects them.
  * ``make_logits``       - the inputs of the GPU test, shared so the bound's constants are set over
                            exactly those inputs (tests/test_logprobs_ref.py).

The bound, against fp64 log_softmax of the same fp32 logits: the kernel's error is (a) the relative
error of the fp32 sums of exp, which is an ABSOLUTE error of the log (a few 1e-7 per rounding, 16
sequential and 8 tree additions per slice, then the slices), and (b) roundings of values of the size
of M, lse and the logit itself: M + log(S) and l - lse round at ulp(max(|M|, |lse|, |l|)) / 2 each,
and m_s - M inside the rescaling exp rounds at the same size. Hence

    |lp_kernel - lp_fp64| <= LP_ABS + LP_ULPS * ulp32(max(|M|, |lse|, |l|))

with LP_ABS = 4e-6 and LP_ULPS = 4: at |logits| <= 100 that is 4e-6 + 4 * 7.63e-6 = 3.5e-5 < 1e-4.
tests/test_logprobs_ref.py holds the emulation's worst error over the GPU test's inputs to half of it.
"""
import numpy as np

from llama_fastapi_k8s_gpu_amd.engine.sampling import token_logprobs

SLICE = 1024          # logits per stage-1 wave
MAX_LOGPROBS = 20     # kMaxLogprobs
REC_WORDS = 2 + 2 * MAX_LOGPROBS
LP_ABS = 4e-6
LP_ULPS = 4

VOCABS = (1000, 1024, 1025, 32000, 151936)
NS = (1, 5, 20)
KINDS = ("normal4", "spike30", "shift90", "dup_in_slice", "dup_across", "equal")


def make_logits(kind: str, V: int, seed: int = 0) -> np.ndarray:
    """The GPU test's inputs (fp32 [V])."""
    rng = np.random.default_rng(1000 * seed + V + 7 * KINDS.index(kind))
    x = (rng.standard_normal(V) * 4).astype(np.float32)
    if kind == "spike30":
        x[(3 * V) // 4] = x.max() + np.float32(30)
    elif kind == "shift90":
        x = (x + np.float32(90)).astype(np.float32)
    elif kind == "dup_in_slice":     # the maximum twice inside the last slice that holds two logits
        lo = ((V - 1) // SLICE) * SLICE
        lo -= SLICE if V - lo < 2 and lo else 0
        top = x.max() + np.float32(1)
        x[lo] = top
        x[min(V - 1, lo + 700)] = top
    elif kind == "dup_across":       # ... and in two slices (one slice only: twice in it)
        top = x.max() + np.float32(1)
        x[V - 1] = top
        x[17] = top
    elif kind == "equal":            # more than 64 ties in every full slice
        x[:] = np.float32(1.25)
    return x


def ref_logprobs(logits: np.ndarray, token: int, n: int):
    """(log p(token), [(id, log p)] top-n) in fp64: token_logprobs, ties by ascending id."""
    logits = np.asarray(logits, np.float32)
    x = logits.astype(np.float64)
    M = x.max()
    lp = x - M - np.log(np.exp(x - M).sum())
    n = max(0, min(int(n), x.shape[0]))
    order = np.lexsort((np.arange(x.shape[0]), -x))[:n]
    top = [(int(i), float(lp[i])) for i in order]
    # token_logprobs is this rounded to fp32 (log_softmax returns fp32, which can also tie two
    # distinct logits); only WHICH of several equal values it lists may differ
    tl_tok, tl_top = token_logprobs(logits, int(token), n)
    tol = 2 * float(np.spacing(np.float32(abs(lp).max())))
    assert abs(tl_tok - lp[int(token)]) <= tol and len(tl_top) == n
    assert all(abs(a - b) <= tol for (_, a), (_, b) in zip(tl_top, top)), "ref_logprobs: not token_logprobs' values"
    return float(lp[int(token)]), top


def ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def lp_bound(logits: np.ndarray, logit: float) -> float:
    """The bound of one value's error (module docstring)."""
    x = np.asarray(logits, np.float64)
    M = float(x.max())
    lse = M + float(np.log(np.exp(x - M).sum()))
    return LP_ABS + LP_ULPS * ulp32(max(abs(M), abs(lse), abs(float(logit))))


def decode_record(words: np.ndarray):
    """A kLogprobRecWords record -> (lp(token), [(id, lp)])."""
    w = np.ascontiguousarray(words, np.uint32)
    assert w.shape == (REC_WORDS,)
    n = int(w[1].view(np.int32))
    assert 0 <= n <= MAX_LOGPROBS, f"record holds n = {n}"
    ids = w[2:2 + MAX_LOGPROBS].view(np.int32)
    lps = w[2 + MAX_LOGPROBS:].view(np.float32)
    return float(w[:1].view(np.float32)[0]), [(int(ids[i]), float(lps[i])) for i in range(n)]


def check_logprobs(record, logits: np.ndarray, token: int, n: int) -> float:
    """Assert that `record` = (lp(token), [(id, lp)]) describes the raw `logits`; returns the worst
    error over its bound."""
    logits = np.asarray(logits, np.float32)
    lp_tok, top = record
    ref_tok, ref_top = ref_logprobs(logits, token, n)
    assert len(top) == len(ref_top) == min(int(n), logits.shape[0]), \
        f"{len(top)} entries, expected {min(int(n), logits.shape[0])}"
    assert [i for i, _ in top] == [i for i, _ in ref_top], \
        f"ids {[i for i, _ in top]} != reference {[i for i, _ in ref_top]}"
    worst = 0.0
    pairs = [(lp_tok, ref_tok, float(logits[int(token)]))]
    pairs += [(v, rv, float(logits[i])) for (i, v), (_, rv) in zip(top, ref_top)]
    for k, (v, rv, l) in enumerate(pairs):
        b = lp_bound(logits, l)
        err = abs(float(v) - rv)
        assert np.isfinite(v) and err <= b, \
            f"{'token' if k == 0 else f'top[{k - 1}]'}: {v!r} vs {rv!r}, error {err:.3g} > bound {b:.3g}"
        worst = max(worst, err / b)
    return worst


def emulate_logprobs(logits: np.ndarray, token: int, n: int, defect: str = None, other: np.ndarray = None,
                     biased: np.ndarray = None):
    """The kernel's arithmetic in fp32 -> (lp(token), [(id, lp)]). `defect` plants one error:
    drop_last_slice, no_max_sub, biased_lse (lse over `biased`), ties_desc_id, unsorted, n_minus_1,
    neighbour_row (the token's logit from `other`), no_rescale."""
    f32 = np.float32
    x = np.asarray(logits, f32)
    V = x.shape[0]
    src = np.asarray(biased, f32) if defect == "biased_lse" else x
    nb = (V + SLICE - 1) // SLICE
    if defect == "drop_last_slice" and nb > 1 and V % SLICE:
        nb -= 1
    m = np.empty(nb, f32)
    s = np.empty(nb, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(nb):
            sl = src[g * SLICE:min(V, (g + 1) * SLICE)]
            m[g] = f32(0) if defect == "no_max_sub" else sl.max()
            # 64 lanes x 16 sequential additions, then the lanes' sums
            e = np.zeros(SLICE, f32)
            e[:sl.shape[0]] = np.exp((sl - m[g]).astype(f32)).astype(f32)
            lanes = np.zeros(64, f32)
            for k in range(SLICE // 64):
                lanes = (lanes + e[64 * k:64 * (k + 1)]).astype(f32)
            s[g] = lanes.sum(dtype=f32)
        M = m.max()
        scale = np.ones(nb, f32) if defect == "no_rescale" else np.exp((m - M).astype(f32)).astype(f32)
        S = (s * scale).astype(f32).sum(dtype=f32)
        lse = f32(M + np.log(S).astype(f32))
    n = max(0, min(int(n), V, MAX_LOGPROBS))
    ids = np.arange(V)
    order = np.lexsort((-ids if defect == "ties_desc_id" else ids, -x.astype(np.float64)))[:n]
    if defect == "n_minus_1":
        order = order[:-1]
    if defect == "unsorted" and len(order) > 1:
        order = np.concatenate([order[1:2], order[0:1], order[2:]])
    top = [(int(i), float(f32(x[i] - lse))) for i in order]
    row = np.asarray(other, f32) if defect == "neighbour_row" else x
    return float(f32(row[int(token)] - lse)), top
