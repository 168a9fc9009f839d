"""The log-probability checker of the GPU tests, tested on the CPU: it accepts the fp32 emulation of
the kernel over the GPU test's own inputs with a factor two to spare, and rejects every planted
single defect (tests/logprobs_ref.py)."""
import numpy as np
import pytest

from logprobs_ref import (KINDS, LP_ABS, LP_ULPS, NS, VOCABS, check_logprobs, emulate_logprobs, lp_bound,
                          make_logits, ref_logprobs, ulp32)


def _token(logits):
    return int(np.argsort(logits)[-3]) if logits.shape[0] > 3 else 0


@pytest.mark.parametrize("V", VOCABS)
def test_emulation_within_half_the_bound(V):
    """The bound's constants: the kernel's arithmetic in fp32 stays within HALF the bound on every
    input of the GPU test."""
    worst = 0.0
    for kind in KINDS:
        x = make_logits(kind, V)
        worst = max(worst, check_logprobs(emulate_logprobs(x, _token(x), max(NS)), x, _token(x), max(NS)))
    print(f"V={V}: emulation worst error / bound = {worst:.3f}")
    assert worst <= 0.5


def test_bound_at_most_1e4():
    x = np.array([100.0, -100.0, 3.0], np.float32)
    assert max(lp_bound(x, v) for v in x) <= 1e-4
    assert LP_ABS + LP_ULPS * ulp32(100.0) <= 1e-4


def test_n_larger_than_vocabulary_and_equal_logits():
    x = make_logits("normal4", 8)
    assert len(ref_logprobs(x, 0, 20)[1]) == 8
    check_logprobs(emulate_logprobs(x, 0, 20), x, 0, 20)
    e = make_logits("equal", 1025)
    lp, top = ref_logprobs(e, 3, 5)
    assert [i for i, _ in top] == [0, 1, 2, 3, 4]
    assert all(abs(v + np.log(1025)) < 1e-12 for _, v in top) and abs(lp + np.log(1025)) < 1e-12


def _rejects(record, logits, token, n):
    with pytest.raises(AssertionError):
        check_logprobs(record, logits, token, n)


def test_rejects_dropped_partial_slice():
    x = make_logits("normal4", 1025)
    x[1024] = x.max() - np.float32(0.5)   # the last slice's one logit carries weight
    t = _token(x)
    check_logprobs(emulate_logprobs(x, t, 5), x, t, 5)
    _rejects(emulate_logprobs(x, t, 5, "drop_last_slice"), x, t, 5)


def test_rejects_missing_max_subtraction():
    x = make_logits("shift90", 32000)
    _rejects(emulate_logprobs(x, _token(x), 5, "no_max_sub"), x, _token(x), 5)


def test_rejects_lse_over_biased_logits():
    x = make_logits("normal4", 32000)
    b = x.copy()
    b[int(np.argmax(x))] += np.float32(2)  # a logit bias / penalty on the top token
    _rejects(emulate_logprobs(x, _token(x), 5, "biased_lse", biased=b), x, _token(x), 5)


def test_rejects_ties_by_descending_id():
    for kind in ("dup_in_slice", "dup_across", "equal"):
        x = make_logits(kind, 1025)
        check_logprobs(emulate_logprobs(x, 0, 5), x, 0, 5)
        _rejects(emulate_logprobs(x, 0, 5, "ties_desc_id"), x, 0, 5)


def test_rejects_unsorted_list():
    x = make_logits("normal4", 1000)
    _rejects(emulate_logprobs(x, 0, 5, "unsorted"), x, 0, 5)


def test_rejects_short_list():
    x = make_logits("normal4", 1000)
    _rejects(emulate_logprobs(x, 0, 5, "n_minus_1"), x, 0, 5)
    _rejects(emulate_logprobs(x, 0, 1, "n_minus_1"), x, 0, 1)


def test_rejects_token_of_the_neighbouring_row():
    x, y = make_logits("normal4", 32000), make_logits("normal4", 32000, seed=1)
    _rejects(emulate_logprobs(x, _token(x), 5, "neighbour_row", other=y), x, _token(x), 5)


def test_rejects_unscaled_slice_sums():
    x = make_logits("normal4", 32000)
    _rejects(emulate_logprobs(x, _token(x), 5, "no_rescale"), x, _token(x), 5)
