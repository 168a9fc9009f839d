"""Kernel-level tests of the device token log-probabilities (sampler.hip logprobs_stage1 / _stage2)
against the fp64 reference of tests/logprobs_ref.py: ids and order exact, values within lp_bound.

Every case first runs the SAMPLER over the same logits with a logit bias and penalties that move the
greedy pick off the raw argmax, so a record that described the biased / penalised logits, or paired
with another token, fails. The logits buffers carry +200 behind their V real values (logits past V
count for nothing) and must be bit-equal afterwards; the records sit between sentinel words."""
import numpy as np
import pytest

from gpu_helpers import hip, stream
from logprobs_ref import KINDS, NS, REC_WORDS, VOCABS, check_logprobs, decode_record, make_logits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


SENT = 0xA5A5A5A5
GUARD = 16
PAD = 37            # words behind each logits row


def _params(torch, top, other):
    """Greedy, with penalties and a bias that push the raw argmax down and `other` up."""
    pb = np.frombuffer(hip().sampler_params_bytes(1, 1.0, 0.0, 0.0, 1.5, 2.0, 1.0, 64, 0, 1, 1.0, 1.0,
                                                  {int(top): -50.0, int(other): 45.0}), np.uint8)
    return torch.from_numpy(pb.copy()).cuda()


def _rows(torch, kind, V, B):
    """B logits rows of pitch V + PAD (the pad holds +200) -> (host rows, device buffer)."""
    xs = [make_logits(kind, V, seed=r) for r in range(B)]
    buf = np.full((B, V + PAD), 200.0, np.float32)
    for r, x in enumerate(xs):
        buf[r, :V] = x
    return xs, torch.from_numpy(buf).cuda()


def _sample_row(torch, dl_ptr, V, x, state, ring, slot):
    """The sampler's two stages over one row into slot `slot` of state / ring -> the token."""
    h = hip()
    top, other = int(np.argmax(x)), int((np.argmax(x) + V // 2) % V)
    ring[slot, :3] = torch.tensor([top, top, 7 % V], dtype=torch.int32)
    state[slot, 3], state[slot, 4] = 3, 3
    dp = _params(torch, top, other)
    cand = torch.zeros(h.sampler_cand_words(V), dtype=torch.int32, device="cuda")
    h.sample(dl_ptr, V, dp.data_ptr(), ring[slot].data_ptr(), state[slot].data_ptr(), cand.data_ptr(), 0, 0, 1,
             stream())
    torch.cuda.synchronize()
    tok = int(state[slot, 0].item())
    if V > 1:
        assert tok != top, "the bias and penalties should have moved the greedy pick"
    return tok


def _records(torch, rows):
    return torch.full((GUARD + rows * REC_WORDS + GUARD,), SENT - (1 << 32), dtype=torch.int32, device="cuda")


def _split(rec):
    w = rec.cpu().numpy().view(np.uint32)
    assert (w[:GUARD] == SENT).all() and (w[-GUARD:] == SENT).all(), "guard words overwritten"
    return w[GUARD:-GUARD].reshape(-1, REC_WORDS)


def _single(torch, kind, V, ns):
    h = hip()
    (x,), dl = _rows(torch, kind, V, 1)
    before = dl.clone()
    state = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    ring = torch.zeros((1, 64), dtype=torch.int32, device="cuda")
    tok = _sample_row(torch, dl.data_ptr(), V, x, state, ring, 0)
    part = torch.zeros(h.logprob_part_words(V), dtype=torch.float32, device="cuda")
    worst = 0.0
    for n in ns:
        rec = _records(torch, 1)
        dn = torch.tensor([n], dtype=torch.int32, device="cuda")
        h.logprobs(dl.data_ptr(), V, dn.data_ptr(), state.data_ptr(), part.data_ptr(),
                   rec.data_ptr() + 4 * GUARD, stream())
        torch.cuda.synchronize()
        r = _split(rec)[0]
        assert int(r[1]) == min(n, V)
        worst = max(worst, check_logprobs(decode_record(r), x, tok, n))
        assert torch.equal(dl.view(torch.int32), before.view(torch.int32)), "the logits row was written"
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", VOCABS)
def test_single_row(torch, V, kind):
    w = _single(torch, kind, V, NS)
    print(f"logprobs single V={V} {kind}: worst error / bound = {w:.3f}")


def test_more_entries_than_vocabulary(torch):
    for kind in ("normal4", "equal"):
        w = _single(torch, kind, 8, (20, 9, 8))
        print(f"logprobs single V=8 {kind}: worst error / bound = {w:.3f}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", VOCABS)
def test_batched_rows(torch, V, kind):
    """3 rows on slots [2, 0, 3], row pitch > V; slot 0 asks for nothing: its row does no work and its
    record keeps the sentinel. Each stage through its own call of the binding."""
    h = hip()
    slots = [2, 0, 3]
    n_probs = [0, 7, 5, 20]  # per slot
    xs, dl = _rows(torch, kind, V, 3)
    before = dl.clone()
    state = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    ring = torch.zeros((4, 64), dtype=torch.int32, device="cuda")
    toks = [_sample_row(torch, dl[b].data_ptr(), V, xs[b], state, ring, slots[b]) for b in range(3)]
    part = torch.zeros(3 * h.logprob_part_words(V), dtype=torch.float32, device="cuda")
    rec = _records(torch, 3)
    dn = torch.tensor(n_probs, dtype=torch.int32, device="cuda")
    ds = torch.tensor(slots, dtype=torch.int32, device="cuda")
    for stage in (1, 2):
        h.logprobs(dl.data_ptr(), V, dn.data_ptr(), state.data_ptr(), part.data_ptr(), rec.data_ptr() + 4 * GUARD,
                   stream(), batch=3, slots=ds.data_ptr(), logits_ld=V + PAD, stage=stage)
    torch.cuda.synchronize()
    r = _split(rec)
    assert (r[1] == SENT).all(), "the record of the row that asked for nothing was written"
    w = max(check_logprobs(decode_record(r[b]), xs[b], toks[b], n_probs[slots[b]]) for b in (0, 2))
    assert torch.equal(dl.view(torch.int32), before.view(torch.int32)), "a logits row was written"
    print(f"logprobs batched V={V} {kind}: worst error / bound = {w:.3f}")
