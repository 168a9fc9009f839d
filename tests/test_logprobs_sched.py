"""Log-probability entries through the continuous-batching scheduler, on the CPU over the
deterministic stand-in engine: its entries are a function of (slot, position, token) alone
(log p = -(1000 slot + position) / 1024, top-j = (token + j mod vocab, log p - j)), so every entry
tells which step of which row it came from. They must arrive with exactly their tokens, in token
order, through synchronous and pipelined steps, joint and chunked admissions, and a request that
leaves early keeps only its own."""
import pytest

from llama_fastapi_k8s_gpu_amd.engine.sampling import SamplingParams
from llama_fastapi_k8s_gpu_amd.runtime import load_cpu
from test_scheduler import VOCAB, sequential

N_CTX = 64


def make(pipeline, n_slots=5, max_batch=4, step_us=200):
    cpu = load_cpu()
    eng = cpu.FakeSlotEngine(n_slots, max_batch, N_CTX, VOCAB, step_us)
    eng.set_pipeline(pipeline)
    return eng, cpu.BatchScheduler(eng)


def collect(sched, rid, chunk_check=True):
    """Poll like the backend does: every wait returns the entries of exactly the tokens it returns."""
    toks, lps = [], []
    for _ in range(2000):
        r = sched.wait(rid, len(toks), 50)
        if chunk_check:
            assert len(r["logprobs"]) in (0, len(r["tokens"]))
        toks += r["tokens"]
        lps += r["logprobs"]
        if r["done"]:
            sched.release(rid)
            return toks, lps, r
    raise AssertionError("request did not finish")


def check_entries(prompt, toks, lps, n):
    assert len(lps) == len(toks)
    slots = set()
    for k, (tok, (lp, top)) in enumerate(zip(toks, lps)):
        code = round(-lp * 1024)
        slots.add(code // 1000)
        assert code % 1000 == len(prompt) + k, f"token {k} carries the entry of position {code % 1000}"
        assert top == [((tok + j) % VOCAB, lp - j) for j in range(n)], f"token {k}: not its own entry"
    assert len(slots) == 1, f"entries of several rows: slots {slots}"


@pytest.mark.parametrize("pipeline", [False, True], ids=["sync", "pipelined"])
def test_entries_arrive_with_their_tokens(pipeline):
    eng, sched = make(pipeline)
    reqs = [([1, 2, 3, 4 + i], 12 + 3 * i, [0, 5, 0, 2][i]) for i in range(4)]
    ids = [sched.submit(p, m, {"n_probs": n}, []) for p, m, n in reqs]
    for rid, (p, m, n) in zip(ids, reqs):
        toks, lps, _ = collect(sched, rid)
        assert toks == sequential(p, m, N_CTX)
        if n:
            check_entries(p, toks, lps, n)
        else:
            assert lps == []
    assert eng.max_rows == 4
    sched.shutdown()


@pytest.mark.parametrize("pipeline", [False, True], ids=["sync", "pipelined"])
def test_wait_slices_entries_with_tokens(pipeline):
    eng, sched = make(pipeline)
    p = [9, 8, 7]
    rid = sched.submit(p, 20, {"n_probs": 3}, [])
    toks, lps, _ = collect(sched, rid, chunk_check=False)
    sched2 = make(pipeline)[1]
    rid2 = sched2.submit(p, 20, {"n_probs": 3}, [])
    while not sched2.wait(rid2, 0, 50)["done"]:
        pass
    for have in (0, 1, 7, 19, 20):
        r = sched2.wait(rid2, have, 0)
        assert r["tokens"] == toks[have:]
        assert len(r["logprobs"]) == len(r["tokens"])
        assert [e[0] for e in r["logprobs"]] == [e[0] for e in lps[have:]]
    check_entries(p, toks, lps, 3)
    sched.shutdown()
    sched2.shutdown()


@pytest.mark.parametrize("pipeline", [False, True], ids=["sync", "pipelined"])
def test_retired_and_cancelled_requests_keep_their_own_entries(pipeline):
    """A short request ends while a long one goes on (under pipelining its row's next step is already
    queued: that token and its entry are dropped); a cancelled one stops early; the request admitted
    into the freed slot starts with its own entries."""
    eng, sched = make(pipeline, n_slots=3, max_batch=2, step_us=500)
    long_p, short_p, late_p = [1, 2, 3], [4, 5], [6, 7, 8, 9]
    rl = sched.submit(long_p, 40, {"n_probs": 2}, [])
    rs = sched.submit(short_p, 4, {"n_probs": 4}, [])
    rc = sched.submit(late_p, 30, {"n_probs": 1}, [])   # waits for the short one's slot
    ts, ls, r = collect(sched, rs)
    assert len(ts) == 4 and r["finish"] == "length"
    check_entries(short_p, ts, ls, 4)
    first = sched.wait(rc, 0, 2000)
    assert first["tokens"]
    sched.cancel(rc)
    tc, lc, r = collect(sched, rc)
    assert r["finish"] == "cancelled" and tc == sequential(late_p, 30, N_CTX)[:len(tc)]
    check_entries(late_p, tc, lc, 1)
    tl, ll, _ = collect(sched, rl)
    assert tl == sequential(long_p, 40, N_CTX)
    check_entries(long_p, tl, ll, 2)
    sched.shutdown()


def test_chunked_admission_first_entry():
    eng, sched = make(True, step_us=300)
    eng.set_prefill_chunk(8)
    a = sched.submit([1, 2, 3], 30, {"n_probs": 2}, [])
    assert sched.wait(a, 0, 2000)["tokens"]
    long_p = list(range(10, 40))
    b = sched.submit(long_p, 10, {"n_probs": 3}, [])
    tb, lb, _ = collect(sched, b)
    check_entries(long_p, tb, lb, 3)
    ta, la, _ = collect(sched, a)
    check_entries([1, 2, 3], ta, la, 2)
    assert sched.stats()["chunked_admissions"] == 1
    sched.shutdown()


def test_gpu_compatible_default_keeps_the_host_route():
    p = SamplingParams(temperature=0.0, n_probs=3)
    assert not p.gpu_compatible(32000)
    assert p.gpu_compatible(32000, 20) and p.gpu_compatible(32000, max_logprobs=3)
    assert not SamplingParams(temperature=0.0, n_probs=21).gpu_compatible(32000, 20)
    assert SamplingParams(temperature=0.0).gpu_compatible(32000)
