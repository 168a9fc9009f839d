"""Embedding jobs in the continuous-batching scheduler (csrc/runtime/scheduler.cpp submit_embed /
wait_embed) on the CPU, over the deterministic stand-in engine (``_cpu.FakeSlotEngine``): its
``embed_begin`` returns a vector that is a pure function of the input's tokens, pooling and
normalize, records every call's inputs and rows, and its admissions and embedding passes in order."""
import time

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.runtime import load_cpu
from test_scheduler import VOCAB, run, sequential

PIPELINE = {"on": False}


@pytest.fixture(autouse=True, params=[False, True], ids=["sync", "pipelined"])
def _pipeline(request):
    PIPELINE["on"] = request.param
    yield


def make(n_slots=5, max_batch=4, n_ctx=64, step_us=200):
    cpu = load_cpu()
    eng = cpu.FakeSlotEngine(n_slots, max_batch, n_ctx, VOCAB, step_us)
    eng.set_pipeline(PIPELINE["on"])
    return eng, cpu.BatchScheduler(eng)


def wait_embed(sched, jid, timeout=20.0):
    t0 = time.time()
    while time.time() - t0 < timeout:
        r = sched.wait_embed(jid, 50)
        if r["done"]:
            sched.release(jid)
            return r
    raise AssertionError("embedding job did not finish")


def want(inputs, pooling, normalize):
    ev = load_cpu().FakeSlotEngine.embed_vector
    return [np.asarray(ev(list(i), pooling, normalize), np.float32) for i in inputs]


def until(cond, timeout=10.0):
    t0 = time.time()
    while not cond():
        assert time.time() - t0 < timeout, "condition not reached"
        time.sleep(0.0005)


def test_job_larger_than_the_free_slots_takes_several_passes():
    eng, sched = make(n_slots=3)     # two scheduler slots (slot 0 stays with generate())
    inputs = [[3 + i, 50, 60 + i] + [7] * i for i in range(5)]
    for pooling, normalize in ((1, False), (3, True), (0, True)):
        n0 = len(eng.embed_calls)
        r = wait_embed(sched, sched.submit_embed(inputs, pooling, normalize))
        assert r["finish"] == "done" and r["error"] == ""
        got = [np.asarray(v) for v in r["vectors"]]
        assert len(got) == 5
        for g, w in zip(got, want(inputs, pooling, normalize)):      # each vector its own input's
            assert g.shape == w.shape and np.array_equal(g, w)
        calls = eng.embed_calls[n0:]
        assert [c[0] for c in calls] == [2, 2, 1]
        assert [c[1] for c in calls] == [7, 11, 7]
        assert all(sorted(s) == [1, 2][:len(s)] for s in eng.embed_slots[n0:])   # never slot 0
    assert np.asarray(r["vectors"][4]).shape == (7 * load_cpu().FakeSlotEngine.EMBED_DIM,)   # none: the rows
    sched.shutdown()


def test_arrival_order_between_a_job_and_requests():
    eng, sched = make(n_slots=2, step_us=1000)     # ONE scheduler slot
    a = sched.submit([11, 2, 3], 12, {}, [])       # holds the slot for a dozen steps
    j = sched.submit_embed([[22, 5], [23, 6]], 1, False)
    b = sched.submit([33, 2, 3], 3, {}, [])        # younger than the job: it must wait for it
    ta, _ = run(sched, a)
    assert wait_embed(sched, j)["finish"] == "done"
    tb, _ = run(sched, b)
    assert ta == sequential([11, 2, 3], 12, 64) and tb == sequential([33, 2, 3], 3, 64)
    # admissions [0, first token] and passes [1, first token of the first input], in order
    assert eng.events == [[0, 11], [1, 22], [1, 23], [0, 33]]
    # ... and a request that is OLDER than a job goes first when both wait for the slot
    eng, sched = make(n_slots=2, step_us=1000)
    a = sched.submit([11, 2, 3], 12, {}, [])
    b = sched.submit([33, 2, 3], 3, {}, [])
    j = sched.submit_embed([[22, 5]], 1, False)
    run(sched, a), run(sched, b)
    wait_embed(sched, j)
    assert eng.events == [[0, 11], [0, 33], [1, 22]]
    sched.shutdown()


def test_row_cap_while_a_row_decodes():
    eng, sched = make(n_slots=5, step_us=300, n_ctx=4096)      # four scheduler slots
    eng.set_prefill_chunk(16)                      # prefill_part_tokens(): the per-pass row bound
    prompt = [9, 8, 7]
    a = sched.submit(prompt, 400, {}, [])          # decodes throughout (400 steps of 0.3 ms)
    until(lambda: sched.wait(a, 0, 1)["tokens"])
    inputs = [[40 + i] * 10 for i in range(5)] + [[60] * 20]     # 10-token inputs, one longer than the cap
    r = wait_embed(sched, sched.submit_embed(inputs, 1, False))
    assert r["finish"] == "done"
    assert not sched.wait(a, 0, 1)["done"], "the generation ended before the job: nothing was capped"
    calls = eng.embed_calls
    # three slots are free, but two 10-token inputs are 20 rows > 16: one input per pass, and the
    # 20-token input still goes (always at least one input)
    assert [c[0] for c in calls] == [1] * 6 and [c[1] for c in calls] == [10] * 5 + [20]
    for g, w in zip(r["vectors"], want(inputs, 1, False)):
        assert np.array_equal(np.asarray(g), w)
    sched.cancel(a)
    toks, ra = run(sched, a)
    assert toks == sequential(prompt, 400, 4096)[:len(toks)]       # the row never noticed
    # nothing decodes now: no cap, as many whole inputs as there are free slots
    n0 = len(eng.embed_calls)
    wait_embed(sched, sched.submit_embed(inputs, 1, False))
    assert [c[0] for c in eng.embed_calls[n0:]] == [4, 2]
    sched.shutdown()


def test_borrowed_slot_keeps_no_prefix():
    eng, sched = make(n_slots=2)                   # one scheduler slot: the job must borrow it
    p1 = list(range(10, 40))
    t1, _ = run(sched, sched.submit(p1, 4, {}, []))
    reused = sched.stats()["reused_tokens"]
    assert wait_embed(sched, sched.submit_embed([[5, 6, 7]], 3, False))["finish"] == "done"
    # the same conversation again: its prefix is NOT resident any more (the fake refuses a reused
    # prefix that is not in its KV: "reused prefix is not resident" / "differs")
    p2 = p1 + t1[:-1] + [77]
    t2, r2 = run(sched, sched.submit(p2, 4, {}, []))
    assert r2["finish"] != "error", r2["error"]
    assert t2 == sequential(p2, 4, 64) and r2["n_prefilled"] == len(p2)
    assert sched.stats()["reused_tokens"] == reused
    sched.shutdown()


def test_cancel_before_the_last_pass():
    eng, sched = make(n_slots=2, step_us=20000)    # one slot, 20 ms per pass: five passes
    inputs = [[3 + i, 4] for i in range(5)]
    j = sched.submit_embed(inputs, 1, False)
    until(lambda: len(eng.embed_calls) >= 1)
    sched.cancel(j)
    r = wait_embed(sched, j)
    assert r["done"] and r["finish"] == "cancelled" and r["vectors"] == []
    assert len(eng.embed_calls) < 5
    assert sched.stats()["embed_jobs"] == 0
    # the scheduler goes on: a later job and a later generation run
    assert wait_embed(sched, sched.submit_embed(inputs[:1], 1, False))["finish"] == "done"
    assert run(sched, sched.submit([1, 2, 3], 3, {}, []))[0] == sequential([1, 2, 3], 3, 64)
    sched.shutdown()


def test_engine_exception_reaches_the_waiter():
    eng, sched = make(n_slots=3)
    eng.embed_fail(True)
    r = wait_embed(sched, sched.submit_embed([[1, 2], [3]], 1, True))
    assert r["finish"] == "error" and "injected embed fault" in r["error"] and r["vectors"] == []
    eng.embed_fail(False)
    r = wait_embed(sched, sched.submit_embed([[1, 2], [3]], 1, True))
    assert r["finish"] == "done" and len(r["vectors"]) == 2
    sched.shutdown()


def test_refused_jobs_and_stats():
    eng, sched = make(n_slots=3, n_ctx=16)
    for bad in ([], [[]], [[1] * 17]):
        with pytest.raises(RuntimeError):
            sched.submit_embed(bad, 1, False)
    with pytest.raises(RuntimeError):
        sched.submit_embed([[1]], 4, False)
    full = [[2] * 16, [3, 4, 5]]                   # an input may fill the whole context
    assert wait_embed(sched, sched.submit_embed(full, 2, False))["finish"] == "done"
    assert wait_embed(sched, sched.submit_embed([[7]], 1, False))["finish"] == "done"
    st = sched.stats()
    assert (st["embed_jobs"], st["embed_inputs"], st["embed_tokens"]) == (2, 3, 20)
    assert st["admitted"] == 0 and st["active"] == 0 and st["pending"] == 0
    with pytest.raises(RuntimeError):
        sched.wait_embed(12345, 1)
    sched.shutdown()


def test_shutdown_ends_a_waiting_job():
    eng, sched = make(n_slots=2, step_us=20000)
    j = sched.submit_embed([[3 + i] for i in range(4)], 1, False)
    until(lambda: len(eng.embed_calls) >= 1)
    sched.shutdown()
    r = sched.wait_embed(j, 1)
    assert r["done"] and r["finish"] in ("cancelled", "done")
