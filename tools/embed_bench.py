"""Text embeddings on the engine the bench serves with (n_slots = 7): ``Engine.embed`` of six
387-token inputs packed in one call against the same six one at a time, warm, several repeats - and,
in the same process, the joint admission (``slots_begin``) and single admission (``slot_begin``) of
the same rows, which run the lm_head and the sampler on top of the same prefill. Prints one JSON
line (``--out FILE`` also writes it); run under ``rocprofv3 --kernel-trace --stats`` for the two
pooling kernels' own time.

    python tools/embed_bench.py [--T 387] [--n 6] [--reps 5] [--pooling 1] [--out profiles/embed_bench.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b-q4_k_m")
    ap.add_argument("--T", type=int, default=387)
    ap.add_argument("--n", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pooling", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import cached_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    path = cached_synthetic_gguf(args.model)
    eng = load_hip().Engine(path, n_ctx=1024, n_batch=512, device=0, use_graph=True, n_slots=7)
    rng = np.random.default_rng(0)
    V, d = eng.hparams["n_vocab"], eng.hparams["n_embd"]
    sp = {"temperature": 1.2, "top_p": 0.9, "frequency_penalty": 0.7, "presence_penalty": 0.8, "seed": 1}
    slots = list(range(1, 1 + args.n))

    def inputs():
        return [[int(t) for t in rng.integers(0, V, args.T)] for _ in range(args.n)]

    def ms(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3
    eng.embed(slots, inputs(), args.pooling, True)        # warm (first-use allocations)
    eng.slots_begin(slots, inputs(), [0] * args.n, [sp] * args.n)
    packed, alone, joint, single = [], [], [], []
    for _ in range(args.reps):                            # the four arms alternate: one clock state for all
        ins = inputs()
        packed.append(ms(lambda: eng.embed(slots, ins, args.pooling, True)))
        alone.append(ms(lambda: [eng.embed([s], [x], args.pooling, True) for s, x in zip(slots, ins)]) / args.n)
        joint.append(ms(lambda: eng.slots_begin(slots, ins, [0] * args.n, [sp] * args.n)))
        single.append(ms(lambda: [eng.slot_begin(s, x, 0, sp) for s, x in zip(slots, ins)]) / args.n)
    med = lambda v: round(float(np.median(v)), 2)  # noqa: E731
    rows = args.n * args.T
    res = {"model": args.model, "T": args.T, "inputs": args.n, "rows": rows, "pooling": args.pooling,
           "reps": args.reps, "prefill_t16": bool(eng.prefill_t16),
           "embed_packed_ms": [round(t, 2) for t in packed], "embed_packed_ms_med": med(packed),
           "embed_alone_ms_each": [round(t, 2) for t in alone], "embed_alone_ms_each_med": med(alone),
           "joint_admission_ms": [round(t, 2) for t in joint], "joint_admission_ms_med": med(joint),
           "single_admission_ms_each": [round(t, 2) for t in single], "single_admission_ms_each_med": med(single),
           # what the two pooling launches move: the rows twice, the partial rows out and back in
           "pool_bytes": 2 * rows * d * 4 + 2 * (rows // 64 + args.n) * d * 4}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
