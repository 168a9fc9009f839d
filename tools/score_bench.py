"""Prompt scoring on the engine the bench serves with (n_slots = 7, scoring on): ``Engine.score`` of
one T-token input against, in the same process, the admission of the same tokens (``slot_begin``:
the prefill + lm_head GEMV of the last row + sampler = the first token) and their embedding
(``Engine.embed``, pooling last: the same prefill with neither head). The arms alternate, warm,
several repeats. ``head_share`` = (score - embed) / score: the output norm, the scoring head over
all T rows and the record copy. Prints one JSON line (``--out FILE`` also writes it).

    python tools/score_bench.py [--T 512] [--reps 7] [--out profiles/score_bench.json]
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
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import cached_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    path = cached_synthetic_gguf(args.model)
    eng = load_hip().Engine(path, n_ctx=1024, n_batch=512, device=0, use_graph=True, n_slots=7, scoring=True)
    rng = np.random.default_rng(0)
    V = eng.hparams["n_vocab"]
    sp = {"temperature": 1.2, "top_p": 0.9, "frequency_penalty": 0.7, "presence_penalty": 0.8, "seed": 1}

    def ms(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3
    warm = [int(t) for t in rng.integers(0, V, args.T)]
    eng.score([warm], [1])
    eng.embed([1], [warm], 3, False)
    eng.slot_begin(1, warm, 0, sp)
    score, embed, admit = [], [], []
    for _ in range(args.reps):    # the arms alternate: one clock state for all
        x = [int(t) for t in rng.integers(0, V, args.T)]
        score.append(ms(lambda: eng.score([x], [1])))
        embed.append(ms(lambda: eng.embed([1], [x], 3, False)))
        admit.append(ms(lambda: eng.slot_begin(1, x, 0, sp)))
    med = lambda v: round(float(np.median(v)), 2)  # noqa: E731
    res = {"model": args.model, "T": args.T, "reps": args.reps, "n_vocab": int(V),
           "score_ms": [round(t, 2) for t in score], "score_ms_med": med(score),
           "embed_last_ms": [round(t, 2) for t in embed], "embed_last_ms_med": med(embed),
           "prefill_first_token_ms": [round(t, 2) for t in admit], "prefill_first_token_ms_med": med(admit),
           "head_share": round((med(score) - med(embed)) / med(score), 3),
           # what storing the logits would have written and read back instead
           "logits_bytes_avoided": 2 * args.T * int(V) * 4}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
