"""The Q8_0 KV cache against the f16 cache, in one process, on the synthetic Llama-3-8B Q4_K_M: the
single-row decode step and the B = 6 batched step with every row at context length L (768, 4096,
16384), and a 512-token prefill + first token. Two engines that differ only in ``kv_type``; medians of
``--reps`` warm repeats, the engines alternating; every step figure stands beside the bytes of K / V
the step reads and their time at 6.3 TB/s (the weights add their 4.6 GB to either engine alike).
``--layers N`` cuts the model to N layers. Prints one JSON line (``--out FILE`` also writes it).

    python tools/kv_q8_bench.py [--layers 32] [--reps 7] [--out profiles/kv_q8_bench.json]
"""
import argparse
import json
import os
import sys
import time
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12
KV_BYTES_PER_VALUE = {"f16": 2.0, "q8_0": 34 / 32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--lengths", type=int, nargs="+", default=[768, 4096, 16384])
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--B", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tokens", type=int, default=16, help="decode tokens / batched steps per repeat")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    cache = os.environ.get("SYNTH_MODEL_DIR") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "llama_amd_models")
    os.makedirs(cache, exist_ok=True)
    name = "llama3-8b-q4_k_m"
    spec = SPECS[name] if not args.layers else replace(SPECS[name], n_layer=args.layers)
    path = os.path.join(cache, f"{name}-s0.gguf" if not args.layers else f"{name}-L{spec.n_layer}.gguf")
    if not os.path.exists(path):
        write_synthetic_gguf(spec, path, seed=0)
    greedy = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
    rng = np.random.default_rng(0)
    # every repeat advances a row by `tokens` positions past L: room for all of them
    n_ctx = max(args.lengths) + 2 * (args.reps + 1) * args.tokens + 64
    engines = {kv: load_hip().Engine(path, n_ctx=n_ctx, n_batch=args.T, device=0, use_graph=True, n_slots=args.B + 1,
                                     kv_type=kv) for kv in KV_BYTES_PER_VALUE}
    hp = engines["f16"].hparams
    V, kv_values = hp["n_vocab"], 2 * hp["n_layer"] * hp["n_head_kv"] * hp["head_dim"]   # K and V values per key

    def ms(f):   # f ends in a device synchronise (it returns tokens)
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    def steps(eng, slots):
        return ms(lambda: [eng.batch_step(slots) for _ in range(args.tokens)]) / args.tokens

    res = {"model": name, "layers": spec.n_layer, "n_ctx": n_ctx, "T": args.T, "B": args.B, "reps": args.reps,
           "tokens_per_repeat": args.tokens, "hbm_tb_per_s": 6.3,
           "device_gb": {kv: round(e.device_bytes / 1e9, 2) for kv, e in engines.items()}}
    for L in args.lengths:
        for kv, eng in engines.items():   # every row of both engines at length L (the prompt's content does not matter)
            for s in range(args.B):
                eng.slot_begin(s, [int(t) for t in rng.integers(0, V, L)], 0, greedy)
            print(f"L={L} {kv}: {args.B} rows prefilled", file=sys.stderr, flush=True)
        arms = {"decode_step_ms": [0], f"batch{args.B}_step_ms": list(range(args.B))}
        runs = {kv: {a: [] for a in arms} for kv in engines}
        for rep in range(args.reps + 1):   # repeat 0 warms every shape and is dropped
            for a, slots in arms.items():
                for kv, eng in engines.items():   # the engines alternate: one clock state for both
                    v = steps(eng, slots)
                    if rep:
                        runs[kv][a].append(round(v, 3))
        res[f"L{L}"] = {}
        for kv in engines:
            r = {}
            for a, slots in arms.items():
                kvb = len(slots) * L * kv_values * KV_BYTES_PER_VALUE[kv]
                r[a + "_med"] = round(float(np.median(runs[kv][a])), 3)
                r[a.replace("_ms", "_kv_mb")] = round(kvb / 1e6, 1)
                r[a.replace("_ms", "_kv_floor_ms")] = round(kvb / HBM_BYTES_PER_S * 1e3, 4)
            res[f"L{L}"][kv] = dict(r, runs=runs[kv])
    pre = {kv: [] for kv in engines}
    for rep in range(args.reps + 1):
        x = [int(t) for t in rng.integers(0, V, args.T)]
        for kv, eng in engines.items():
            v = ms(lambda: eng.slot_begin(args.B, x, 0, greedy))
            if rep:
                pre[kv].append(round(v, 3))
    res[f"prefill{args.T}_first_token_ms"] = {kv: {"med": round(float(np.median(v)), 3), "runs": v} for kv, v in pre.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
