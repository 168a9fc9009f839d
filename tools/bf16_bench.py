"""BF16 serving against its F16 twin, in one process: single-row decode ms / token, the B = 6
batched step and a 512-token prefill + first token, on ``llama3-8b-bf16`` (f32-activation GEMV
launches and gemm_bf16w) and on ``llama3-8b-f16`` (the existing F16 GEMV and gemm_dq). Medians of
``--reps`` warm repeats, the two models alternating; every figure stands beside the byte floor of
its weight stream at 6.3 TB/s (a token or a step reads every matrix once; the prefill reads them at
least once). ``--layers N`` cuts both models to N layers (a shorter file to write; the floors
follow). Prints one JSON line (``--out FILE`` also writes it).

    python tools/bf16_bench.py [--layers 32] [--reps 7] [--out profiles/bf16_bench.json]
"""
import argparse
import json
import os
import sys
import time
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--B", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tokens", type=int, default=32, help="decode tokens / batched steps per repeat")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    cache = os.environ.get("SYNTH_MODEL_DIR") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "llama_amd_models")
    os.makedirs(cache, exist_ok=True)
    greedy = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
    rng = np.random.default_rng(0)
    engines, info = {}, {}
    for name in ("llama3-8b-bf16", "llama3-8b-f16"):
        spec = SPECS[name] if not args.layers else replace(SPECS[name], n_layer=args.layers)
        path = os.path.join(cache, f"{name}-L{spec.n_layer}.gguf")
        if not os.path.exists(path):
            write_synthetic_gguf(spec, path, seed=0)
        t = GGUFReader(path).tensors   # a token reads every matrix but the embedding table
        wbytes = sum(v.nbytes for k, v in t.items() if len(v.shape) == 2 and k != "token_embd.weight")
        engines[name] = load_hip().Engine(path, n_ctx=1024, n_batch=args.T, device=0, use_graph=True, n_slots=args.B + 1)
        info[name] = {"layers": spec.n_layer, "weight_gb": round(wbytes / 1e9, 2),
                      "byte_floor_ms": round(wbytes / HBM_BYTES_PER_S * 1e3, 3)}
    V = engines["llama3-8b-bf16"].hparams["n_vocab"]

    def ms(f):   # f ends in a device synchronise (it returns tokens)
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    def decode(eng):   # one slot: the single-row graph
        eng.slot_begin(0, [int(t) for t in rng.integers(0, V, 16)], 0, greedy)
        return ms(lambda: [eng.batch_step([0]) for _ in range(args.tokens)]) / args.tokens

    def batch(eng):
        slots = list(range(args.B))
        for s in slots:
            eng.slot_begin(s, [int(t) for t in rng.integers(0, V, 16 + s)], 0, greedy)
        return ms(lambda: [eng.batch_step(slots) for _ in range(args.tokens)]) / args.tokens

    def prefill(eng):
        x = [int(t) for t in rng.integers(0, V, args.T)]
        return ms(lambda: eng.slot_begin(args.B, x, 0, greedy))
    arms = {"decode_ms_per_token": decode, f"batch{args.B}_step_ms": batch, f"prefill{args.T}_first_token_ms": prefill}
    runs = {n: {a: [] for a in arms} for n in engines}
    for rep in range(args.reps + 1):   # repeat 0 warms every shape and is dropped
        for a, f in arms.items():
            for n, eng in engines.items():   # the models alternate: one clock state for both
                v = f(eng)
                if rep:
                    runs[n][a].append(round(v, 3))
    res = {"T": args.T, "B": args.B, "reps": args.reps, "tokens_per_repeat": args.tokens, "hbm_tb_per_s": 6.3}
    for n in engines:
        res[n] = dict(info[n], **{a + "_med": round(float(np.median(v)), 3) for a, v in runs[n].items()}, runs=runs[n])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
