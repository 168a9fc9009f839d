"""Qwen3-MoE step timing on the synthetic Qwen3-30B-A3B shape (no HTTP): single-row ms/token, the
batched step at B = 1 / 6 / 8, a 512-token prompt chunk - each next to the time its bytes need at the
README's 6.3 TB/s: per token the active experts (k of E), attention, routers and the head are streamed
once; a batched step streams the experts its rows route to (counted as min(E, B k), an upper bound) and a
chunk all of them. Writes one JSON object (--out) and prints it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_TBS = 6.3


def streamed_bytes(path, E, k):
    """(bytes every token reads: attention, norms, routers, head; bytes of all experts)."""
    from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
    fixed = experts = 0
    for name, t in GGUFReader(path).tensors.items():
        n = int(t.nbytes)
        if "_exps." in name:
            experts += n
        elif name != "token_embd.weight":
            fixed += n
    return fixed, experts


def timed(fn, reps):
    fn()  # warm
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best.append((time.perf_counter() - t0) * 1e3)
    return sorted(best)[len(best) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen3-30b-a3b-q4_k_m")
    ap.add_argument("--n-ctx", type=int, default=1024)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,6,8")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "qwen3moe_bench.json"))
    args = ap.parse_args()
    import numpy as np
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    d = os.environ.get("SYNTH_MODEL_DIR") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "llama_amd_models")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"{args.model}-s0.gguf")
    if not os.path.exists(path):
        t0, n = time.time(), [0]

        def log(name):
            n[0] += 1
            if n[0] % 40 == 0:
                print(f"[gen] {n[0]} tensors, {time.time() - t0:.0f}s", file=sys.stderr, flush=True)
        write_synthetic_gguf(args.model, path, seed=0, log=log)
    spec = SPECS[args.model]
    E, k = spec.n_expert, spec.n_expert_used
    fixed, experts = streamed_bytes(path, E, k)
    floor = lambda b: round(b / (HBM_TBS * 1e12) * 1e3, 3)   # ms at 6.3 TB/s
    res = {"model": args.model, "hbm_tb_s": HBM_TBS, "bytes_fixed": fixed, "bytes_experts": experts}
    t0 = time.time()
    eng = load_hip().Engine(path, n_ctx=args.n_ctx, n_batch=512, device=0, use_graph=True, n_slots=8)
    res["load_s"] = round(time.time() - t0, 1)
    res["batch_plan_ffn"] = eng.batch_plan(6)[0]["ffn"]
    rng = np.random.default_rng(0)
    toks = [int(t) for t in rng.integers(0, eng.hparams["n_vocab"], args.prompt)]
    res["prefill_tokens"] = args.prompt
    res["prefill_ms"] = round(timed(lambda: eng.eval_logits(toks, 0), args.reps), 3)
    res["prefill_floor_ms"] = floor(fixed + experts)
    greedy = {"temperature": 0.0, "top_k": 1, "repeat_penalty": 1.0}
    gen = lambda n: eng.generate(toks[:32], 0, n, greedy, [], None, None)
    long_ms, short_ms = timed(lambda: gen(args.steps + 1), args.reps), timed(lambda: gen(1), args.reps)
    res["decode_ms_per_token"] = round((long_ms - short_ms) / args.steps, 4)
    res["decode_floor_ms"] = floor(fixed + experts * k / E)
    sp = {"temperature": 1.2, "top_p": 0.9, "frequency_penalty": 0.7, "presence_penalty": 0.8, "seed": 1}
    for s in range(8):
        eng.slot_begin(s, [int(t) for t in rng.integers(0, eng.hparams["n_vocab"], 300)], 0, sp)
    for B in [int(b) for b in args.batches.split(",")]:
        slots = list(range(B))
        ms = timed(lambda: [eng.batch_step(slots) for _ in range(args.steps)], args.reps) / args.steps
        res[f"B{B}_ms_per_step"] = round(ms, 4)
        res[f"B{B}_floor_ms"] = floor(fixed + experts * min(E, B * k) / E)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
