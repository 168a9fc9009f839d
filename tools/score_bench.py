"""Prompt scoring on the engine the bench serves with (n_slots = 7, scoring on): ``Engine.score`` of
one T-token input against, in the same process, the admission of the same tokens (``slot_begin``:
the prefill + lm_head GEMV of the last row + sampler = the first token) and their embedding
(``Engine.embed``, pooling last: the same prefill with neither head). The arms alternate, warm,
several repeats. ``head_share`` = (score - embed) / score: the output norm, the scoring head over
all T rows and the record copy. ``--layers N`` cuts the model to N layers (a shorter file to write).
On a BF16 / F16 model two more arms run on a random head of the model's shape, each timed from the
host around one launch and a synchronise: the fused ``score_head_w16`` and what the lm_head path
would do instead for the same rows, ``gemm`` (gemm_bf16w) into a [T][V] fp32 buffer - that arm leaves
the log-softmax over the stored logits out. Prints one JSON line (``--out FILE`` also writes it).

    python tools/score_bench.py [--model llama3-8b-bf16 --layers 8] [--T 512] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def head_arms(T, V, K, quant):
    """[fused scoring head, gemm into stored [T][V] logits] on a random 16-bit head, or [] for other types."""
    if quant not in ("bf16", "f16"):
        return []
    import torch
    from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
    from llama_fastapi_k8s_gpu_amd.ops import GEMM_STORE
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    hip, dt = load_hip(), torch.bfloat16 if quant == "bf16" else torch.float16
    qt = int(GGMLType.BF16 if quant == "bf16" else GGMLType.F16)
    g = torch.Generator(device="cuda").manual_seed(0)
    w = (torch.randn((V, K), device="cuda", generator=g) * 0.02).to(dt)
    x = torch.randn((T, K), device="cuda", generator=g).to(dt)
    xb = x.to(torch.bfloat16)   # gemm takes bf16 rows whatever the weight type
    tg = torch.randint(0, V, (T,), device="cuda", generator=g, dtype=torch.int32)
    tgl = tg.tolist()
    words = hip.score_head_w16_workspace_words(T, V)
    part, rec = torch.empty(words, device="cuda"), torch.empty((T, 4), device="cuda")
    logits = torch.empty((T, V), device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def fused():
        hip.score_head_w16(w.data_ptr(), qt, V, K, V, x.data_ptr(), T, tg.data_ptr(), tgl, part.data_ptr(), words,
                           rec.data_ptr(), st)
        torch.cuda.synchronize()

    def stored():
        hip.gemm(w.data_ptr(), qt, V, K, xb.data_ptr(), T, logits.data_ptr(), 0, V, GEMM_STORE, st)
        torch.cuda.synchronize()
    return [fused, stored]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b-q4_k_m")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, cached_synthetic_gguf, write_synthetic_gguf
    from llama_fastapi_k8s_gpu_amd.runtime import load_hip
    if args.layers:
        cache = os.environ.get("SYNTH_MODEL_DIR") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "llama_amd_models")
        os.makedirs(cache, exist_ok=True)
        path = os.path.join(cache, f"{args.model}-L{args.layers}.gguf")
        if not os.path.exists(path):
            write_synthetic_gguf(replace(SPECS[args.model], n_layer=args.layers), path, seed=0)
    else:
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
    head = head_arms(args.T, int(V), eng.hparams["n_embd"], SPECS[args.model].quant)
    score, embed, admit, fused, stored = [], [], [], [], []
    for f in head:
        f()   # warm
    for _ in range(args.reps):    # the arms alternate: one clock state for all
        x = [int(t) for t in rng.integers(0, V, args.T)]
        score.append(ms(lambda: eng.score([x], [1])))
        embed.append(ms(lambda: eng.embed([1], [x], 3, False)))
        admit.append(ms(lambda: eng.slot_begin(1, x, 0, sp)))
        if head:
            fused.append(ms(head[0]))
            stored.append(ms(head[1]))
    med = lambda v: round(float(np.median(v)), 2)  # noqa: E731
    res = {"model": args.model, "layers": int(eng.hparams["n_layer"]), "T": args.T, "reps": args.reps, "n_vocab": int(V),
           "score_ms": [round(t, 2) for t in score], "score_ms_med": med(score),
           "embed_last_ms": [round(t, 2) for t in embed], "embed_last_ms_med": med(embed),
           "prefill_first_token_ms": [round(t, 2) for t in admit], "prefill_first_token_ms_med": med(admit),
           "head_share": round((med(score) - med(embed)) / med(score), 3),
           # what storing the logits would have written and read back instead
           "logits_bytes_avoided": 2 * args.T * int(V) * 4}
    if head:
        res.update({"score_head_w16_ms": [round(t, 3) for t in fused], "score_head_w16_ms_med": med(fused),
                    "gemm_store_logits_ms": [round(t, 3) for t in stored], "gemm_store_logits_ms_med": med(stored)})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
