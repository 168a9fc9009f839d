"""Random-init GGUF models of the BASELINE architectures (no network: real
checkpoints cannot be fetched, so every benchmark and test runs on synthetic
weights of the exact shapes and quant-type mixes - SURVEY §2.3, §7.2).

``SPECS`` holds the BASELINE.json configs plus tiny test models. Tensor types
follow the upstream Q4_K_M mix rule::

    use_more_bits(i, n) = i < n/8 or i >= 7n/8 or (i - n/8) % 3 == 2
    attn_v, ffn_down -> Q6_K when use_more_bits (70B: non-bumped attn_v -> Q5_K)
    8-expert models  -> attn_k/attn_v Q8_0
    output.weight    -> Q6_K ; token_embd -> Q4_K ; norms/router -> F32

The legacy file types ("q4_0", "q4_1", "q5_0", "q5_1") are uniform: every 2-D tensor,
token_embd included, has the file's type and output.weight is Q6_K, as llama.cpp writes them.

The 2- and 3-bit K-quant files ("q2_k", "q3_k_s", "q3_k_m") follow the rule in ``tensor_types``.

The non-linear 4-bit files ("iq4_nl", "iq4_xs") follow a model of the upstream rule, also in
``tensor_types``. The mix is not load-relevant: any mix of supported types loads.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Tuple

import numpy as np

from .constants import (FTYPE_MOSTLY_IQ4_NL, FTYPE_MOSTLY_IQ4_XS, FTYPE_MOSTLY_Q2_K, FTYPE_MOSTLY_Q3_K_M, FTYPE_MOSTLY_Q3_K_S, FTYPE_MOSTLY_Q4_0,
                        FTYPE_MOSTLY_Q4_1, FTYPE_MOSTLY_Q4_K_M, FTYPE_MOSTLY_Q5_0, FTYPE_MOSTLY_Q5_1, FTYPE_MOSTLY_Q8_0, GGMLType, GGUFValueType,
                        TOKEN_TYPE_BYTE, TOKEN_TYPE_CONTROL, TOKEN_TYPE_NORMAL)
from .constants import ARCH_QWEN3, KEY_ATTN_KEY_LENGTH, KEY_ATTN_VALUE_LENGTH, TENSOR_ATTN_K_NORM, TENSOR_ATTN_Q_NORM
from .quants import random_blocks
from .writer import GGUFWriter

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")

LLAMA3_CHAT_TEMPLATE = (
    "{% set loop_messages = messages %}{% for message in loop_messages %}{% set content = "
    "'<|start_header_id|>' + message['role'] + '<|end_header_id|>\n\n'+ message['content'] | trim + "
    "'<|eot_id|>' %}{% if loop.index0 == 0 %}{% set content = bos_token + content %}{% endif %}"
    "{{ content }}{% endfor %}{% if add_generation_prompt %}{{ '<|start_header_id|>assistant"
    "<|end_header_id|>\n\n' }}{% endif %}")
ZEPHYR_CHAT_TEMPLATE = (
    "{% for message in messages %}\n{% if message['role'] == 'user' %}\n{{ '<|user|>\n' + "
    "message['content'] + eos_token }}\n{% elif message['role'] == 'system' %}\n{{ '<|system|>\n' + "
    "message['content'] + eos_token }}\n{% elif message['role'] == 'assistant' %}\n{{ '<|assistant|>\n'"
    "  + message['content'] + eos_token }}\n{% endif %}\n{% if loop.last and add_generation_prompt %}\n"
    "{{ '<|assistant|>' }}\n{% endif %}\n{% endfor %}")
MISTRAL_CHAT_TEMPLATE = (
    "{{ bos_token }}{% for message in messages %}{% if (message['role'] == 'user') != "
    "(loop.index0 % 2 == 0) %}{{ raise_exception('Conversation roles must alternate "
    "user/assistant/user/assistant/...') }}{% endif %}{% if message['role'] == 'user' %}"
    "{{ '[INST] ' + message['content'] + ' [/INST]' }}{% elif message['role'] == 'assistant' %}"
    "{{ message['content'] + eos_token}}{% else %}{{ raise_exception('Only user and assistant "
    "roles are supported!') }}{% endif %}{% endfor %}")

CHATML_CHAT_TEMPLATE = (
    "{% for message in messages %}{{'<|im_start|>' + message['role'] + '\n' + message['content'] + "
    "'<|im_end|>' + '\n'}}{% endfor %}{% if add_generation_prompt %}{{ '<|im_start|>assistant\n' }}"
    "{% endif %}")

QWEN2_SPECIALS = {0: "<|endoftext|>", 1: "<|im_start|>", 2: "<|im_end|>"}
LLAMA3_SPECIALS = {0: "<|begin_of_text|>", 1: "<|end_of_text|>", 6: "<|start_header_id|>",
                   7: "<|end_header_id|>", 9: "<|eot_id|>"}


@dataclass
class ModelSpec:
    name: str
    n_embd: int
    n_layer: int
    n_head: int
    n_head_kv: int
    n_ff: int
    n_vocab: int
    rope_base: float
    tokenizer: str            # "bpe" | "spm"
    quant: str                # "q4_k_m" | "q8_0" | "f32" | "mixed-test" | LEGACY_QUANTS | "legacy-mixed-test"
    #                           | K23_QUANTS | "kmixed-test" | IQ4_QUANTS | "iq4-mixed-test"
    n_expert: int = 0
    n_expert_used: int = 0
    n_ctx_train: int = 8192
    rms_eps: float = 1e-5
    size_class: str = "8B"    # "8B" | "70B" (affects the Q4_K_M attn_v rule)
    weight_std: float = 0.02
    chat_template: Optional[str] = None
    arch: str = "llama"       # general.architecture: "llama" | "qwen2" | "qwen3" (keys under it; NeoX RoPE, no BOS)
    qkv_bias: bool = False    # F32 blk.N.attn_{q,k,v}.bias (Qwen2)
    tied_output: bool = False  # no output.weight: the head is token_embd.weight
    qk_norm: bool = False     # F32 blk.N.attn_{q,k}_norm.weight [head_dim] (Qwen3)
    hd: int = 0               # head width where it is not n_embd / n_head (Qwen3: attention.key_length)

    @property
    def head_dim(self) -> int:
        return self.hd or self.n_embd // self.n_head

    @property
    def n_q(self) -> int:     # rows of attn_q / columns of attn_output
        return self.head_dim * self.n_head


# uniform legacy (32-weight block) file types: quant name -> (tensor type, general.file_type)
LEGACY_QUANTS = {
    "q4_0": (GGMLType.Q4_0, FTYPE_MOSTLY_Q4_0),
    "q4_1": (GGMLType.Q4_1, FTYPE_MOSTLY_Q4_1),
    "q5_0": (GGMLType.Q5_0, FTYPE_MOSTLY_Q5_0),
    "q5_1": (GGMLType.Q5_1, FTYPE_MOSTLY_Q5_1),
}

# the 2- and 3-bit K-quant file types: quant name -> (base tensor type, general.file_type)
K23_QUANTS = {
    "q2_k": (GGMLType.Q2_K, FTYPE_MOSTLY_Q2_K),
    "q3_k_s": (GGMLType.Q3_K, FTYPE_MOSTLY_Q3_K_S),
    "q3_k_m": (GGMLType.Q3_K, FTYPE_MOSTLY_Q3_K_M),
}

# the non-linear 4-bit file types: quant name -> (base tensor type, general.file_type)
IQ4_QUANTS = {
    "iq4_nl": (GGMLType.IQ4_NL, FTYPE_MOSTLY_IQ4_NL),
    "iq4_xs": (GGMLType.IQ4_XS, FTYPE_MOSTLY_IQ4_XS),
}

SPECS: Dict[str, ModelSpec] = {
    "llama3-8b-q4_k_m": ModelSpec("Llama-3-8B", 4096, 32, 32, 8, 14336, 128256, 500000.0, "bpe", "q4_k_m"),
    "llama3-70b-q4_k_m": ModelSpec("Llama-3-70B", 8192, 80, 64, 8, 28672, 128256, 500000.0, "bpe", "q4_k_m",
                                   size_class="70B"),
    "mixtral-8x7b-q4_k_m": ModelSpec("Mixtral-8x7B", 4096, 32, 32, 8, 14336, 32000, 1e6, "spm", "q4_k_m",
                                     n_expert=8, n_expert_used=2, n_ctx_train=32768),
    "tinyllama-1.1b-q8_0": ModelSpec("TinyLlama-1.1B", 2048, 22, 32, 4, 5632, 32000, 10000.0, "spm", "q8_0",
                                     n_ctx_train=2048),
    # --- tiny models for tests (same code paths, seconds to build)
    "tiny-llama3-q4_k_m": ModelSpec("tiny-llama3", 256, 4, 4, 2, 512, 0, 500000.0, "bpe", "q4_k_m",
                                    n_ctx_train=1024),
    "tiny-llama3-mixed": ModelSpec("tiny-llama3-mixed", 256, 4, 4, 2, 512, 0, 500000.0, "bpe", "mixed-test",
                                   n_ctx_train=1024),
    "tiny-tinyllama-q8_0": ModelSpec("tiny-tinyllama", 512, 3, 8, 1, 768, 0, 10000.0, "spm", "q8_0",
                                     n_ctx_train=1024),
    "tiny-mixtral-q4_k_m": ModelSpec("tiny-mixtral", 256, 3, 4, 2, 512, 0, 1e6, "spm", "q4_k_m",
                                     n_expert=4, n_expert_used=2, n_ctx_train=1024),
    # tensor-parallel test shapes: per-rank head / FFN slices stay multiples of 256 at TP=2
    "tiny-llama3-tp": ModelSpec("tiny-llama3-tp", 512, 2, 8, 4, 1024, 0, 500000.0, "bpe", "q4_k_m",
                                n_ctx_train=1024),
    # 4 kv heads of 256 q columns each: uneven tensor_split ratios and TP=3 are representable
    "tiny-llama3-tp4": ModelSpec("tiny-llama3-tp4", 1024, 2, 8, 4, 1024, 0, 500000.0, "bpe", "q4_k_m",
                                 n_ctx_train=1024),
    "tiny-mixtral-tp": ModelSpec("tiny-mixtral-tp", 512, 2, 8, 4, 1024, 0, 1e6, "spm", "q4_k_m",
                                 n_expert=4, n_expert_used=2, n_ctx_train=1024),
    # wide enough for several 2048-feature FFN slices (fused decode FFN hand-off), partial last slice
    "tiny-llama3-wide": ModelSpec("tiny-llama3-wide", 1024, 3, 8, 2, 5120, 0, 500000.0, "bpe", "q4_k_m",
                                  n_ctx_train=1024),
    # Q8_0 with n_ff = 576: 2F = 1152 gate/up rows is NOT a multiple of 256 (the attention
    # weight touch's per-CU gate/up segments must clamp to the plane end)
    "tiny-q8-oddff": ModelSpec("tiny-q8-oddff", 256, 2, 4, 2, 576, 0, 10000.0, "spm", "q8_0",
                               n_ctx_train=1024),
    # one layer: each engine path against the rounding-emulating reference op for op (with more
    # layers, 1e-7 summation-order differences flip q8 / bf16 roundings downstream)
    "tiny-llama3-1l": ModelSpec("tiny-llama3-1l", 256, 1, 4, 2, 512, 0, 500000.0, "bpe", "q4_k_m",
                                n_ctx_train=1024),
    "tiny-mixed-1l": ModelSpec("tiny-mixed-1l", 256, 1, 4, 2, 512, 0, 500000.0, "bpe", "mixed-test",
                               n_ctx_train=1024),
    "tiny-q8-1l": ModelSpec("tiny-q8-1l", 512, 1, 8, 1, 768, 0, 10000.0, "spm", "q8_0", n_ctx_train=1024),
    "tiny-mixtral-1l": ModelSpec("tiny-mixtral-1l", 256, 1, 4, 2, 512, 0, 1e6, "spm", "q4_k_m",
                                 n_expert=4, n_expert_used=2, n_ctx_train=1024),
    # 32 layers (the 8B's depth) at d 1024: the Q4_K_M bump pattern over a full-depth stack
    "tiny-llama3-deep32": ModelSpec("tiny-llama3-deep32", 1024, 32, 8, 2, 512, 0, 500000.0, "bpe", "q4_k_m",
                                    n_ctx_train=1024),
    # d = 4096 with the Llama-3 GQA grouping (32 q heads on 8 kv heads), 4 layers (Q4_K_M mix:
    # layers 0 and 3 bump V/down to Q6_K): full-width kernels at test cost
    "pd-llama-g4": ModelSpec("pd-llama-g4", 4096, 4, 32, 8, 2048, 0, 500000.0, "bpe", "q4_k_m",
                             n_ctx_train=1024),
    # d = 8192 (the 70B's width) in one layer: six rows no longer fit the one-part staging, so the
    # batched step takes the prep (bprep) FFN path beside the split-K Q|K|V
    "tiny-llama3-d8k": ModelSpec("tiny-llama3-d8k", 8192, 1, 64, 8, 512, 0, 500000.0, "bpe", "q4_k_m",
                                 n_ctx_train=1024),
    # Llama-3-70B's layer shape in 2 layers (small vocabulary): the TP = 8 rehearsal's per-rank
    # shapes are the 70B's own (1 KV head, 8 query heads, 3584 FFN features per rank)
    "llama3-70b-2l": ModelSpec("llama3-70b-2l", 8192, 2, 64, 8, 28672, 0, 500000.0, "bpe", "q4_k_m",
                               n_ctx_train=1024, size_class="70B"),
    # Mixtral's width (d = 4096, 8 experts, top-2) in one layer: the single-row decode routes
    # inside the gate/up GEMV at this width (csrc/kernels/gemv.hip, GemvArgs::route_w)
    "tiny-mixtral-d4k": ModelSpec("tiny-mixtral-d4k", 4096, 1, 32, 8, 512, 0, 1e6, "spm", "q4_k_m",
                                  n_expert=8, n_expert_used=2, n_ctx_train=1024),
    "tiny-llama3-f32": ModelSpec("tiny-llama3-f32", 128, 2, 2, 1, 256, 0, 500000.0, "bpe", "f32",
                                 n_ctx_train=512),
}

# Qwen2 / Qwen2.5: Q|K|V biases, NeoX RoPE, GQA groups that are no power of two (7, 6, 5), no BOS
def _qwen2(name, d, n_layer, n_head, n_kv, n_ff, quant, n_vocab=0, **kw):
    return ModelSpec(name, d, n_layer, n_head, n_kv, n_ff, n_vocab, 1e6, "bpe", quant, n_ctx_train=1024,
                     rms_eps=1e-6, arch="qwen2", qkv_bias=True, **kw)


SPECS.update({
    "tiny-qwen2-g7": _qwen2("tiny-qwen2-g7", 1792, 2, 14, 2, 512, "q4_k_m"),
    "tiny-qwen2-g6-hd64": _qwen2("tiny-qwen2-g6-hd64", 768, 2, 12, 2, 512, "q4_k_m", tied_output=True),
    "tiny-qwen2-g5": _qwen2("tiny-qwen2-g5", 1280, 2, 10, 2, 512, "mixed-test"),
    # the 0.5B geometry: K = 896 is no multiple of 256 (no K-quants, no tile16 copies)
    "tiny-qwen2-d896": _qwen2("tiny-qwen2-d896", 896, 2, 14, 2, 512, "q8_0"),
    # TP = 2 at G = 7: kv heads move in pairs (2 x 7 x 128 q columns = whole 256-wide superblocks),
    # so 4 kv heads is the smallest split shard.h accepts
    "tiny-qwen2-tp": _qwen2("tiny-qwen2-tp", 3584, 2, 28, 4, 512, "q4_k_m"),
    # Qwen2.5-7B-Instruct's shape (for measuring, not for tests)
    "qwen2.5-7b-q4_k_m": replace(_qwen2("Qwen2.5-7B", 3584, 28, 28, 4, 18944, "q4_k_m", n_vocab=152064),
                                 n_ctx_train=32768),
})

# Qwen3 (dense): no biases, QK-norm, a head width of its own (key_length), NeoX RoPE, the qwen2 tokenizer
def _qwen3(name, d, n_layer, n_head, n_kv, hd, n_ff, quant, n_vocab=0, **kw):
    return ModelSpec(name, d, n_layer, n_head, n_kv, n_ff, n_vocab, 1e6, "bpe", quant, n_ctx_train=1024,
                     rms_eps=1e-6, arch="qwen3", qk_norm=True, hd=hd, **kw)


SPECS.update({
    # n_q = 1024 != d = 768 (the 0.6B's kind of geometry), tied output
    "tiny-qwen3-g2-hd128": _qwen3("tiny-qwen3-g2-hd128", 768, 2, 8, 4, 128, 512, "q4_k_m", tied_output=True),
    "tiny-qwen3-g4-hd64": _qwen3("tiny-qwen3-g4-hd64", 512, 2, 8, 2, 64, 512, "q8_0"),
    # mixed types: the batched step takes the unfused path (bprep + bmm + head-norm kernel)
    "tiny-qwen3-g5": _qwen3("tiny-qwen3-g5", 1280, 2, 10, 2, 128, 512, "mixed-test"),
    "tiny-qwen3-g8": _qwen3("tiny-qwen3-g8", 2048, 2, 16, 2, 128, 512, "q4_k_m"),
    "tiny-qwen3-tp": _qwen3("tiny-qwen3-tp", 1536, 2, 16, 4, 128, 512, "q4_k_m"),
    # Qwen3-8B's shape (for measuring, not for tests)
    "qwen3-8b-q4_k_m": replace(_qwen3("Qwen3-8B", 4096, 36, 32, 8, 128, 12288, "q4_k_m", n_vocab=151936),
                               n_ctx_train=40960),
})

# the legacy 32-weight block formats (Q4_0 / Q4_1 / Q5_0 / Q5_1) over existing shapes
SPECS.update({
    "tiny-llama3-q4_0": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-llama3-q4_0", quant="q4_0"),
    "tiny-llama3-q5_1": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-llama3-q5_1", quant="q5_1"),
    "tiny-llama3-legacy-mixed": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-llama3-legacy-mixed",
                                        quant="legacy-mixed-test"),
    "tiny-legacy-mixed-1l": replace(SPECS["tiny-mixed-1l"], name="tiny-legacy-mixed-1l",
                                    quant="legacy-mixed-test"),
    # n_ff = 576: the down projection's K is not a multiple of 256 (no tile16 copy)
    "tiny-q5_0-oddff": replace(SPECS["tiny-q8-oddff"], name="tiny-q5_0-oddff", quant="q5_0"),
    "llama3-8b-q4_0": replace(SPECS["llama3-8b-q4_k_m"], name="Llama-3-8B-Q4_0", quant="q4_0"),
})


# the 2- and 3-bit K-quants (Q2_K / Q3_K) over existing shapes
SPECS.update({
    "tiny-llama3-q2_k": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-llama3-q2_k", quant="q2_k"),
    "tiny-llama3-q3_k_s": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-llama3-q3_k_s", quant="q3_k_s"),
    "tiny-llama3-q3_k_m": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-llama3-q3_k_m", quant="q3_k_m"),
    # one layer holding Q2_K, Q3_K, Q4_K and Q6_K
    "tiny-kmixed-1l": replace(SPECS["tiny-mixed-1l"], name="tiny-kmixed-1l", quant="kmixed-test"),
    # Q|K|V biases and the NeoX row permutation on a Q3_K attn_q; the tied head is a Q3_K GEMV
    "tiny-qwen2-q3_k_m": replace(SPECS["tiny-qwen2-g6-hd64"], name="tiny-qwen2-q3_k_m", quant="q3_k_m"),
    "llama3-8b-q3_k_m": replace(SPECS["llama3-8b-q4_k_m"], name="Llama-3-8B-Q3_K_M", quant="q3_k_m"),
    "llama3-8b-q2_k": replace(SPECS["llama3-8b-q4_k_m"], name="Llama-3-8B-Q2_K", quant="q2_k"),
})


# the non-linear 4-bit pair (IQ4_NL / IQ4_XS) over existing shapes
SPECS.update({
    "tiny-llama3-iq4_xs": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-llama3-iq4_xs", quant="iq4_xs"),
    "tiny-llama3-iq4_nl": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-llama3-iq4_nl", quant="iq4_nl"),
    # Q|K|V biases and the NeoX row permutation on IQ4_XS attn_q / attn_k; the tied head is an IQ4_XS GEMV
    "tiny-qwen2-iq4_xs": replace(SPECS["tiny-qwen2-g6-hd64"], name="tiny-qwen2-iq4_xs", quant="iq4_xs"),
    # IQ4_NL, IQ4_XS, Q4_K and Q6_K in one model, and in one layer
    "tiny-iq4-mixed": replace(SPECS["tiny-llama3-q4_k_m"], name="tiny-iq4-mixed", quant="iq4-mixed-test"),
    "tiny-iq4-mixed-1l": replace(SPECS["tiny-mixed-1l"], name="tiny-iq4-mixed-1l", quant="iq4-mixed-test"),
    # n_ff = 576: a multiple of 32 but not of 256 (IQ4_NL's block, not IQ4_XS's; no tile16 copy of down)
    "tiny-iq4_nl-oddff": replace(SPECS["tiny-q8-oddff"], name="tiny-iq4_nl-oddff", quant="iq4_nl"),
    "llama3-8b-iq4_xs": replace(SPECS["llama3-8b-q4_k_m"], name="Llama-3-8B-IQ4_XS", quant="iq4_xs"),
})


def use_more_bits(i: int, n: int) -> bool:
    return i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2


def tensor_types(spec: ModelSpec, layer: int) -> Dict[str, GGMLType]:
    """Per-layer ggml types of the 2-D weights for the spec's quant mix.

    The 2- and 3-bit K-quant files follow llama.cpp's llama_tensor_get_type for dense models
    (token_embd has the base type and output.weight is Q6_K, see ``tensor_plan``):

      q3_k_s: every matrix Q3_K.
      q3_k_m: base Q3_K; attn_v Q5_K in the first two layers, Q4_K after; attn_output Q4_K;
              ffn_down Q5_K in the first n_layer/16 layers, Q4_K after.
      q2_k:   base Q2_K; attn_v Q4_K when the GQA group is >= 4, else Q3_K; attn_output Q3_K;
              ffn_down Q3_K.
    8-expert models keep attn_k / attn_v at Q8_0 as in the Q4_K_M rule.

    The non-linear 4-bit files model the upstream rule for dense models (written from memory, with
    no copy to check against; the mix is not load-relevant - any mix of supported types loads):

      iq4_nl / iq4_xs: the base type everywhere; attn_v Q5_K when the GQA group is >= 4; ffn_down
                       Q5_K in the first n_layer/8 layers; token_embd the base type; output.weight
                       Q6_K."""
    q = spec.quant
    if q in IQ4_QUANTS:
        base = IQ4_QUANTS[q][0]
        out = {k: base for k in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")}
        if spec.n_head // spec.n_head_kv >= 4:
            out["attn_v"] = GGMLType.Q5_K
        if layer < spec.n_layer // 8:
            out["ffn_down"] = GGMLType.Q5_K
        return out
    if q == "iq4-mixed-test":  # IQ4_NL and IQ4_XS beside Q4_K and Q6_K in one model
        cyc = [GGMLType.IQ4_NL, GGMLType.IQ4_XS, GGMLType.Q4_K, GGMLType.Q6_K]
        names = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down")
        out = {k: cyc[(layer + j) % 4] for j, k in enumerate(names)}
        out["ffn_up"] = out["ffn_gate"]
        return out
    if q in K23_QUANTS:
        base = K23_QUANTS[q][0]
        out = {k: base for k in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")}
        if q == "q3_k_m":
            out["attn_v"] = GGMLType.Q5_K if layer < 2 else GGMLType.Q4_K
            out["attn_output"] = GGMLType.Q4_K
            out["ffn_down"] = GGMLType.Q5_K if layer < spec.n_layer // 16 else GGMLType.Q4_K
        elif q == "q2_k":
            out["attn_v"] = GGMLType.Q4_K if spec.n_head // spec.n_head_kv >= 4 else GGMLType.Q3_K
            out["attn_output"] = GGMLType.Q3_K
            out["ffn_down"] = GGMLType.Q3_K
        if spec.n_expert == 8:
            out["attn_k"] = GGMLType.Q8_0
            out["attn_v"] = GGMLType.Q8_0
        return out
    if q == "kmixed-test":  # Q2_K and Q3_K beside Q4_K and Q6_K in one model
        cyc = [GGMLType.Q2_K, GGMLType.Q3_K, GGMLType.Q4_K, GGMLType.Q6_K]
        names = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down")
        out = {k: cyc[(layer + j) % 4] for j, k in enumerate(names)}
        out["ffn_up"] = out["ffn_gate"]
        return out
    if q == "q8_0":
        t = GGMLType.Q8_0
        return {k: t for k in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")}
    if q == "f32":
        t = GGMLType.F32
        return {k: t for k in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")}
    if q in LEGACY_QUANTS:
        t = LEGACY_QUANTS[q][0]
        return {k: t for k in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")}
    if q == "legacy-mixed-test":  # the four legacy formats and Q8_0 in one model
        cyc = [GGMLType.Q4_0, GGMLType.Q4_1, GGMLType.Q5_0, GGMLType.Q5_1, GGMLType.Q8_0]
        names = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down")
        out = {k: cyc[(layer + j) % 5] for j, k in enumerate(names)}
        out["ffn_up"] = out["ffn_gate"]  # gate/up are one interleaved matrix on the GPU
        return out
    if q == "mixed-test":  # every quant format in one model, to test all kernels end to end
        cyc = [GGMLType.Q4_K, GGMLType.Q5_K, GGMLType.Q6_K, GGMLType.Q8_0]
        names = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_down")
        out = {k: cyc[(layer + j) % 4] for j, k in enumerate(names)}
        out["ffn_up"] = out["ffn_gate"]  # gate/up are one interleaved matrix on the GPU
        return out
    assert q == "q4_k_m"
    n = spec.n_layer
    bump = use_more_bits(layer, n)
    out = {k: GGMLType.Q4_K for k in ("attn_q", "attn_k", "attn_output", "ffn_gate", "ffn_up")}
    if spec.n_expert == 8:
        out["attn_k"] = GGMLType.Q8_0
        out["attn_v"] = GGMLType.Q8_0
    elif bump:
        out["attn_v"] = GGMLType.Q6_K
    else:
        out["attn_v"] = GGMLType.Q5_K if spec.size_class == "70B" else GGMLType.Q4_K
    out["ffn_down"] = GGMLType.Q6_K if bump else GGMLType.Q4_K
    return out


def _load_json(name):
    with open(os.path.join(ASSETS, name), encoding="utf-8") as f:
        return json.load(f)


def build_vocab(spec: ModelSpec) -> Tuple[Dict, int]:
    """Tokenizer metadata + final vocab size."""
    if spec.tokenizer == "bpe":
        v = _load_json("bpe_vocab.json")
        tokens = list(v["tokens"])
        n_regular = (spec.n_vocab - 256) if spec.n_vocab else len(tokens)
        existing = set(tokens)
        i = 0
        while len(tokens) < n_regular:
            cand = f"Ġfill{i}q"
            i += 1
            if cand not in existing:
                tokens.append(cand)
        base = len(tokens)
        types = [TOKEN_TYPE_NORMAL] * base
        qwen2 = spec.arch in ("qwen2", "qwen3")
        for k in range(256):
            name = (QWEN2_SPECIALS if qwen2 else LLAMA3_SPECIALS).get(k, f"<|reserved_special_token_{k}|>")
            tokens.append(name)
            types.append(TOKEN_TYPE_CONTROL)
        if qwen2:  # no BOS, eos = <|im_end|>, ChatML
            md = {"tokenizer.ggml.model": "gpt2", "tokenizer.ggml.pre": "qwen2",
                  "tokenizer.ggml.tokens": tokens, "tokenizer.ggml.token_type": types,
                  "tokenizer.ggml.merges": v["merges"],
                  "tokenizer.ggml.bos_token_id": base + 0, "tokenizer.ggml.eos_token_id": base + 2,
                  "tokenizer.ggml.padding_token_id": base + 0, "tokenizer.ggml.add_bos_token": False,
                  "tokenizer.chat_template": spec.chat_template or CHATML_CHAT_TEMPLATE}
            return md, len(tokens)
        md = {"tokenizer.ggml.model": "gpt2", "tokenizer.ggml.pre": "llama-bpe",
              "tokenizer.ggml.tokens": tokens, "tokenizer.ggml.token_type": types,
              "tokenizer.ggml.merges": v["merges"],
              "tokenizer.ggml.bos_token_id": base + 0, "tokenizer.ggml.eos_token_id": base + 9,
              "tokenizer.chat_template": spec.chat_template or LLAMA3_CHAT_TEMPLATE}
        return md, len(tokens)
    v = _load_json("spm_vocab.json")
    pieces, scores, types = list(v["pieces"]), list(v["scores"]), list(v["types"])
    target = spec.n_vocab or len(pieces)
    existing = set(pieces)
    i = 0
    while len(pieces) < target:
        cand = f"▁fill{i}q"
        i += 1
        if cand not in existing:
            pieces.append(cand)
            scores.append(-1e4 - i)
            types.append(TOKEN_TYPE_NORMAL)
    tmpl = spec.chat_template or (MISTRAL_CHAT_TEMPLATE if spec.n_expert else ZEPHYR_CHAT_TEMPLATE)
    md = {"tokenizer.ggml.model": "llama", "tokenizer.ggml.tokens": pieces,
          "tokenizer.ggml.scores": scores, "tokenizer.ggml.token_type": types,
          "tokenizer.ggml.bos_token_id": 1, "tokenizer.ggml.eos_token_id": 2,
          "tokenizer.ggml.unknown_token_id": 0, "tokenizer.ggml.add_bos_token": True,
          "tokenizer.ggml.add_space_prefix": True, "tokenizer.chat_template": tmpl}
    return md, len(pieces)


def tensor_plan(spec: ModelSpec, n_vocab: int) -> List[Tuple[str, GGMLType, Tuple[int, ...]]]:
    d, f, L = spec.n_embd, spec.n_ff, spec.n_layer
    dkv, nq = spec.head_dim * spec.n_head_kv, spec.n_q
    if spec.quant == "q8_0":
        emb_t, out_t = GGMLType.Q8_0, GGMLType.Q8_0
    elif spec.quant == "f32":
        emb_t, out_t = GGMLType.F32, GGMLType.F32
    elif spec.quant in LEGACY_QUANTS:
        emb_t, out_t = LEGACY_QUANTS[spec.quant][0], GGMLType.Q6_K
    elif spec.quant == "legacy-mixed-test":
        emb_t, out_t = GGMLType.Q5_0, GGMLType.Q6_K
    elif spec.quant in K23_QUANTS:
        emb_t, out_t = K23_QUANTS[spec.quant][0], GGMLType.Q6_K
    elif spec.quant == "kmixed-test":
        emb_t, out_t = GGMLType.Q2_K, GGMLType.Q6_K
    elif spec.quant in IQ4_QUANTS:
        emb_t, out_t = IQ4_QUANTS[spec.quant][0], GGMLType.Q6_K
    elif spec.quant == "iq4-mixed-test":
        emb_t, out_t = GGMLType.IQ4_XS, GGMLType.Q6_K
    else:
        emb_t, out_t = GGMLType.Q4_K, GGMLType.Q6_K
    plan = [("token_embd.weight", emb_t, (d, n_vocab))]
    for i in range(L):
        tt = tensor_types(spec, i)
        p = f"blk.{i}."
        plan += [(p + "attn_norm.weight", GGMLType.F32, (d,)),
                 (p + "attn_q.weight", tt["attn_q"], (d, nq)),
                 (p + "attn_k.weight", tt["attn_k"], (d, dkv)),
                 (p + "attn_v.weight", tt["attn_v"], (d, dkv)),
                 (p + "attn_output.weight", tt["attn_output"], (nq, d)),
                 (p + "ffn_norm.weight", GGMLType.F32, (d,))]
        if spec.qkv_bias:
            plan += [(p + "attn_q.bias", GGMLType.F32, (nq,)), (p + "attn_k.bias", GGMLType.F32, (dkv,)),
                     (p + "attn_v.bias", GGMLType.F32, (dkv,))]
        if spec.qk_norm:
            plan += [(p + TENSOR_ATTN_Q_NORM, GGMLType.F32, (spec.head_dim,)),
                     (p + TENSOR_ATTN_K_NORM, GGMLType.F32, (spec.head_dim,))]
        if spec.n_expert:
            E = spec.n_expert
            plan += [(p + "ffn_gate_inp.weight", GGMLType.F32, (d, E)),
                     (p + "ffn_gate_exps.weight", tt["ffn_gate"], (d, f, E)),
                     (p + "ffn_down_exps.weight", tt["ffn_down"], (f, d, E)),
                     (p + "ffn_up_exps.weight", tt["ffn_up"], (d, f, E))]
        else:
            plan += [(p + "ffn_gate.weight", tt["ffn_gate"], (d, f)),
                     (p + "ffn_down.weight", tt["ffn_down"], (f, d)),
                     (p + "ffn_up.weight", tt["ffn_up"], (d, f))]
    plan += [("output_norm.weight", GGMLType.F32, (d,))]
    if not spec.tied_output:
        plan += [("output.weight", out_t, (d, n_vocab))]
    return plan


def hparams_metadata(spec: ModelSpec, n_vocab: int) -> Dict:
    a = spec.arch
    if spec.quant in LEGACY_QUANTS:
        ftype = LEGACY_QUANTS[spec.quant][1]
    elif spec.quant in K23_QUANTS:
        ftype = K23_QUANTS[spec.quant][1]
    elif spec.quant in IQ4_QUANTS:
        ftype = IQ4_QUANTS[spec.quant][1]
    else:
        ftype = FTYPE_MOSTLY_Q8_0 if spec.quant == "q8_0" else FTYPE_MOSTLY_Q4_K_M
    md = {"general.architecture": a, "general.name": spec.name + " (synthetic random-init)",
          "general.file_type": ftype,
          f"{a}.context_length": spec.n_ctx_train, f"{a}.embedding_length": spec.n_embd,
          f"{a}.block_count": spec.n_layer, f"{a}.feed_forward_length": spec.n_ff,
          f"{a}.rope.dimension_count": spec.head_dim, f"{a}.attention.head_count": spec.n_head,
          f"{a}.attention.head_count_kv": spec.n_head_kv,
          f"{a}.attention.layer_norm_rms_epsilon": float(spec.rms_eps),
          f"{a}.rope.freq_base": float(spec.rope_base), f"{a}.vocab_size": n_vocab}
    if spec.n_expert:
        md[f"{a}.expert_count"] = spec.n_expert
        md[f"{a}.expert_used_count"] = spec.n_expert_used
    if a == "qwen2":  # (Qwen2 files carry no rope.dimension_count: head_dim = n_embd / n_head)
        del md[f"{a}.rope.dimension_count"]
    if a == ARCH_QWEN3:  # the head width is a key of its own, for keys and for values
        del md[f"{a}.rope.dimension_count"]
        md[f"{a}.{KEY_ATTN_KEY_LENGTH}"] = spec.head_dim
        md[f"{a}.{KEY_ATTN_VALUE_LENGTH}"] = spec.head_dim
    return md


def qkv_bias_std(spec: ModelSpec) -> float:
    return 4.0 * spec.weight_std * float(np.sqrt(spec.n_embd))


def write_synthetic_gguf(spec, path: str, seed: int = 0, log=None, extra_metadata: Optional[Dict] = None,
                         skip_tensors: Tuple[str, ...] = (), untie_output: bool = False) -> str:
    """Stream a random-init GGUF for ``spec`` (a ModelSpec or a SPECS key) to ``path``.

    For loader tests: ``extra_metadata`` adds keys, ``skip_tensors`` leaves tensors out (the other
    tensors keep the values they have in the full file), and ``untie_output`` writes a
    ``tied_output`` spec's head as an explicit ``output.weight`` holding token_embd's own blocks."""
    if isinstance(spec, str):
        spec = SPECS[spec]
    rng = np.random.default_rng(seed)
    vocab_md, n_vocab = build_vocab(spec)
    tmp = path + ".tmp"
    w = GGUFWriter(tmp)
    for k, v in hparams_metadata(spec, n_vocab).items():
        w.add(k, v)
    for k, v in vocab_md.items():
        if k == "tokenizer.ggml.scores":
            w.add(k, v, GGUFValueType.ARRAY, GGUFValueType.FLOAT32)
        elif k == "tokenizer.ggml.token_type":
            w.add(k, v, GGUFValueType.ARRAY, GGUFValueType.INT32)
        elif k.endswith("_token_id"):
            w.add(k, int(v), GGUFValueType.UINT32)
        else:
            w.add(k, v)
    for k, v in (extra_metadata or {}).items():
        w.add(k, v)
    plan = tensor_plan(spec, n_vocab)
    if untie_output and spec.tied_output:
        plan.append(("output.weight", plan[0][1], plan[0][2]))
    for name, t, shape in plan:
        if name not in skip_tensors:
            w.declare_tensor(name, t, shape)
    w.begin()
    embd = None
    for name, t, shape in plan:
        n = int(np.prod(shape))
        if name == "output.weight" and untie_output and spec.tied_output:
            w.write_tensor_data(embd)
            continue
        if name.endswith((TENSOR_ATTN_Q_NORM, TENSOR_ATTN_K_NORM)):
            # far from ones, so that a dropped or unpermuted QK-norm weight shows
            data = (1.0 + 0.5 * rng.standard_normal(n)).astype(np.float32)
        elif name.endswith("norm.weight"):
            data = (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)
        elif name.endswith(".bias"):
            # four times the standard deviation of the projection's own output on a normed input
            # (weight_std * sqrt(d)): real Qwen2 biases are large, and a dropped one must show
            data = (qkv_bias_std(spec) * rng.standard_normal(n)).astype(np.float32)
        else:
            std = spec.weight_std
            if name == "token_embd.weight":
                std = 1.0  # keeps the first RMSNorm well conditioned
            data = random_blocks(t, n, rng, std=std)
        if name == "token_embd.weight" and untie_output:
            embd = data
        if name in skip_tensors:
            continue
        w.write_tensor_data(data)
        if log:
            log(name)
    w.close()
    os.replace(tmp, path)
    return path


def cached_synthetic_gguf(name: str, cache_dir: Optional[str] = None, seed: int = 0) -> str:
    """Path of a synthetic model, generated once per cache dir."""
    cache_dir = cache_dir or os.environ.get("SYNTH_MODEL_DIR") or os.path.join(
        os.environ.get("TMPDIR", "/tmp"), "llama_amd_models")
    os.makedirs(cache_dir, exist_ok=True)
    path = os.path.join(cache_dir, f"{name}-s{seed}.gguf")
    if not os.path.exists(path):
        write_synthetic_gguf(name, path, seed)
    return path
