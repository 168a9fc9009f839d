"""Pooling of text embeddings (llama.cpp's ``llama_pooling_type`` values) on the host.

The MI355X engine pools on the device (csrc/kernels/misc.hip ``pool_rows`` / ``pool_finish``);
the CPU and reference backends hand their normed final rows to :func:`pool_host`.
"""
from __future__ import annotations

import numpy as np

POOLING_UNSPECIFIED = -1
POOLING_NONE = 0
POOLING_MEAN = 1
POOLING_CLS = 2
POOLING_LAST = 3
POOLING_RANK = 4
POOLING_NAMES = {"none": POOLING_NONE, "mean": POOLING_MEAN, "cls": POOLING_CLS, "last": POOLING_LAST}


def check_pooling(pooling: int) -> int:
    """``pooling`` as one of none / mean / cls / last; anything else (``rank`` = 4 included) is refused."""
    pooling = int(pooling)
    if pooling == POOLING_RANK:
        raise NotImplementedError("pooling_type 4 (rank) is not supported: this engine serves no reranking")
    if pooling not in (POOLING_NONE, POOLING_MEAN, POOLING_CLS, POOLING_LAST):
        raise NotImplementedError(f"pooling_type {pooling} is not supported (0 none, 1 mean, 2 cls, 3 last)")
    return pooling


def resolve_pooling(requested: int, model_pooling: int) -> int:
    """-1 resolves to the model's ``{arch}.pooling_type`` and, where the key is absent, to none."""
    requested = int(requested)
    if requested != POOLING_UNSPECIFIED:
        return requested
    return int(model_pooling) if int(model_pooling) >= 0 else POOLING_NONE


def rms_norm_rows(x: np.ndarray, w: np.ndarray, eps: float, dtype=np.float32) -> np.ndarray:
    """The model's output RMSNorm over rows ``x`` [T, d]."""
    x = np.asarray(x, dtype)
    scale = 1.0 / np.sqrt((x * x).mean(-1, keepdims=True, dtype=dtype) + dtype(eps))
    return (x * scale * np.asarray(w, dtype)).astype(dtype)


def pool_host(rows: np.ndarray, pooling: int, normalize: bool, dtype=np.float32) -> np.ndarray:
    """Pool the normed rows [T, d] of one input: [d], or for none the rows [T, d] themselves;
    ``normalize`` divides each returned vector by its L2 norm (a zero vector stays zero, as
    upstream). Returned as float32."""
    rows = np.asarray(rows, dtype)
    if pooling == POOLING_MEAN:
        v = rows.mean(0, dtype=dtype)
    elif pooling == POOLING_CLS:
        v = rows[0]
    elif pooling == POOLING_LAST:
        v = rows[-1]
    elif pooling == POOLING_NONE:
        v = rows
    else:
        check_pooling(pooling)
        raise AssertionError
    if normalize:
        norm = np.sqrt((v * v).sum(-1, keepdims=True, dtype=dtype))
        v = v * np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1), 0).astype(dtype)   # a zero vector stays zero
    return np.ascontiguousarray(v, np.float32)
