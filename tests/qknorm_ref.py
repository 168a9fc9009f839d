"""fp64 reference of the Q|K|V stage of a QK-norm model (qwen3): qkv_ref.qkv_reference with an RMSNorm
over each q and k head between the raw projection and the rotation. The weights are in the kernels'
(pair-permuted) row order, so the rotation stays qkv_ref's adjacent-pair one. check_qkv is qkv_ref's
own, unchanged. Needs no GPU (test_qknorm_ref.py plants defects and shows the checker rejects each)."""
import numpy as np

from qkv_ref import QkvRef, _rope_pairs, qkv_reference


def neox_perm(hd):
    """Index map of the loaders' permutation: new entry 2i = file entry i, 2i + 1 = i + hd/2."""
    j = np.arange(hd)
    return (j >> 1) + np.where(j & 1, hd // 2, 0)


def head_norm(y, w, eps, hd):
    """y [..., n] of whole heads of hd values: y_i * rsqrt(mean_head(y^2) + eps) * w_(i % hd), fp64."""
    y = np.asarray(y, np.float64)
    h = y.reshape(y.shape[:-1] + (-1, hd))
    h = h / np.sqrt((h ** 2).mean(-1, keepdims=True) + eps) * np.asarray(w, np.float64)
    return h.reshape(y.shape)


def qknorm_reference(X, norm_w, eps, Ws, qk_norm, qkn_eps, pos, slots, tab, n_ctx, hd, staging="xh", raw=None):
    """qk_norm: [q_norm | k_norm], 2 hd values in the kernels' order; qkn_eps: the head norm's eps (a
    launch argument at every site). ``raw`` [B][nq + 2 nkv]: projection sums to use in place of the
    staged product (the kernels that start from given rows)."""
    base = qkv_reference(X, norm_w, eps, Ws, None, pos, slots, tab, n_ctx, hd, staging)
    y = base.raw if raw is None else np.asarray(raw, np.float64)
    B = y.shape[0]
    nq, nkv = Ws[0].shape[0], Ws[1].shape[0]
    wq, wk = np.asarray(qk_norm, np.float64)[:hd], np.asarray(qk_norm, np.float64)[hd:2 * hd]
    qn, kn = head_norm(y[:, :nq], wq, qkn_eps, hd), head_norm(y[:, nq:nq + nkv], wk, qkn_eps, hd)
    q = np.stack([_rope_pairs(qn[b], base.pos[b], tab) for b in range(B)])
    k = np.stack([_rope_pairs(kn[b], base.pos[b], tab) for b in range(B)]).reshape(B, nkv // hd, hd)
    v = y[:, nq + nkv:].reshape(B, nkv // hd, hd).copy()
    return QkvRef(q, k, v, base.pos, base.slots, y, n_ctx, hd)


def qknorm_from_rows(rows, nq, nkv, qk_norm, qkn_eps, pos, slots, tab, n_ctx, hd):
    """The reference of a kernel that starts from given projection rows [B][nq + 2 nkv]."""
    rows = np.asarray(rows, np.float64)
    Ws = [np.zeros((n, 1)) for n in (nq, nkv, nkv)]
    return qknorm_reference(np.zeros((rows.shape[0], 1)), None, 0.0, Ws, qk_norm, qkn_eps, pos, slots, tab, n_ctx, hd,
                            raw=rows)


# the split-K test's cases (hd, G, big_eps) and inputs, shared by the GPU test and by the CPU test that
# computes, before any GPU run, what the f16 staging of these very inputs costs against fp64
SK_CASES = [(128, 2, False), (128, 5, False), (64, 4, False), (128, 5, True), (64, 4, True)]
SK_B, SK_HKV, SK_K, SK_NCTX = 3, 2, 512, 128


def splitk_inputs(hd, G, big_eps, t):
    """Three Q4_K-style matrices of standard-normal weights (ggml type t: raw blocks and dequantised),
    standard-normal rows times (0.5, 1, 2) - the rows' 1/rms differ from 1, the projections' sizes do
    not -, the attention norm weight, [q_norm | k_norm] in kernel order, positions L = 1, 65, n_ctx."""
    from gpu_helpers import make_matrix
    rng = np.random.default_rng(hd + G + 100 * big_eps)
    nq, nkv = G * SK_HKV * hd, SK_HKV * hd
    mats = [make_matrix(t, R, SK_K, rng, std=1.0) for R in (nq, nkv, nkv)]
    X = (rng.standard_normal((SK_B, SK_K)) * np.array([0.5, 1.0, 2.0])[:, None]).astype(np.float32)
    nw = (1.0 + 0.1 * rng.standard_normal(SK_K)).astype(np.float32)
    w = (1.0 + 0.5 * rng.standard_normal(2 * hd)).astype(np.float32)
    return dict(rng=rng, mats=mats, X=X, nw=nw, w=w, eps=1e-6,
                qkn_eps=0.5 * SK_K if big_eps else 1e-6,   # a head's mean square is ~K (unit-variance inputs and weights)
                pos=np.array([0, 64, SK_NCTX - 1], np.int32), slots=np.array([3, 0, 2], np.int32), nq=nq, nkv=nkv)


def f16_staged_error(ref):
    """Largest segment error (norm-relative) of the reference's own k / v rows after the f16 cache
    rounding - what the storage format alone costs, as a fraction of nothing (compare with a bound)."""
    worst = 0.0
    for a in (ref.k, ref.v):
        r = a.astype(np.float16).astype(np.float64)
        for b in range(a.shape[0]):
            worst = max(worst, float(np.linalg.norm(r[b] - a[b]) / np.linalg.norm(a[b])))
    return worst
