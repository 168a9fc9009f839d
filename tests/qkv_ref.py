"""fp64 reference and checker of the batched decode step's Q|K|V stage: projection (+ bias), RoPE
on adjacent pairs, Q rows out, K / V rows as f16 into the slot caches at each row's position.
Needs no GPU, so the checker has a CPU self-test (test_qkv_ref.py)."""
import numpy as np

from gpu_helpers import rel_err

# the project's bound on one projection row against fp64 (test_bmm_qkv_splitk_then_attention)
NORM_BOUND = 3e-3
# per element, as a fraction of the rms of the row's segment: an error of NORM_BOUND * rms per
# element (rms) puts 0.05 * rms more than 16 standard deviations out, while a misplaced, un-rotated
# or un-biased element is off by the order of rms itself
ELEM_BOUND = 0.05
F16_HALF_ULP = 2.0 ** -11


def _rope_table(n_ctx, hd, theta=5e5):
    inv = theta ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    ang = np.arange(n_ctx, dtype=np.float64)[:, None] * inv[None, :]
    return np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)   # [n_ctx][hd/2][2]


def _rope_pairs(y, pos, tab):
    """RoPE on adjacent pairs (GGUF normal mode) of y [rows] at position pos, rows % hd per head."""
    hd2 = tab.shape[1]
    z = y.reshape(-1, hd2, 2).astype(np.float64)
    c, s = tab[pos, :, 0].astype(np.float64), tab[pos, :, 1].astype(np.float64)
    return np.stack([z[..., 0] * c - z[..., 1] * s, z[..., 0] * s + z[..., 1] * c], -1).reshape(y.shape)


def staged_x(X, norm_w, eps, staging):
    """The activation rows as the kernels stage them, in fp64.
    "xh": X is the f16 input itself. "folded": f16(x * norm_w) times the row's rsqrt(mean(x^2) + eps)
    (the one-part staging with the norm folded in). "bprep": f16(rmsnorm(x) * norm_w)."""
    X64 = np.asarray(X, np.float64)
    if staging == "xh":
        return np.asarray(X, np.float16).astype(np.float64)
    rs = 1.0 / np.sqrt((X64 ** 2).mean(1, keepdims=True) + eps)
    if staging == "folded":
        return (np.asarray(X, np.float32) * np.asarray(norm_w, np.float32)).astype(np.float16).astype(np.float64) * rs
    if staging == "bprep":
        return (X64 * rs * np.asarray(norm_w, np.float64)).astype(np.float16).astype(np.float64)
    raise ValueError(staging)


class QkvRef:
    """q [B][nq]; k, v [B][Hkv][hd] (the row each b writes); pos (clamped) and slots [B]; raw [B][ncol]:
    the projections before bias and rotation."""

    def __init__(self, q, k, v, pos, slots, raw, n_ctx, hd):
        self.q, self.k, self.v, self.pos, self.slots, self.raw, self.n_ctx, self.hd = q, k, v, pos, slots, raw, n_ctx, hd


def qkv_reference(X, norm_w, eps, Ws, bias, pos, slots, tab, n_ctx, hd, staging="xh"):
    """Ws: the three dequantised matrices (Q [nq][K], K and V [nkv][K]); bias: None or one vector
    [nq + 2 nkv] added before the rotation; pos: clamped to [0, n_ctx) as the kernels do."""
    x = staged_x(X, norm_w, eps, staging)
    B = x.shape[0]
    nq, nkv = Ws[0].shape[0], Ws[1].shape[0]
    raw = np.concatenate([x @ np.asarray(W, np.float64).T for W in Ws], axis=1)
    y = raw + (np.asarray(bias, np.float64)[None, :] if bias is not None else 0.0)
    pc = np.clip(np.asarray(pos, np.int64), 0, n_ctx - 1)
    q = np.stack([_rope_pairs(y[b, :nq], pc[b], tab) for b in range(B)])
    k = np.stack([_rope_pairs(y[b, nq:nq + nkv], pc[b], tab) for b in range(B)]).reshape(B, nkv // hd, hd)
    v = y[:, nq + nkv:].reshape(B, nkv // hd, hd).copy()
    return QkvRef(q, k, v, pc, np.asarray(slots, np.int64), raw, n_ctx, hd)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def check_qkv(got_q, got_K, got_V, ref, sentinelK, sentinelV, sentinel_q=None, slot0=0):
    """got_q [>= B rows][>= nq columns] f32; got_K / got_V [slots][Hkv][n_ctx][hd] f16, the whole
    allocation (slot0 = index of the slot the kernels saw as slot 0); sentinel*: what the buffers
    held before the launch. Raises AssertionError; returns the largest norm and per-element errors
    as fractions of their bounds."""
    B, nq = ref.q.shape
    got_q = np.asarray(got_q)
    worst = {"norm": 0.0, "elem": 0.0}

    def segment(name, b, got, want, f16):
        got, want = np.asarray(got, np.float64).ravel(), want.ravel()
        assert np.all(np.isfinite(got)), (name, b, "non-finite")
        e = rel_err(got, want)
        worst["norm"] = max(worst["norm"], e / NORM_BOUND)
        assert e < NORM_BOUND, (name, b, "norm", e)
        rms = np.sqrt(np.mean(want ** 2))
        bound = ELEM_BOUND * rms + (F16_HALF_ULP * np.abs(want) if f16 else 0.0)
        frac = np.abs(got - want) / bound
        i = int(np.argmax(frac))
        worst["elem"] = max(worst["elem"], float(frac[i]))
        assert frac[i] <= 1.0, (name, b, "element", i, got[i], want[i], float(frac[i]))

    written = np.zeros(got_K.shape, bool)
    for b in range(B):
        s, p = slot0 + int(ref.slots[b]), int(ref.pos[b])
        segment("q", b, got_q[b, :nq], ref.q[b], False)
        segment("k", b, got_K[s, :, p], ref.k[b], True)
        segment("v", b, got_V[s, :, p], ref.v[b], True)
        written[s, :, p] = True
    for name, got, sent in (("K", got_K, sentinelK), ("V", got_V, sentinelV)):
        bad = (_bits(got) != _bits(sent)) & ~written
        assert not bad.any(), (name, "cache written outside the rows' (slot, head, pos)",
                               [tuple(int(x) for x in i) for i in np.argwhere(bad)[:4]])
    if sentinel_q is not None:
        outside = np.ones(got_q.shape, bool)
        outside[:B, :nq] = False
        bad = (_bits(got_q) != _bits(sentinel_q)) & outside
        assert not bad.any(), ("q_out written outside [B][nq]", [tuple(int(x) for x in i) for i in np.argwhere(bad)[:4]])
    return worst
