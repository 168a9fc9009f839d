"""Q8_0 KV cache kernels (csrc/kernels/attention_q8.hip) against fp64, through the existing bindings with
kv_type="q8_0". Append: per stored block, d within one f16 ulp of amax / 127 and |d q - x| <= d / 2 +
2^-11 |x| (one Q8_0 step plus the f32 rotation), q_out within qkv_ref.NORM_BOUND. Readers: caches the test
quantises itself, fp64 attention over the dequantised cache and the f32 q, ATTN_BOUND = 5e-3 of the row's
norm (the project's figure). Each test prints worst / bound (profiles/kv_q8_test_figures.txt)."""
import numpy as np
import pytest

from gpu_helpers import hip, stream
from qkv_ref import NORM_BOUND, _rope_table

pytestmark = pytest.mark.gpu
ATTN_BOUND = 5e-3
GUARD = 1   # guard slots in front of and behind the slots the kernels see
Q8 = {"kv_type": "q8_0"}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def q8_quant(x):
    """x [..., hd] -> (q int8 [..., hd], d f16 [..., hd / 32]): GGML's Q8_0 along the last axis."""
    b = np.asarray(x, np.float64).reshape(*x.shape[:-1], -1, 32)
    d = (np.abs(b).max(-1) / 127).astype(np.float16)
    df = d.astype(np.float64)[..., None]
    q = np.where(df > 0, np.rint(b / np.where(df > 0, df, 1)), 0).clip(-127, 127).astype(np.int8)
    return q.reshape(x.shape), d


def q8_pack(q, d):   # [S][Hkv][n_ctx][hd] int8 + [S][Hkv][n_ctx][hd / 32] f16 -> uint8 [S][slot bytes]
    return np.concatenate([q.reshape(len(q), -1).view(np.uint8), d.reshape(len(q), -1).view(np.uint8)], 1)


def q8_unpack(buf, Hkv, n_ctx, hd):
    n = Hkv * n_ctx * hd
    return (np.ascontiguousarray(buf[:, :n]).view(np.int8).reshape(-1, Hkv, n_ctx, hd),
            np.ascontiguousarray(buf[:, n:]).view(np.float16).reshape(-1, Hkv, n_ctx, hd // 32))


def deq(q, d):
    return (q.astype(np.float64).reshape(*d.shape, 32) * d.astype(np.float64)[..., None]).reshape(q.shape)


def attention(q, K, V, n_keys, scale):
    """q [G][hd] f32 of one kv head, K / V [n_ctx][hd] fp64 -> [G][hd] fp64 (max-subtracted softmax)."""
    s = (q.astype(np.float64) @ K[:n_keys].T) * scale
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)) @ V[:n_keys], np.abs(s).max()


def row_err(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


def worst_rows(got, q, K, V, n_keys, G, scale):
    """got / q [H][hd] of one token, K / V [Hkv][n_ctx][hd] fp64 -> (worst row error, largest |logit|)."""
    res = [attention(q[h * G:(h + 1) * G], K[h], V[h], n_keys, scale) for h in range(len(K))]
    return (max(row_err(got[h * G + g], want[g]) for h, (want, _) in enumerate(res) for g in range(G)),
            max(top for _, top in res))


def unswizzle(a):   # bmm's 4-group order (0, 2, 1, 3) back to plain
    return a.reshape(*a.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(a.shape)


# ---------------------------------------------------------------- append
APPEND_FORMS = [("chunk", 1, 0), ("chunk", 1, 70), ("chunk", 33, 0), ("chunk", 33, 70), ("rows", 3, 0), ("pos_dev", 1, 0)]


@pytest.mark.parametrize("mode", ["plain", "bias", "norm"])
@pytest.mark.parametrize("form,T,pos0", APPEND_FORMS, ids=[f"{f}-T{t}-p{p}" for f, t, p in APPEND_FORMS])
@pytest.mark.parametrize("hd", [64, 128])
def test_append(torch, hd, form, T, pos0, mode):
    rng = np.random.default_rng(hd + 3 * T + pos0 + len(mode))
    Hkv, G, n_ctx, eps = 2, 3, 104, 1e-6
    nq, nkv, nhq, nhk = G * Hkv * hd, Hkv * hd, G * Hkv, Hkv
    rows = rng.standard_normal((T, nq + 2 * nkv)).astype(np.float32)
    bias = rng.standard_normal(nq + 2 * nkv).astype(np.float32) if mode == "bias" else None
    for a in (rows[0], bias):
        if a is not None:
            a[nq:nq + 32] = 0                                # an all-zero block: d = 0, q = 0
    w = (1.0 + 0.5 * rng.standard_normal(2 * hd)).astype(np.float32) if mode == "norm" else None
    tab = _rope_table(n_ctx, hd)
    pos = {"chunk": np.arange(pos0, pos0 + T), "rows": np.array([5, n_ctx - 1, 0]), "pos_dev": np.array([17])}[form]
    slots = np.array([2, 0, 3]) if form == "rows" else np.zeros(T, np.int64)
    # fp64 reference of what is stored: (bias | head norm), rotation of the q and k heads' adjacent pairs
    heads = (rows.astype(np.float64) + (0 if bias is None else bias.astype(np.float64))).reshape(T, -1, hd)
    y = heads[:, :nhq + nhk]
    if w is not None:
        wh = np.concatenate([np.tile(w[:hd], (nhq, 1)), np.tile(w[hd:], (nhk, 1))])
        y = y / np.sqrt((y * y).mean(-1, keepdims=True) + eps) * wh
    cs, a0, a1 = tab[pos].astype(np.float64)[:, None], y[..., 0::2], y[..., 1::2]
    rot = np.stack([a0 * cs[..., 0] - a1 * cs[..., 1], a0 * cs[..., 1] + a1 * cs[..., 0]], -1).reshape(y.shape)
    heads = np.concatenate([rot, heads[:, nhq + nhk:]], 1)
    slot_bytes = Hkv * n_ctx * hd * 17 // 16
    sent = [rng.integers(0, 256, ((4 if form == "rows" else 1) + 2 * GUARD, slot_bytes), dtype=np.uint8) for _ in range(2)]
    dK, dV = (torch.from_numpy(s).cuda() for s in sent)
    sq = rng.standard_normal((T + 1, nq)).astype(np.float32)
    dq, drows, dtab = torch.from_numpy(sq).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(tab).cuda()
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("pos", pos.astype(np.int32)), ("slots", slots.astype(np.int32)),
                                                      ("bias", bias), ("w", w)) if v is not None}
    kw = dict(Q8)
    if form == "rows":
        kw.update(pos_arr=dev["pos"].data_ptr(), slot_arr=dev["slots"].data_ptr(), slot_stride=slot_bytes // 2)
    if form == "pos_dev":
        kw.update(pos_dev=dev["pos"].data_ptr())
    head = (drows.data_ptr(), T, pos0, nq, nkv, hd, n_ctx, dtab.data_ptr())
    tail = (dq.data_ptr(), dK.data_ptr() + GUARD * slot_bytes, dV.data_ptr() + GUARD * slot_bytes, stream())
    if mode == "norm":
        hip().qk_norm_rope_kv(*head, dev["w"].data_ptr(), eps, *tail, **kw)
    else:
        hip().rope_kv_prefill(*head, *tail, **({"bias": dev["bias"].data_ptr()} if mode == "bias" else {}), **kw)
    torch.cuda.synchronize()
    gq = dq.cpu().numpy()
    assert np.array_equal(gq[T], sq[T])                      # the row behind the last written one
    worst_q = max(row_err(gq[t], heads[t, :nhq].reshape(-1)) for t in range(T))
    assert worst_q <= NORM_BOUND, worst_q
    worst_d = worst_x = 0.0
    for which, (d_dev, s0) in enumerate(((dK, sent[0]), (dV, sent[1]))):
        got, sl = d_dev.cpu().numpy(), GUARD + slots
        (q8, d8), (want_q, want_d) = q8_unpack(got, Hkv, n_ctx, hd), q8_unpack(s0, Hkv, n_ctx, hd)
        xr = heads[:, nhq + which * nhk:nhq + (which + 1) * nhk]            # [T][Hkv][hd]
        gq8, gd8 = q8[sl, :, pos], d8[sl, :, pos]                           # the written rows, every block judged
        d, dref = gd8.astype(np.float64), np.abs(xr.reshape(T, Hkv, -1, 32)).max(-1) / 127
        ulp = np.spacing(np.maximum(dref, 2.0 ** -14).astype(np.float16)).astype(np.float64)
        assert (np.abs(d - dref) <= ulp).all(), (d, dref)
        err, bound = np.abs(deq(gq8, gd8) - xr), np.repeat(d, 32, -1) / 2 + 2.0 ** -11 * np.abs(xr)
        assert (err <= bound).all(), float((err - bound).max())
        worst_d = max(worst_d, float((np.abs(d - dref) / ulp).max()))
        worst_x = max(worst_x, float((err / np.maximum(bound, 1e-30)).max()))
        want_q[sl, :, pos], want_d[sl, :, pos] = gq8, gd8    # sentinels everywhere but in the written rows
        assert np.array_equal(q8_pack(want_q, want_d), got), "a byte outside the written rows changed"
    print("append", hd, form, T, pos0, mode, f"q {worst_q / NORM_BOUND:.3f} d {worst_d:.3f} x {worst_x:.3f} of their bounds")


# ---------------------------------------------------------------- decode
LENGTHS = [1, 63, 64, 65, 130, 1000]


def _host_caches(rng, n_slots, Hkv, n_ctx, hd, gain=1.0):
    """Random K / V quantised on the host: (fp64 dequantised K, V [S][Hkv][n_ctx][hd], packed K, V bytes)."""
    out = []
    for _ in range(2):
        q, d = q8_quant(gain * rng.standard_normal((n_slots, Hkv, n_ctx, hd)))
        out.append((deq(q, d), q8_pack(q, d)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


@pytest.mark.parametrize("hd,G,big", [(hd, G, False) for hd in (64, 128) for G in (1, 4, 7)] + [(128, 4, True)])
def test_decode(torch, hd, G, big):
    """Single row at every length of LENGTHS, then three batched rows on slots [2, 0, 3]. `big`: logits
    above 80 in magnitude (a missing maximum subtraction overflows)."""
    rng = np.random.default_rng(100 * hd + G)
    Hkv, n_ctx, H, gain, scale = 2, 1024, 2 * G, 5.0 if big else 1.0, 1.0 / np.sqrt(hd)
    K, V, bK, bV = _host_caches(rng, 4, Hkv, n_ctx, hd, gain)
    dK, dV = torch.from_numpy(bK).cuda(), torch.from_numpy(bV).cuda()
    part = torch.zeros(3 * hip().attn_decode_workspace_floats(n_ctx, H, hd), dtype=torch.float32).cuda()
    cnt = torch.zeros(3 * 64, dtype=torch.int32).cuda()
    worst, top = 0.0, 0.0
    for slots, lens in [([0], [L]) for L in LENGTHS] + [([2, 0, 3], [65, 1000, 1])]:
        B = len(slots)
        q = (gain * rng.standard_normal((B, H, hd))).astype(np.float32)
        dq, dslots = torch.from_numpy(q).cuda(), torch.tensor(slots, dtype=torch.int32).cuda()
        dpos = torch.tensor([n - 1 for n in lens], dtype=torch.int32).cuda()
        out, out_h = torch.full((B, H, hd), float("nan")).cuda(), torch.zeros((B, H * hd), dtype=torch.float16).cuda()
        kw = dict(batch=B, slots=dslots.data_ptr(), slot_stride=bK.shape[1] // 2, out_h=out_h.data_ptr()) if B > 1 else {}
        hip().attn_decode(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), dpos.data_ptr(), n_ctx, H, Hkv, hd, scale,
                          part.data_ptr(), out.data_ptr(), stream(), cnt.data_ptr(), **kw, **Q8)
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.float64)
        for b in range(B):
            e, t = worst_rows(got[b], q[b], K[slots[b]], V[slots[b]], lens[b], G, scale)
            worst, top = max(worst, e), max(top, t)
        if B > 1:   # the f16 copy in bmm's 4-group order is the f32 output rounded
            assert np.array_equal(unswizzle(out_h.cpu().numpy()).reshape(B, H, hd), got.astype(np.float32).astype(np.float16))
    assert int(cnt.cpu().abs().sum()) == 0                   # every launch leaves the split counters at 0
    if big:
        assert top > 80, top
    print("decode", hd, G, "logits80" if big else "unit", f"worst / bound {worst / ATTN_BOUND:.3f} (top |logit| {top:.1f})")
    assert worst <= ATTN_BOUND, worst


# ---------------------------------------------------------------- prefill
@pytest.mark.parametrize("out_h", [False, True], ids=["f32", "f16x4"])
@pytest.mark.parametrize("G", [4, 7])
@pytest.mark.parametrize("hd", [64, 128])
def test_prefill(torch, hd, G, out_h):
    """T in {1, 33, 65, 130} x pos0 in {0, 70} as a plain chunk on slot 0, then two packed pieces of unequal length on
    slots 2 and 1. The row behind the last live key of each head carries NaN scales in K and V."""
    rng = np.random.default_rng(7 * hd + G + out_h)
    Hkv, n_ctx, H, scale = 2, 208, 2 * G, 1.0 / np.sqrt(hd)
    K, V, bK, bV = _host_caches(rng, 3, Hkv, n_ctx, hd)
    slot_bytes, n8 = bK.shape[1], Hkv * n_ctx * hd
    worst = 0.0

    def run(pieces, T, pos0):
        nonlocal worst
        rows = sum(n for _, n, _, _ in pieces)
        q = rng.standard_normal((rows, H, hd)).astype(np.float32)
        cK, cV = bK.copy(), bV.copy()
        for _, n, p, slot in pieces:                         # NaN scales in the row behind the last live key
            if p + n < n_ctx:
                for c in (cK, cV):
                    sc = c[slot, n8:].view(np.float16).reshape(Hkv, n_ctx, hd // 32)
                    sc[:, p + n] = np.nan
        dK, dV, dq = torch.from_numpy(cK).cuda(), torch.from_numpy(cV).cuda(), torch.from_numpy(q).cuda()
        out = torch.zeros((rows, H * hd), dtype=torch.float16 if out_h else torch.float32).cuda()
        hip().attn_prefill(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), T, pos0, n_ctx, H, Hkv, hd, scale,
                           out.data_ptr(), stream(), out_h=out_h, pieces=[list(p) for p in pieces] if len(pieces) > 1 else [],
                           slot_stride=slot_bytes // 2, **Q8)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        got = (unswizzle(got) if out_h else got).astype(np.float64).reshape(rows, H, hd)
        assert np.isfinite(got).all()
        for row, n, p, slot in pieces:
            worst = max([worst] + [worst_rows(got[row + t], q[row + t], K[slot], V[slot], p + t + 1, G, scale)[0] for t in range(n)])

    for T, pos0 in [(T, p) for T in (1, 33, 65, 130) for p in (0, 70)]:
        run([(0, T, pos0, 0)], T, pos0)
    run([(0, 41, 70, 2), (41, 130, 3, 1)], 0, 0)
    print("prefill", hd, G, "f16x4" if out_h else "f32", f"worst / bound {worst / ATTN_BOUND:.3f}")
    assert worst <= ATTN_BOUND, worst
