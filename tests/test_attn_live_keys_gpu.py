"""Batched decode attention, which keys a block loads (AttnDecodeArgs::live, LFK_ATTN_LIVE):
0 = every launched block loads its 64 rows before the position is known, 1 = only the keys below a
row's length are loaded, 2 = those spread evenly over the launched splits.

Kernel level, through the attn_decode binding, against a numpy fp64 attention over the keys < L.
The cache rows at and beyond L are NaN: a mode that lets one of them into a sum fails. Bounds: those
of tests/test_kernels_gpu.py for the same kernel and reference (3e-3 plain, 5e-3 over the split-K
raw sums, 3e-3 for the appended key / value rows).
"""
import numpy as np
import pytest

from gpu_helpers import hip, rel_err, stream

pytestmark = pytest.mark.gpu

MODES = [0, 1, 2]
N_SLOTS = 8
SLOTS = [5, 2, 7, 0, 3, 6]            # row -> KV slot, not the identity
LENS = [1, 64, 65, 130, 255, 256]     # one key; one full split; one key in a second block; ...; L = n_ctx
CONFIGS = [(128, 2, 4), (64, 2, 1)]   # head_dim, kv heads, GQA group
KDIM, EPS = 512, 1e-5                 # the raw sums' model width and RMSNorm epsilon


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _attn_ref(q, K, V, L, scale):
    # q [H, D], K / V [Hkv, n_ctx, D]
    H, D = q.shape
    G = H // K.shape[0]
    out = np.zeros((H, D))
    for h in range(H):
        k = K[h // G, :L].astype(np.float64)
        s = k @ q[h].astype(np.float64) * scale
        p = np.exp(s - s.max())
        p /= p.sum()
        out[h] = p @ V[h // G, :L].astype(np.float64)
    return out


def _rot(x, pos, freq):
    """Adjacent pairs of every head rotated by pos * freq[pair]."""
    z = x.astype(np.float64).reshape(*x.shape[:-1], -1, 2)
    ang = float(pos) * freq.astype(np.float64)
    c, s = np.cos(ang), np.sin(ang)
    return np.stack([z[..., 0] * c - z[..., 1] * s, z[..., 0] * s + z[..., 1] * c], -1).reshape(x.shape)


_CASES = {}


def _case(hd, n_kv, G, n_ctx, lens, raw):
    """Inputs and the fp64 reference of one launch, built once per shape and shared by the tests."""
    key = (hd, n_kv, G, n_ctx, tuple(lens), raw)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(hd + 7 * G + n_ctx + 13 * sum(lens) + raw)
    B, H = len(lens), n_kv * G
    nq, nkv = H * hd, n_kv * hd
    scale = 1 / np.sqrt(hd)
    c = dict(hd=hd, n_kv=n_kv, G=G, H=H, n_ctx=n_ctx, lens=list(lens), raw=raw, B=B, nq=nq, nkv=nkv, scale=scale,
             slots=SLOTS[:B])
    Kc = rng.standard_normal((N_SLOTS, n_kv, n_ctx, hd)).astype(np.float16)
    Vc = rng.standard_normal((N_SLOTS, n_kv, n_ctx, hd)).astype(np.float16)
    c["K"], c["V"] = Kc, Vc
    ref = np.zeros((B, H, hd))
    if raw:
        c["qkv"] = (rng.standard_normal((B, nq + 2 * nkv)) * 3).astype(np.float32)
        c["ss"] = np.zeros(16, np.float32)
        c["ss"][:B] = (KDIM * 9 * (0.5 + rng.random(B))).astype(np.float32)
        c["freq"] = (5e5 ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)).astype(np.float32)
        c["kn"], c["vn"] = [], []
        for b, L in enumerate(lens):
            rs = 1.0 / np.sqrt(float(c["ss"][b]) / KDIM + EPS)
            row = c["qkv"][b]
            q = _rot(row[:nq].reshape(H, hd), L - 1, c["freq"]) * rs
            kn = (_rot(row[nq:nq + nkv].reshape(n_kv, hd), L - 1, c["freq"]) * rs).astype(np.float16)
            vn = (row[nq + nkv:].astype(np.float64).reshape(n_kv, hd) * rs).astype(np.float16)
            Kr, Vr = Kc[c["slots"][b]].copy(), Vc[c["slots"][b]].copy()
            Kr[:, L - 1], Vr[:, L - 1] = kn, vn
            ref[b] = _attn_ref(q, Kr, Vr, L, scale)
            c["kn"].append(kn)
            c["vn"].append(vn)
    else:
        c["q"] = rng.standard_normal((B, H, hd)).astype(np.float32)
        for b, L in enumerate(lens):
            ref[b] = _attn_ref(c["q"][b], Kc[c["slots"][b]], Vc[c["slots"][b]], L, scale)
    c["ref"] = ref
    _CASES[key] = c
    return c


def _poisoned(c):
    """The caches with every row the result must not depend on as NaN: rows >= L of each row's slot
    and, in the raw form, the not yet written row L - 1."""
    K, V = c["K"].copy(), c["V"].copy()
    for b, L in enumerate(c["lens"]):
        first = L - 1 if c["raw"] else L
        K[c["slots"][b], :, first:] = np.nan
        V[c["slots"][b], :, first:] = np.nan
    return K, V


class _Bufs:
    """Workspace, split counters and outputs of one shape (kept across launches)."""

    def __init__(self, torch, c):
        B, H, hd, n_ctx = c["B"], c["H"], c["hd"], c["n_ctx"]
        self.part = torch.zeros(B * hip().attn_decode_workspace_floats(n_ctx, H, hd), device="cuda")
        self.cnt = torch.zeros(64 * B, dtype=torch.int32, device="cuda")
        self.out = torch.zeros(B, H * hd, device="cuda")
        self.out_h = torch.zeros(B, H * hd, dtype=torch.float16, device="cuda")


def _launch(torch, c, mode, dK, dV, bufs):
    """One launch; returns (f32 output [B, H, hd], f16 output as its bits [B, H * hd])."""
    B, H, hd, n_kv, n_ctx = c["B"], c["H"], c["hd"], c["n_kv"], c["n_ctx"]
    dpos = torch.tensor([L - 1 for L in c["lens"]], dtype=torch.int32, device="cuda")
    dslots = torch.tensor(c["slots"], dtype=torch.int32, device="cuda")
    bufs.out.fill_(float("nan"))
    bufs.out_h.fill_(float("nan"))
    kw = dict(batch=B, slots=dslots.data_ptr(), slot_stride=n_kv * n_ctx * hd, out_h=bufs.out_h.data_ptr(), live=mode)
    if c["raw"]:
        dq = torch.from_numpy(c["qkv"]).cuda()
        dss, dfreq = torch.from_numpy(c["ss"]).cuda(), torch.from_numpy(c["freq"]).cuda()
        kw.update(qkv_raw=dq.data_ptr(), qkv_ld=c["nq"] + 2 * c["nkv"], k_off=c["nq"], v_off=c["nq"] + c["nkv"],
                  ss=dss.data_ptr(), inv_k=1.0 / KDIM, eps=EPS, rope_freq=dfreq.data_ptr())
    else:
        dq = torch.from_numpy(c["q"]).cuda()
    hip().attn_decode(dq.data_ptr(), dK.data_ptr(), dV.data_ptr(), dpos.data_ptr(), n_ctx, H, n_kv, hd, c["scale"],
                      bufs.part.data_ptr(), bufs.out.data_ptr(), stream(), bufs.cnt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return bufs.out.cpu().numpy().reshape(B, H, hd), bufs.out_h.cpu().numpy().view(np.uint16)


def _check(c, out, tag):
    bound = 5e-3 if c["raw"] else 3e-3
    for b, L in enumerate(c["lens"]):
        err = rel_err(out[b], c["ref"][b]) if np.isfinite(out[b]).all() else float("nan")
        print(f"{tag} L {L}: rel err {err:.3g}")
    for b, L in enumerate(c["lens"]):
        assert np.isfinite(out[b]).all(), (tag, L)
        assert rel_err(out[b], c["ref"][b]) < bound, (tag, L, rel_err(out[b], c["ref"][b]))


def _unswz4(x):
    """f16 output: bmm's k order inside each 4-group, (0, 2, 1, 3), undone."""
    return x.reshape(*x.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(x.shape)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
@pytest.mark.parametrize("hd,n_kv,G", CONFIGS)
def test_live_keys_only(torch, hd, n_kv, G, raw, mode):
    """Every mode attends over the keys < L alone (the rows from L on are NaN, in the raw form the
    stale row L - 1 too); the raw form appends the new key / value at row L - 1 of the row's slot and
    no launch changes any other cache row."""
    c = _case(hd, n_kv, G, 256, LENS, raw)
    Kp, Vp = _poisoned(c)
    dK, dV = torch.from_numpy(Kp).cuda(), torch.from_numpy(Vp).cuda()
    bufs = _Bufs(torch, c)
    out, out_h = _launch(torch, c, mode, dK, dV, bufs)
    _check(c, out, f"hd {hd} G {G} raw {raw} mode {mode}")
    oh = _unswz4(out_h.view(np.float16).astype(np.float64)).reshape(out.shape)
    for b in range(c["B"]):  # the f16 copy (the Wo input): the f32 output rounded
        assert np.isfinite(oh[b]).all() and rel_err(oh[b], out[b]) < 1e-3, b
    assert int(bufs.cnt.abs().sum()) == 0
    Kg, Vg = dK.cpu().numpy(), dV.cpu().numpy()
    if raw:
        for b, L in enumerate(c["lens"]):
            s = c["slots"][b]
            assert rel_err(Kg[s, :, L - 1], c["kn"][b]) < 3e-3, (b, L)
            assert rel_err(Vg[s, :, L - 1], c["vn"][b]) < 3e-3, (b, L)
            Kp[s, :, L - 1], Vp[s, :, L - 1] = Kg[s, :, L - 1], Vg[s, :, L - 1]
    # whole caches, bit for bit (NaN rows included)
    assert np.array_equal(Kg.view(np.uint16), Kp.view(np.uint16))
    assert np.array_equal(Vg.view(np.uint16), Vp.view(np.uint16))


@pytest.mark.parametrize("raw", [False, True], ids=["plain", "raw"])
@pytest.mark.parametrize("hd,n_kv,G", CONFIGS)
def test_mode1_is_mode0_bit_for_bit(torch, hd, n_kv, G, raw):
    """Gated loads keep the key grouping and the merge order: the f32 and the f16 outputs (and the
    appended cache rows) are the bits of mode 0."""
    c = _case(hd, n_kv, G, 256, LENS, raw)
    res = []
    for mode in (0, 1):
        dK, dV = torch.from_numpy(c["K"]).cuda(), torch.from_numpy(c["V"]).cuda()
        out, out_h = _launch(torch, c, mode, dK, dV, _Bufs(torch, c))
        assert np.isfinite(out).all()
        res.append((out.view(np.uint32).copy(), out_h.copy(), dK.cpu().numpy().view(np.uint16),
                    dV.cpu().numpy().view(np.uint16)))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mode", MODES)
def test_counters_reset_between_lengths(torch, mode):
    """Three launches back to back on one workspace and one set of split counters, the rows'
    lengths - and with them the number of splits each kv head waits for - changing in between."""
    hd, n_kv, G = CONFIGS[0]
    sets = [LENS, [256, 130, 1, 65, 64, 255], [100, 17, 200, 33, 256, 129]]
    cases = [_case(hd, n_kv, G, 256, lens, False) for lens in sets]
    bufs = _Bufs(torch, cases[0])
    for c in cases:
        Kp, Vp = _poisoned(c)
        dK, dV = torch.from_numpy(Kp).cuda(), torch.from_numpy(Vp).cuda()
        out, _ = _launch(torch, c, mode, dK, dV, bufs)
        _check(c, out, f"counters mode {mode}")
        assert int(bufs.cnt.abs().sum()) == 0


@pytest.mark.parametrize("mode", MODES)
def test_long_context(torch, mode):
    """n_ctx 2048 (32 launched splits): L = 40 leaves all but one block of a row dead, L = 1500 is
    past the 1024 keys that mode 2 spreads (64-key splits again, two merge batches)."""
    hd, n_kv, G = CONFIGS[0]
    c = _case(hd, n_kv, G, 2048, [40, 1500], False)
    Kp, Vp = _poisoned(c)
    dK, dV = torch.from_numpy(Kp).cuda(), torch.from_numpy(Vp).cuda()
    bufs = _Bufs(torch, c)
    out, _ = _launch(torch, c, mode, dK, dV, bufs)
    _check(c, out, f"n_ctx 2048 mode {mode}")
    assert int(bufs.cnt.abs().sum()) == 0
