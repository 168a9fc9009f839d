"""The batched decode step's Q|K|V stage outside the split-K launch, kernel by kernel against fp64
(qkv_ref): the one-part epilogue (BmmArgs::qkv_epi), bmm_qkv2, the unfused chain bprep -> multi-
segment bmm -> rope_kv_prefill, and the step's first launch (batch_gather / batch_gather_embed).

Caches are allocated with one guard slot on either side of the slots the kernels see and filled
with a sentinel, so a write one position before or past a slot lands in allocated memory and
fails the sentinel check."""
import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from gpu_helpers import dev_bytes, hip, make_matrix, rel_err, stream, to_planar
from qkv_ref import NORM_BOUND, _rope_table, check_qkv, qkv_reference

pytestmark = pytest.mark.gpu

N_CTX = 64
EPS = 1e-5
Q4K, Q5K, Q6K, Q80, Q40 = GGMLType.Q4_K, GGMLType.Q5_K, GGMLType.Q6_K, GGMLType.Q8_0, GGMLType.Q4_0


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _swizzle4(x):
    """bprep's k order inside each 4-group: (0, 2, 1, 3)."""
    return x.reshape(*x.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(x.shape)


_MATS = {}


def _mat(torch, t, R, K, seed):
    """(tile16 copy on the device, dequantised fp32 [R][K]) of a random matrix, built once per shape."""
    key = (int(t), R, K, seed)
    if key not in _MATS:
        raw, W = make_matrix(t, R, K, np.random.default_rng(seed * 7919 + int(t) * 131 + R + K))
        dw = dev_bytes(to_planar(t, raw, R, K))
        tw = torch.empty(hip().t16_bytes(int(t), R, K), dtype=torch.uint8, device="cuda")
        hip().t16_repack(dw.data_ptr(), int(t), R, K, tw.data_ptr(), stream())
        torch.cuda.synchronize()
        _MATS[key] = (tw, W)
    return _MATS[key]


def _positions(rng, B, clamp):
    """Always 0 and N_CTX - 1 (one row: the last position); clamp: also -1 and N_CTX + 5."""
    fixed = [N_CTX - 1] if B == 1 else [0, N_CTX - 1] + ([-1, N_CTX + 5] if clamp else [])
    assert len(fixed) <= B
    pos = np.array(fixed + rng.integers(1, N_CTX - 1, B - len(fixed)).tolist(), np.int32)
    return pos[rng.permutation(B)]


class Case:
    """One Q|K|V problem: three matrices, B activation rows, positions, slots, sentinel-filled buffers."""

    def __init__(self, torch, types, B, K, hd, H=4, Hkv=2, bias=False, staging="xh", clamp=False, seed=0):
        self.torch, self.types, self.B, self.K, self.hd, self.staging = torch, types, B, K, hd, staging
        self.nq, self.nkv = H * hd, Hkv * hd
        self.ncol = self.nq + 2 * self.nkv
        rng = np.random.default_rng(seed + B * 1009 + K + hd * 3 + H + sum(int(t) for t in types) + 17 * bias)
        self.mats = [_mat(torch, t, R, K, i) for i, (t, R) in enumerate(zip(types, (self.nq, self.nkv, self.nkv)))]
        Ws = [m[1] for m in self.mats]
        if staging == "xh":
            self.X = rng.standard_normal((B, K)).astype(np.float16)
            self.nw = None
        else:
            self.X = (rng.standard_normal((B, K)) * 3).astype(np.float32)
            self.nw = (0.5 + rng.random(K)).astype(np.float32)
        self.pos = _positions(rng, B, clamp)
        self.n_slots = B + 2                                    # at least two idle slots
        self.slots = rng.permutation(self.n_slots)[:B].astype(np.int32)
        self.tab = _rope_table(N_CTX, hd)
        args = (self.X, self.nw, EPS, Ws, None, self.pos, self.slots, self.tab, N_CTX, hd, staging)
        self.ref = qkv_reference(*args)
        self.bias = None
        if bias:   # ~3x the projection's rms: a missing or late bias is far outside every bound
            rms = float(np.sqrt(np.mean(self.ref.raw ** 2)))
            self.bias = (rng.standard_normal(self.ncol) * 3 * rms).astype(np.float32)
            self.ref = qkv_reference(*args[:4], self.bias, *args[5:])
        shape = (self.n_slots + 2, Hkv, N_CTX, hd)
        self.sentK = rng.standard_normal(shape).astype(np.float16)
        self.sentV = rng.standard_normal(shape).astype(np.float16)
        self.slot_stride = Hkv * N_CTX * hd
        self.dpos = torch.from_numpy(self.pos).cuda()
        self.dslots = torch.from_numpy(self.slots).cuda()
        self.dtab = torch.from_numpy(self.tab).cuda()
        self.dbias = torch.from_numpy(self.bias).cuda() if bias else None
        self.dnw = torch.from_numpy(self.nw).cuda() if self.nw is not None else None

    def mat_args(self):
        return [(m[0].data_ptr(), int(t), R) for m, t, R in zip(self.mats, self.types, (self.nq, self.nkv, self.nkv))]

    def caches(self):
        torch = self.torch
        return torch.from_numpy(self.sentK).cuda(), torch.from_numpy(self.sentV).cuda()

    def fused(self, two_launch=True):
        """The one-part epilogue launch(es). Returns (one launch?, q_out, K cache, V cache) as NumPy."""
        torch, B, K = self.torch, self.B, self.K
        q_ld = self.nq + 4
        self.sentq = np.random.default_rng(3).standard_normal((B + 1, q_ld)).astype(np.float32)
        dq = torch.from_numpy(self.sentq).cuda()
        dK, dV = self.caches()
        kw = dict(fused=True, q_out=dq.data_ptr(), q_ld=q_ld, k_cache=dK[1].data_ptr(), v_cache=dV[1].data_ptr(),
                  slot_stride=self.slot_stride, n_ctx=N_CTX, head_dim=self.hd, pos=self.dpos.data_ptr(),
                  slots=self.dslots.data_ptr(), rope=self.dtab.data_ptr(),
                  bias=self.dbias.data_ptr() if self.dbias is not None else 0, two_launch=two_launch)
        if self.staging == "xh":
            dx = torch.from_numpy(_swizzle4(self.X)).cuda()
            kw.update(xh=dx.data_ptr(), ldh=K)
        else:
            ldxf = K + 4
            dx = torch.zeros(B, ldxf, device="cuda")
            dx[:, :K] = torch.from_numpy(self.X).cuda()
            kw.update(xf=dx.data_ptr(), ldxf=ldxf, norm=self.dnw.data_ptr(), eps=EPS)
        one = hip().bmm_qkv(self.mat_args(), K, B, stream(), **kw)
        torch.cuda.synchronize()
        return one, dq.cpu().numpy(), dK.cpu().numpy(), dV.cpu().numpy()

    def check(self, q, Kc, Vc):
        w = check_qkv(q, Kc, Vc, self.ref, self.sentK, self.sentV, sentinel_q=self.sentq, slot0=1)
        print(f"worst error / bound: norm {w['norm']:.3f} element {w['elem']:.3f}")
        return w


# ------------------------------------------------------------------ a. one-part epilogue, one type
EPI_SHAPES = [  # (B, K, hd, H, Hkv, bias, clamp)
    (1, 256, 64, 4, 2, False, False),      # one step: seven of the eight waves idle
    (9, 4096, 128, 4, 2, False, False),    # the largest B that fits at the 8B width
    (9, 4096, 128, 4, 2, True, False),
    (16, 2304, 128, 4, 2, False, False),   # the largest K at B = 16; 9 steps: the ping-pong roles swap per tile
    (5, 1024, 64, 4, 2, False, True),      # positions -1 and N_CTX + 5 clamped
    (5, 1024, 64, 4, 2, True, True),
    (5, 1024, 72, 4, 1, False, False),     # K and V segments of 72 rows: a partial last tile
    (5, 1024, 72, 4, 1, True, False),      # ... whose bias reads are clamped to the segment
]


def test_bmm_qkv_fits_boundaries(torch):
    for B, K, *_ in EPI_SHAPES:
        assert hip().bmm_qkv_fits(K, B), (B, K)
    assert not hip().bmm_qkv_fits(4096, 10)
    assert not hip().bmm_qkv_fits(2560, 16)


@pytest.mark.parametrize("t", [Q4K, Q6K, Q80, Q5K, Q40], ids=lambda t: t.name)
@pytest.mark.parametrize("B,K,hd,H,Hkv,bias,clamp", EPI_SHAPES)
def test_bmm_qkv_epilogue_vs_fp64(torch, t, B, K, hd, H, Hkv, bias, clamp):
    """qkv_epilogue<BIAS> over xh, one weight type: q_out, the K / V cache rows and everything
    around them against the fp64 projection + bias + RoPE."""
    assert hip().bmm_qkv_fits(K, B)
    c = Case(torch, (t,) * 3, B, K, hd, H, Hkv, bias=bias, clamp=clamp)
    one, q, Kc, Vc = c.fused()
    assert not one   # one run: a plain bmm launch
    c.check(q, Kc, Vc)


# ------------------------------------------------------------------ b. ... with the folded norm
@pytest.mark.parametrize("t", [Q4K, Q6K], ids=lambda t: t.name)
@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("bias", [False, True])
def test_bmm_qkv_epilogue_folded_norm(torch, t, B, bias):
    """The same epilogue over the fp32 rows with the RMSNorm folded into the staging: f16(x * w)
    staged, the column scale applied to the reduced tile before bias and rotation."""
    K = 4096
    assert hip().bmm_norm_fits(K, B)
    c = Case(torch, (t,) * 3, B, K, 128, bias=bias, staging="folded")
    one, q, Kc, Vc = c.fused()
    assert not one
    c.check(q, Kc, Vc)


# ------------------------------------------------------------------ c. two runs, one launch
def _many_tiles_heads(torch, hd):
    """Q heads so that the Q|K and V runs together hold more tiles than two per CU."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H = 2 * cus * 16 // hd + 2
    assert (H * hd + 2 * 2 * hd) // 16 > 2 * cus
    return H


@pytest.mark.parametrize("tv", [Q6K, Q5K], ids=lambda t: t.name)
@pytest.mark.parametrize("B", [3, 16])
@pytest.mark.parametrize("shape", ["small", "many_tiles"])
def test_bmm_qkv2_two_types_one_launch(torch, tv, B, shape):
    """Q|K Q4_K + V Q6_K / Q5_K through bmm_qkv2: against fp64, and bit-identical to the two runs
    launched one by one. many_tiles: more tiles than resident blocks, so blocks of both runs walk
    several tiles and the runs' block split is not one tile per block."""
    if shape == "small":
        K, hd, H = 1024, 64, 4
    else:
        K, hd, H = 256, 128, _many_tiles_heads(torch, 128)
    c = Case(torch, (Q4K, Q4K, tv), B, K, hd, H, 2, bias=(B == 3))
    one, q, Kc, Vc = c.fused(two_launch=True)
    assert one, "bmm_qkv2 refused a mix it serves"
    c.check(q, Kc, Vc)
    one2, q2, Kc2, Vc2 = c.fused(two_launch=False)
    assert not one2
    for a, b in ((q, q2), (Kc, Kc2), (Vc, Vc2)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("B", [3, 16])
def test_bmm_qkv2_refused_mix_falls_back(torch, B):
    """Q Q4_K + K|V Q8_0: two runs bmm_qkv2 does not take - the launches one by one."""
    c = Case(torch, (Q4K, Q80, Q80), B, 1024, 64, bias=(B == 3))
    one, q, Kc, Vc = c.fused(two_launch=True)
    assert not one
    c.check(q, Kc, Vc)


# ------------------------------------------------------------------ d. the unfused chain
@pytest.mark.parametrize("types", [(Q4K,) * 3, (Q4K, Q4K, Q6K)], ids=["nseg3", "nseg2+1"])
@pytest.mark.parametrize("B,K", [(10, 4096), (16, 2560)])
@pytest.mark.parametrize("bias", [False, True])
def test_unfused_qkv_path_vs_fp64(torch, types, B, K, bias):
    """Where the x slice does not fit one K part: bprep (norm, zeroing qkv_), the multi-segment
    split-K bmm into qkv_, rope_kv_prefill with position / slot arrays. The intermediate qkv_ rows
    are checked too, so a failure names its stage."""
    assert not hip().bmm_qkv_fits(K, B)
    hd = 128
    c = Case(torch, types, B, K, hd, bias=bias, staging="bprep", clamp=True)
    dx = torch.from_numpy(c.X).cuda()
    xh = torch.zeros(B, K, dtype=torch.float16, device="cuda")
    qkv = torch.full((B + 1, c.ncol), 7.0, device="cuda")      # the zero side job clears rows < B
    hip().bprep(dx.data_ptr(), K, False, c.dnw.data_ptr(), EPS, K, B, xh.data_ptr(), K, stream(),
                qkv.data_ptr(), B * c.ncol)
    one = hip().bmm_qkv(c.mat_args(), K, B, stream(), xh=xh.data_ptr(), ldh=K, fused=False,
                        out=qkv.data_ptr(), ldo=c.ncol)
    assert not one
    torch.cuda.synchronize()
    raw = qkv.cpu().numpy()
    assert np.all(raw[B] == 7.0)
    for b in range(B):
        for name, lo, hi in (("q", 0, c.nq), ("k", c.nq, c.nq + c.nkv), ("v", c.nq + c.nkv, c.ncol)):
            e = rel_err(raw[b, lo:hi], c.ref.raw[b, lo:hi])
            assert e < NORM_BOUND, ("qkv_ after the bmm", name, b, e)
    c.sentq = np.random.default_rng(4).standard_normal((B + 1, c.nq)).astype(np.float32)
    dq = torch.from_numpy(c.sentq).cuda()
    dK, dV = c.caches()
    hip().rope_kv_prefill(qkv.data_ptr(), B, 0, c.nq, c.nkv, hd, N_CTX, c.dtab.data_ptr(), dq.data_ptr(),
                          dK[1].data_ptr(), dV[1].data_ptr(), stream(), pos_arr=c.dpos.data_ptr(),
                          slot_arr=c.dslots.data_ptr(), slot_stride=c.slot_stride,
                          bias=c.dbias.data_ptr() if bias else 0)
    torch.cuda.synchronize()
    c.check(dq.cpu().numpy(), dK.cpu().numpy(), dV.cpu().numpy())


# ------------------------------------------------------------------ e. rope_kv_prefill alone
def _f32(x):
    return np.asarray(x, np.float32)


def _rot_candidates(a0, a1, c, s):
    """The kernel's y0 = a0 c - a1 s and y1 = a0 s + a1 c in fp32: the two-product form, and the two
    forms with one product contracted into an fma (a compiler may pick any). fp32 products are
    exact in fp64, so the fma forms are one fp64 operation rounded to fp32."""
    a0, a1, c, s = (np.asarray(v, np.float64) for v in (a0, a1, c, s))
    p = lambda x, y: _f32(x * y).astype(np.float64)   # a rounded fp32 product
    y0 = [_f32(p(a0, c) - p(a1, s)), _f32(a0 * c - p(a1, s)), _f32(p(a0, c) - a1 * s)]
    y1 = [_f32(p(a0, s) + p(a1, c)), _f32(a0 * s + p(a1, c)), _f32(p(a0, s) + a1 * c)]
    return y0, y1


@pytest.mark.parametrize("hd,H,Hkv", [(64, 4, 2), (128, 4, 2), (64, 2, 1)],   # the last: 128 pairs, half the block idle
                         ids=["hd64", "hd128", "short_row"])
@pytest.mark.parametrize("form", ["prompt", "batched"])
@pytest.mark.parametrize("bias", [False, True])
def test_rope_kv_prefill_alone(torch, hd, H, Hkv, form, bias):
    """qkv rows given directly (no GEMM noise): Q to 1e-6, the cache rows exactly f16 of the
    kernel's fp32 formula, every other cache element and q row untouched."""
    rng = np.random.default_rng(hd + H + 7 * bias + (form == "batched"))
    nq, nkv = H * hd, Hkv * hd
    ncol = nq + 2 * nkv
    assert (ncol // 2 < 256) == (H == 2)
    T = 5
    if form == "prompt":
        pos_in, pos = None, 7 + np.arange(T)
        slots = np.zeros(T, np.int64)
        n_slots = 1
    else:
        pos_in = np.array([0, N_CTX - 1, -1, N_CTX + 5, 23], np.int32)[rng.permutation(T)]
        pos = np.clip(pos_in, 0, N_CTX - 1)
        n_slots = T + 2
        slots = rng.permutation(n_slots)[:T]
    rows = rng.standard_normal((T, ncol)).astype(np.float32)
    b32 = (rng.standard_normal(ncol) * 3).astype(np.float32) if bias else None
    tab = _rope_table(N_CTX, hd)
    y = rows + b32[None, :] if bias else rows                    # fp32, as the kernel adds it
    sentK = rng.standard_normal((n_slots + 2, Hkv, N_CTX, hd)).astype(np.float16)
    sentV = rng.standard_normal((n_slots + 2, Hkv, N_CTX, hd)).astype(np.float16)
    sentq = rng.standard_normal((T + 1, nq)).astype(np.float32)
    dq, dK, dV = (torch.from_numpy(a).cuda() for a in (sentq, sentK, sentV))
    drows, dtab = torch.from_numpy(rows).cuda(), torch.from_numpy(tab).cuda()
    dbias = torch.from_numpy(b32).cuda() if bias else None
    kw = {}
    if form == "batched":
        dpos, dslots = torch.from_numpy(pos_in).cuda(), torch.from_numpy(slots.astype(np.int32)).cuda()
        kw = dict(pos_arr=dpos.data_ptr(), slot_arr=dslots.data_ptr(), slot_stride=Hkv * N_CTX * hd)
    hip().rope_kv_prefill(drows.data_ptr(), T, 7 if form == "prompt" else 0, nq, nkv, hd, N_CTX, dtab.data_ptr(),
                          dq.data_ptr(), dK[1].data_ptr(), dV[1].data_ptr(), stream(),
                          bias=dbias.data_ptr() if bias else 0, **kw)
    torch.cuda.synchronize()
    gq, gK, gV = dq.cpu().numpy(), dK.cpu().numpy(), dV.cpu().numpy()
    assert np.array_equal(gq[T].view(np.uint32), sentq[T].view(np.uint32))
    # expected caches per candidate form: the sentinel with the rows' (slot, head, pos) replaced
    expK = [sentK.copy() for _ in range(9)]
    expV = sentV.copy()
    for t in range(T):
        c = np.tile(tab[pos[t], :, 0], H + Hkv)                  # per pair of the Q|K columns
        s = np.tile(tab[pos[t], :, 1], H + Hkv)
        a0, a1 = y[t, 0:nq + nkv:2], y[t, 1:nq + nkv:2]
        y0, y1 = _rot_candidates(a0, a1, c, s)
        # Q: within three fp32 roundings of the exact rotation of the fp32 inputs, relative to the
        # terms' size (1e-6 > 3 * 2^-24), and 1e-6 of the row in norm
        a0d, a1d, cd, sd = (v.astype(np.float64) for v in (a0, a1, c, s))
        ex0, ex1 = a0d * cd - a1d * sd, a0d * sd + a1d * cd
        nqp = nq // 2
        assert np.all(np.abs(gq[t, 0::2] - ex0[:nqp]) <= 1e-6 * (np.abs(a0d * cd) + np.abs(a1d * sd))[:nqp])
        assert np.all(np.abs(gq[t, 1::2] - ex1[:nqp]) <= 1e-6 * (np.abs(a0d * sd) + np.abs(a1d * cd))[:nqp])
        assert rel_err(gq[t], np.stack([ex0[:nqp], ex1[:nqp]], -1).ravel()) < 1e-6
        for i in range(3):
            for j in range(3):
                k = np.stack([y0[i][nqp:], y1[j][nqp:]], -1).astype(np.float16).reshape(Hkv, hd)
                expK[3 * i + j][1 + slots[t], :, pos[t]] = k
        expV[1 + slots[t], :, pos[t]] = y[t, nq + nkv:].astype(np.float16).reshape(Hkv, hd)
    assert np.array_equal(gV.view(np.uint16), expV.view(np.uint16))
    assert any(np.array_equal(gK.view(np.uint16), e.view(np.uint16)) for e in expK)


# ------------------------------------------------------------------ f. the step's first launch
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("zero_n", [0, 1, 70, 300])
def test_batch_gather_and_embed(torch, B, zero_n):
    """batch_gather and batch_gather_embed: tok / pos of each row's slot, the embedded rows equal
    to embed's bit for bit, entries past B untouched, and the strided zero side job clearing
    exactly the words i * stride, i < zero_n."""
    rng = np.random.default_rng(B * 13 + zero_n)
    n_state, i_tok, i_pos = hip().state_layout()
    V, d, n_slots, stride = 300, 256, 20, 32
    slots = rng.permutation(n_slots)[:B].astype(np.int32)
    toks = (1 + rng.permutation(V - 2)[:n_slots]).astype(np.int32)      # distinct, in [1, V - 2]
    toks[slots[-1]] = V - 1                                             # the table's last row
    if B > 1:
        toks[slots[0]] = 0                                              # ... and its first
    state = rng.integers(1000, 2000, (n_slots, n_state)).astype(np.int32)
    state[:, i_tok] = toks
    state[:, i_pos] = rng.permutation(500)[:n_slots]
    dstate, dslots = torch.from_numpy(state).cuda(), torch.from_numpy(slots).cuda()

    def outputs():
        tok = torch.full((B + 3,), -7, dtype=torch.int32, device="cuda")
        pos = torch.full((B + 3,), -9, dtype=torch.int32, device="cuda")
        z = torch.full((max(zero_n, 1) * stride + 5,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        return tok, pos, z

    def check_common(tok, pos, z):
        tok, pos, z = tok.cpu().numpy(), pos.cpu().numpy(), z.cpu().numpy()
        assert np.array_equal(tok[:B], state[slots, i_tok]) and np.all(tok[B:] == -7)
        assert np.array_equal(pos[:B], state[slots, i_pos]) and np.all(pos[B:] == -9)
        want = np.full_like(z, 0x5A5A5A5A)
        want[np.arange(zero_n) * stride] = 0
        assert np.array_equal(z, want)

    tok, pos, z = outputs()
    hip().batch_gather(dslots.data_ptr(), B, dstate.data_ptr(), tok.data_ptr(), pos.data_ptr(), stream(),
                       zero=z.data_ptr(), zero_n=zero_n, zero_stride=stride)
    torch.cuda.synchronize()
    check_common(tok, pos, z)
    for t in (GGMLType.Q4_K, GGMLType.Q8_0):      # a 256-block and a 32-block type
        raw, _ = make_matrix(t, V, d, np.random.default_rng(int(t)))
        dw = dev_bytes(to_planar(t, raw, V, d))
        tok, pos, z = outputs()
        x = torch.full((B + 1, d), 3.0, device="cuda")
        hip().batch_gather_embed(dslots.data_ptr(), B, dstate.data_ptr(), tok.data_ptr(), pos.data_ptr(),
                                 dw.data_ptr(), int(t), V, d, x.data_ptr(), stream(), zero=z.data_ptr(),
                                 zero_n=zero_n, zero_stride=stride)
        torch.cuda.synchronize()
        check_common(tok, pos, z)
        want = torch.zeros(B, d, device="cuda")
        dtoks = torch.from_numpy(state[slots, i_tok].copy()).cuda()
        hip().embed(dw.data_ptr(), int(t), V, d, dtoks.data_ptr(), B, want.data_ptr(), stream())
        torch.cuda.synchronize()
        assert torch.equal(x[:B].view(torch.int32), want.view(torch.int32))
        assert bool((x[B] == 3.0).all())
