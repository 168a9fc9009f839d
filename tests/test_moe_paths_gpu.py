"""The MoE expert paths at kernel level, at the shapes where they can go wrong and the engine tests
(tiny models, prompts of 40 tokens, F <= 1024) never take them:

  * grouped prefill - moe_route_group, gather_rows_bf16, gemm_t16 / gemm_dq over a device-side row
    range (groups crossing a 64- or 128-token tile, larger than the rows hint, empty, equal to T;
    the grouped split-K STORE), moe_scatter_add - every launch on its own with poisoned buffers, so
    a store past a group's last row shows (in the engine the next expert overwrites it);
  * batched decode - bmm over the stacked experts with per-row routing weights (BmmArgs::ew):
    whole-expert skipping in the gate/up and in the K-concatenated down over poisoned memory,
    Mixtral's 7-step parts-per-expert search, the folded norm;
  * single-row decode - moe_down_splitk with more than one 64-chunk part, and the per-slot kernel's
    K-quant instantiations.

References and checkers: tests/moe_ref.py (CPU self-test: tests/test_moe_ref.py)."""
import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from gpu_helpers import dev_bytes, hip, make_matrix, q8_emulate, rel_err, stream, to_planar
from qkv_ref import staged_x
import moe_ref as mr

pytestmark = pytest.mark.gpu

Q4_K, Q5_K, Q6_K, Q8_0 = GGMLType.Q4_K, GGMLType.Q5_K, GGMLType.Q6_K, GGMLType.Q8_0
SLACK = 128   # rows allocated past T k in every gathered buffer: they must keep their sentinel


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch
    _CACHE.clear()   # the module's weights leave the device with it


def _filled(torch, shape, dtype, pattern):
    """A device tensor of `dtype` whose every element has the bit pattern `pattern`."""
    it = {2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]
    return torch.full(shape, pattern, dtype=it, device="cuda").view(dtype)


def _bits(torch, t):
    it, ut = {2: (torch.int16, np.uint16), 4: (torch.int32, np.uint32)}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy().view(ut)


def _values(bits, kind):
    """uint16 bits of f16 (un-swizzled from the kernels' 4-group order) or bf16 rows -> fp64."""
    if kind == "f16":
        return mr.swizzle4(bits.view(np.float16).astype(np.float64))
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


_CACHE = {}


def _experts(t, E, d, F):
    """E experts' gate/up [2F][d] (gate / up rows in 32-row groups) and down [d][F] matrices: planar
    copies on the device, the dequantised values on the host. Made once per shape and type."""
    key = ("w", int(t), E, d, F)
    if key not in _CACHE:
        rng = np.random.default_rng(int(t) * 1000 + E + d + F)
        gu = [make_matrix(t, 2 * F, d, rng) for _ in range(E)]
        dn = [make_matrix(t, d, F, rng) for _ in range(E)]
        _CACHE[key] = dict(Wgu=[w for _, w in gu], Wd=[w for _, w in dn],
                           pgu=[dev_bytes(to_planar(t, r, 2 * F, d)) for r, _ in gu],
                           pdn=[dev_bytes(to_planar(t, r, d, F)) for r, _ in dn])
    return _CACHE[key]


def _stacked_t16(torch, t, E, d, F):
    """The experts' tile16 copies as the engine stacks them for its batched and grouped paths:

      gate/up: each expert's SwiGLU tile16 copy (t16_repack swiglu = true) back to back - expert e
               is bytes [e gu1, (e + 1) gu1), i.e. tiles [e 2F / 16, (e + 1) 2F / 16) of one matrix
               of E 2F rows;
      down:    one matrix of d rows and K = E F: every 16-row tile holds expert 0's F / 256 steps,
               then expert 1's, ... - expert e's own tile-major copy ([d / 16 tiles][run bytes])
               strided into bytes [e run, (e + 1) run) of every tile of E run bytes.

    Returns (gate/up bytes, down bytes, gu1, the down's tile stride E run)."""
    key = ("t16", int(t), E, d, F)
    if key not in _CACHE:
        ex, h = _experts(t, E, d, F), hip()
        gu1, dn1, dtiles = h.t16_bytes(int(t), 2 * F, d), h.t16_bytes(int(t), d, F), d // 16
        run = dn1 // dtiles
        assert run * dtiles == dn1 and run * E == h.t16_bytes(int(t), 16, E * F)
        gu = torch.empty(E * gu1, dtype=torch.uint8, device="cuda")
        dn = torch.empty((dtiles, E, run), dtype=torch.uint8, device="cuda")
        tmp = torch.empty(dn1, dtype=torch.uint8, device="cuda")
        for e in range(E):
            h.t16_repack(ex["pgu"][e].data_ptr(), int(t), 2 * F, d, gu.data_ptr() + e * gu1, stream(), swiglu=True)
            h.t16_repack(ex["pdn"][e].data_ptr(), int(t), d, F, tmp.data_ptr(), stream())
            dn[:, e, :] = tmp.view(dtiles, run)
        torch.cuda.synchronize()
        _CACHE[key] = (gu, dn, gu1, run * E)
    return _CACHE[key]


# ------------------------------------------------------------------ routing and data movement
def _route_dev(torch, lg, k, tail=8):
    """moe_route_group on logits lg [T][E]; every output has `tail` sentinel elements past its end."""
    T, E = lg.shape
    R = T * k
    dl = torch.from_numpy(lg).cuda()
    o = dict(sel=torch.full((R + tail,), -7, dtype=torch.int32, device="cuda"),
             selw=torch.full((R + tail,), -7.0, device="cuda"),
             cnt_off=torch.full((E + 1 + tail,), -7, dtype=torch.int32, device="cuda"),
             tok=torch.full((R + tail,), -7, dtype=torch.int32, device="cuda"),
             gw=torch.full((R + tail,), -7.0, device="cuda"),
             pos=torch.full((R + tail,), -7, dtype=torch.int32, device="cuda"))
    hip().moe_route_group(dl.data_ptr(), T, E, k, o["sel"].data_ptr(), o["selw"].data_ptr(), o["cnt_off"].data_ptr(),
                          o["tok"].data_ptr(), o["gw"].data_ptr(), o["pos"].data_ptr(), stream())
    torch.cuda.synchronize()
    return o


def _check_route(o, lg, k):
    T, E = lg.shape
    R = T * k
    n = dict(sel=R, selw=R, cnt_off=E + 1, tok=R, gw=R, pos=R)
    host = {name: v.cpu().numpy() for name, v in o.items()}
    for name, v in host.items():
        assert np.all(v[n[name]:] == -7), (name, "written past its end")
    ref = mr.route_reference(lg, k)
    mr.check_routing({name: v[:n[name]] for name, v in host.items()}, ref, T, E, k)
    return ref


@pytest.mark.parametrize("T,E,k,kind", mr.ROUTE_CASES)
def test_moe_route_group_vs_fp64(torch, T, E, k, kind):
    """Softmax, top-k (lowest index on ties), renormalised weights and the per-expert row lists in
    ascending token order: sel, cnt_off, tok and pos exactly, the weights at the router bound. The
    inputs hold rows of exactly equal logits, an empty expert, an expert that takes every token."""
    lg = mr.routing_logits(T, E, k, kind, mr.route_seed(T, E, k, kind))
    assert mr.route_margin(lg, k) >= mr.MARGIN
    ref = _check_route(_route_dev(torch, lg, k), lg, k)
    if kind == "random" and T > 3:
        assert list(ref.sel[3]) == list(range(k))


@pytest.mark.parametrize("d", [256, 4096])
def test_gather_rows_bit_equal(torch, d):
    rng = np.random.default_rng(d)
    T, R = 37, 74
    src = torch.from_numpy(rng.integers(0, 1 << 15, (T, d), dtype=np.int16)).cuda()
    tok = rng.integers(0, T, R).astype(np.int32)
    tok[:2] = [T - 1, 0]
    dt = torch.from_numpy(tok).cuda()
    dst = _filled(torch, (R + 5, d), torch.float16, mr.NAN16)
    hip().gather_rows(src.data_ptr(), dt.data_ptr(), R, d, dst.data_ptr(), stream())
    torch.cuda.synchronize()
    got = _bits(torch, dst)
    assert np.array_equal(got[:R], src.cpu().numpy().view(np.uint16)[tok])
    assert np.all(got[R:] == mr.NAN16)


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("d", [250, 512])
def test_moe_scatter_add_vs_fp64(torch, k, d):
    """acc[t] += sum_j gw[pos[t k + j]] y[pos[t k + j]] against fp64 of the same f32 inputs, per element
    within the fp32 sum's bound (k + 1) 2^-23 (|acc0| + sum_j |gw_j y_j|); rows past T are untouched."""
    rng = np.random.default_rng(10 * k + d)
    T = 33
    R = T * k
    pos = rng.permutation(R).astype(np.int32)
    gw = (0.05 + rng.random(R)).astype(np.float32)
    y = rng.standard_normal((R, d)).astype(np.float32)
    acc0 = rng.standard_normal((T + 2, d)).astype(np.float32)
    dp, dg, dy, da = (torch.from_numpy(a).cuda() for a in (pos, gw, y, acc0))
    hip().moe_scatter_add(da.data_ptr(), dy.data_ptr(), dp.data_ptr(), dg.data_ptr(), T, k, d, stream())
    torch.cuda.synchronize()
    got = da.cpu().numpy()
    p = pos.reshape(T, k)
    terms = np.stack([gw[p[:, j]].astype(np.float64)[:, None] * y[p[:, j]].astype(np.float64) for j in range(k)])
    ref = acc0[:T].astype(np.float64) + terms.sum(0)
    frac = np.abs(got[:T] - ref) / mr.scatter_bound(acc0[:T].astype(np.float64), terms)
    print(f"MOE_FRAC scatter_add k={k} d={d} {frac.max():.3f}")
    i = np.unravel_index(int(np.argmax(frac)), frac.shape)
    assert frac[i] <= 1.0, ("element", i, float(got[:T][i]), float(ref[i]), float(frac[i]))
    assert np.array_equal(got[T:], acc0[T:])


# ------------------------------------------------------------------ grouped GEMMs
class _Grouped:
    """One routed prompt as the engine sets the grouped expert GEMMs up: E = 4, k = 2, d = 512; the
    row counts come from constructed logits run through moe_route_group itself; the 2-byte token
    rows are gathered by gather_rows into T k + SLACK rows (the slack rows hold a NaN pattern)."""

    E, k, d = 4, 2, 512

    def __init__(self, torch, form, t, F, pat):
        self.torch, self.form, self.t, self.F = torch, form, t, F
        E, k, d = self.E, self.k, self.d
        self.T, counts = mr.GROUP_PATTERNS[pat]
        T = self.T
        self.R = T * k
        lg = mr.logits_for_counts(T, counts, 50 + pat)
        self.rt_dev = _route_dev(torch, lg, k)
        self.rt = _check_route(self.rt_dev, lg, k)
        self.off = [int(v) for v in self.rt.cnt_off]
        assert tuple(np.diff(self.off)) == counts
        self.hint = max(1, T * k // E)    # the engine's rows_hint
        self.ex = _experts(t, E, d, F)
        rng = np.random.default_rng(pat * 10 + int(t) + F)
        X = rng.standard_normal((T, d)).astype(np.float32)
        if form == "t16":   # f16 rows in the 4-group k order (rmsnorm_bf16's f16sw output)
            self.kind, self.dt, self.nan = "f16", torch.float16, mr.NAN16
            self.x_ref = X.astype(np.float16).astype(np.float64)
            self.x = torch.from_numpy(mr.swizzle4(X.astype(np.float16))).cuda()
            self.gu, self.dn, self.gu1, self.tstride = _stacked_t16(torch, t, E, d, F)
        else:               # bf16 rows
            self.kind, self.dt, self.nan = "bf16", torch.bfloat16, mr.NANBF
            self.x = torch.from_numpy(X).cuda().to(torch.bfloat16)
            self.x_ref = self.x.float().cpu().numpy().astype(np.float64)
        self.xg = _filled(torch, (self.R + SLACK, d), self.dt, self.nan)
        hip().gather_rows(self.x.data_ptr(), self.rt_dev["tok"].data_ptr(), self.R, d, self.xg.data_ptr(), stream())
        torch.cuda.synchronize()
        xb = _bits(torch, self.xg)
        assert np.array_equal(xb[:self.R], _bits(torch, self.x)[self.rt.tok]) and np.all(xb[self.R:] == self.nan)
        self.xg_ref = self.x_ref[self.rt.tok]

    def seg(self, e):
        return self.rt_dev["cnt_off"].data_ptr() + 4 * e

    def gate_up(self, e, h, ldh):
        """Expert e's rows of silu(gate) * up into h [rows][ldh] (ldh = F for the planar form)."""
        F, d, t = self.F, self.d, int(self.t)
        if self.form == "t16":
            hip().gemm_t16(self.gu.data_ptr() + e * self.gu1, t, 2 * F, d, self.xg.data_ptr(), self.T, 0, 0,
                           h.data_ptr(), ldh, 2, stream(), seg_dev=self.seg(e), rows_hint=self.hint)
        else:
            assert ldh == F
            hip().gemm(self.ex["pgu"][e].data_ptr(), t, 2 * F, d, self.xg.data_ptr(), self.T, 0, h.data_ptr(), 0, 2,
                       stream(), seg_dev=self.seg(e), rows_hint=self.hint)

    def down(self, e, h, y, ldo):
        """Expert e's rows of h [rows][F] through its down projection into the pre-zeroed y [rows][ldo]."""
        F, d, t = self.F, self.d, int(self.t)
        if self.form == "t16":
            hip().gemm_t16(self.dn.data_ptr(), t, d, F, h.data_ptr(), self.T, y.data_ptr(), ldo, 0, 0, 0, stream(),
                           seg_dev=self.seg(e), rows_hint=self.hint, out_zeroed=True, tile_stride=self.tstride,
                           step0=e * (F // 256))
        else:
            hip().gemm(self.ex["pdn"][e].data_ptr(), t, d, F, h.data_ptr(), self.T, y.data_ptr(), 0, ldo, 0, stream(),
                       seg_dev=self.seg(e), rows_hint=self.hint)


GROUP_CASES = ([(t, 1024, p) for t in (Q4_K, Q6_K) for p in range(4)] + [(Q4_K, 512, 0), (Q6_K, 512, 2)]
               + [(Q5_K, 1024, 0), (Q8_0, 1024, 0)])
GROUP_BOUNDS = {"t16": (mr.T16_GU, mr.T16_DN), "dq": (mr.DQ_GU, mr.DQ_DN)}


@pytest.mark.parametrize("t,F,pat", GROUP_CASES)
@pytest.mark.parametrize("form", ["t16", "dq"])
def test_grouped_expert_launches(torch, form, t, F, pat):
    """Every expert's gate/up and down launch on its own, over fresh sentinels: the group's rows
    against fp64 of the same 2-byte inputs, row by row (the down over the SwiGLU rows read back from
    the device), and every row outside [off[e], off[e + 1]) - the other groups, the slack rows past
    T k - and every pad column bit-identical to the sentinel. F = 1024: the down splits K (4 steps)
    and adds into the pre-zeroed output, so its sentinel is 0; F = 512: the unsplit STORE over NaN."""
    g = _Grouped(torch, form, t, F, pat)
    d, rows = g.d, g.R + SLACK
    ldh = F + 8 if form == "t16" else F   # (the planar form's SwiGLU rows have no stride argument)
    ldo = d + 4
    b_gu, b_dn = GROUP_BOUNDS[form]
    worst = [0.0, 0.0]
    for e in range(g.E):
        r0, r1 = g.off[e], g.off[e + 1]
        what = (form, "expert", e, "rows", r0, r1)
        h = _filled(torch, (rows, ldh), g.dt, g.nan)
        g.gate_up(e, h, ldh)
        torch.cuda.synchronize()
        hb = _bits(torch, h)
        mr.check_group_untouched(hb, np.full(hb.shape, g.nan, np.uint16), r0, r1, F, what + ("swiglu",))
        if r1 > r0:
            hv = _values(hb[r0:r1, :F], g.kind)
            worst[0] = max(worst[0], mr.check_rows(hv, mr.swiglu_ref(g.xg_ref[r0:r1], g.ex["Wgu"][e]), b_gu,
                                                   what + ("swiglu",)))
        # the down reads rows of stride F: this expert's SwiGLU rows in a buffer that is NaN elsewhere
        hin = _filled(torch, (rows, F), g.dt, g.nan)
        hin[r0:r1] = h[r0:r1, :F]
        y = _filled(torch, (rows, ldo), torch.float32, 0 if F == 1024 else mr.NAN32)
        sent = _bits(torch, y)
        g.down(e, hin, y, ldo)
        torch.cuda.synchronize()
        mr.check_group_untouched(_bits(torch, y), sent, r0, r1, d, what + ("down",))
        if r1 > r0:
            worst[1] = max(worst[1], mr.check_rows(y[r0:r1, :d].cpu().numpy(), mr.down_ref(hv, g.ex["Wd"][e]), b_dn,
                                                   what + ("down",)))
    print(f"MOE_FRAC grouped {form} {t.name} F={F} pat={pat} swiglu {worst[0]:.3f} down {worst[1]:.3f}")


@pytest.mark.parametrize("t,pat", [(Q4_K, 0), (Q4_K, 1), (Q4_K, 2), (Q4_K, 3), (Q6_K, 2)])
@pytest.mark.parametrize("form", ["t16", "dq"])
def test_grouped_ffn_end_to_end(torch, form, t, pat):
    """The chain as the engine runs it - route, gather, every expert's gate/up and down in ascending
    order over shared buffers (row strides F and d, the output zeroed once), scatter-add into a
    random residual - per token row against fp64 of the whole routed FFN; the bound is the sum of
    the stage bounds. The slack rows of both gathered buffers keep their sentinels."""
    F = 1024
    g = _Grouped(torch, form, t, F, pat)
    d, T, k, rows = g.d, g.T, g.k, g.R + SLACK
    h = _filled(torch, (rows, F), g.dt, g.nan)
    y = torch.zeros((rows, d), device="cuda")
    for e in range(g.E):
        g.gate_up(e, h, F)
        g.down(e, h, y, d)
    rng = np.random.default_rng(pat)
    res = rng.standard_normal((T + 1, d)).astype(np.float32)
    acc = torch.from_numpy(res).cuda()
    hip().moe_scatter_add(acc.data_ptr(), y.data_ptr(), g.rt_dev["pos"].data_ptr(), g.rt_dev["gw"].data_ptr(), T, k, d,
                          stream())
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    ref = mr.moe_ffn_ref(g.x_ref, g.ex["Wgu"], g.ex["Wd"], g.rt, k)
    frac = mr.check_rows(got[:T].astype(np.float64) - res[:T], ref, sum(GROUP_BOUNDS[form]), (form, "ffn"))
    print(f"MOE_FRAC grouped_ffn {form} {t.name} pat={pat} {frac:.3f}")
    assert np.array_equal(got[T:], res[T:])
    assert np.all(_bits(torch, h)[g.R:] == g.nan) and np.all(_bits(torch, y)[g.R:] == 0)


# ------------------------------------------------------------------ batched decode experts
def _run_bmm_experts(torch, t, E, d, F, B, folded):
    ex = _experts(t, E, d, F)
    gu, dn, _, _ = _stacked_t16(torch, t, E, d, F)
    rng = np.random.default_rng(B * 100 + F + int(t))
    X = (rng.standard_normal((B, d)) * (3 if folded else 1)).astype(np.float32)
    eps = 1e-5
    if folded:   # fp32 rows, the RMSNorm folded into the staging
        nw = (0.5 + rng.random(d)).astype(np.float32)
        ldxf = d + 4
        dx = torch.zeros(B, ldxf, device="cuda")
        dx[:, :d] = torch.from_numpy(X).cuda()
        dnw = torch.from_numpy(nw).cuda()
        xin = dict(xf=dx.data_ptr(), ldxf=ldxf, norm=dnw.data_ptr(), eps=eps)
        x_ref, xh_ptr = staged_x(X, nw, eps, "folded"), 0
    else:        # f16 rows in the 4-group k order
        dxh = torch.from_numpy(mr.swizzle4(X.astype(np.float16))).cuda()
        xin, x_ref, xh_ptr = {}, staged_x(X, None, eps, "xh"), dxh.data_ptr()
    y0 = rng.standard_normal((B, d)).astype(np.float32)
    ldh, ldo, ew_ld = E * F + 8, d + 4, E + 1
    worst = [0.0, 0.0]
    for name, ew in mr.ew_patterns(B, E, B + F):
        what = (t.name, "F", F, "B", B, name)
        ewp = np.full((B, ew_ld), 5.0, np.float32)   # the pad column is never a weight
        ewp[:, :E] = ew
        dew = torch.from_numpy(ewp).cuda()
        h = _filled(torch, (B, ldh), torch.float16, mr.NAN16)
        hip().bmm(gu.data_ptr(), int(t), E * 2 * F, d, xh_ptr, d, 0, 0, B, stream(), h_out=h.data_ptr(), ldh_out=ldh,
                  ew=dew.data_ptr(), ew_ld=ew_ld, tiles_per_expert=2 * F // 16, **xin)
        out = torch.full((B, ldo), 3.0, device="cuda")
        out[:, :d] = torch.from_numpy(y0).cuda()
        zero = torch.ones(1024, device="cuda")
        zargs = dict(zero=zero.data_ptr(), zero_n=1024) if B <= 8 else {}   # a side job of the wave-owned kernels
        hip().bmm(dn.data_ptr(), int(t), d, E * F, h.data_ptr(), ldh, out.data_ptr(), ldo, B, stream(),
                  ew=dew.data_ptr(), ew_ld=ew_ld, steps_per_expert=F // 256, **zargs)
        torch.cuda.synchronize()
        hb = _bits(torch, h)
        worst[0] = max(worst[0], mr.check_bmm_gu(hb, np.full(hb.shape, mr.NAN16, np.uint16),
                                                 mr.bmm_gu_ref(x_ref, ex["Wgu"], ew), ew, F, what))
        got = out.cpu().numpy()
        assert np.all(np.isfinite(got)), (what, "the down projection read a skipped expert's columns")
        assert np.all(got[:, d:] == 3.0), (what, "pad columns")
        hd = mr.swizzle4(hb[:, :E * F].view(np.float16).astype(np.float64))   # NaN where no expert wrote
        ref = mr.bmm_down_ref(hd, ex["Wd"], ew)
        delta = got[:, :d].astype(np.float64) - y0
        routed = np.any(ew != 0, axis=1)
        assert np.all(delta[~routed] == 0), (what, "a row routed nowhere changed")
        worst[1] = max(worst[1], mr.check_rows(delta[routed], ref[routed], mr.BMM_DN, what + ("down",)))
        if B <= 8:
            assert float(zero.abs().sum()) == 0.0, (what, "zero side job")
    return worst


BMM_CASES = ([(t, F, B) for t in (Q4_K, Q6_K) for F in (1536, 1792) for B in (1, 6, 8, 9, 16)]
             + [(t, 1536, B) for t in (Q5_K, Q8_0) for B in (1,)])


@pytest.mark.parametrize("t,F,B", BMM_CASES)
def test_bmm_stacked_experts(torch, t, F, B):
    """E = 8 experts as ONE gate/up and ONE down launch (d = 256; F / 256 = 6 or 7 steps per expert - 7
    runs the parts-per-expert search to its end; B <= 8: the wave-owned kernels, B > 8: bmm_kernel),
    over five hand-made routings. h_out starts as f16 NaN: routed (row, expert) blocks against
    ew silu(g) u in fp64, unrouted rows of an active expert exactly zero, skipped experts' columns
    and the pad columns still NaN; the down, over the device's own h of the active experts, per row -
    finite everywhere, so no skipped column was read."""
    w = _run_bmm_experts(torch, t, 8, 256, F, B, folded=False)
    print(f"MOE_FRAC bmm_experts {t.name} F={F} B={B} swiglu {w[0]:.3f} down {w[1]:.3f}")


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("B", [1, 6, 8])
def test_bmm_stacked_experts_folded_norm(torch, t, B):
    """The same with the RMSNorm folded into the gate/up staging (fp32 rows, K = 4096): the batched
    step's actual gate/up launch. E = 4, F = 256."""
    assert hip().bmm_norm_fits(4096, B)
    w = _run_bmm_experts(torch, t, 4, 4096, 256, B, folded=True)
    print(f"MOE_FRAC bmm_experts_folded {t.name} B={B} swiglu {w[0]:.3f} down {w[1]:.3f}")


# ------------------------------------------------------------------ single-row decode down
def _moe_down(torch, t, F, rows, n_slots):
    rng = np.random.default_rng(F + rows + n_slots + int(t))
    E = n_slots + 1
    downs = [make_matrix(t, rows, F, rng) for _ in range(E)]
    planar = [to_planar(t, r, rows, F) for r, _ in downs]
    dd = dev_bytes(np.concatenate(planar))
    ids = [(2 * s + 1) % E for s in range(n_slots)]   # distinct (E is odd)
    wts = rng.random(n_slots).astype(np.float32) + 0.1
    wts /= wts.sum()
    h = rng.standard_normal((n_slots, F)).astype(np.float32)
    dh, di, dw = torch.from_numpy(h).cuda(), torch.tensor(ids, dtype=torch.int32, device="cuda"), torch.from_numpy(wts).cuda()
    y = torch.ones(rows + 3, device="cuda")
    hip().moe_down(dd.data_ptr(), int(t), rows, F, planar[0].size, dh.data_ptr(), di.data_ptr(), dw.data_ptr(), n_slots,
                   y.data_ptr(), stream())
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    ref = sum(float(wts[s]) * downs[ids[s]][1].astype(np.float64) @ q8_emulate(h[s]).astype(np.float64)
              for s in range(n_slots))
    assert np.all(got[rows:] == 1.0)
    return rel_err(got[:rows].astype(np.float64) - 1, ref)


@pytest.mark.parametrize("t,F,n_slots", [(Q4_K, 2304, 2), (Q6_K, 2304, 2), (Q8_0, 2304, 2), (Q4_K, 4096, 2),
                                         (Q4_K, 4096, 4)])
def test_moe_down_splitk_parts(torch, t, F, n_slots):
    """The split-K single-row down with more than one 64-chunk K part per slot (F > 2048; every
    engine model has one): F = 2304 - two parts, the second a ragged 8 chunks; F = 4096 - two exact
    parts, with two and four slots. 130 rows: the last 4-row group is partial."""
    e = _moe_down(torch, t, F, 130, n_slots)
    print(f"MOE_FRAC moe_down_splitk {t.name} F={F} slots={n_slots} {e / 1e-3:.2e}")
    assert e < 1e-3, e


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_moe_down_per_slot_kquants(torch, t):
    """The per-slot kernel's K-quant instantiations: n_slots F = 66560 is past the split-K form's
    65536 activation bytes, so gemv_moe_down falls through to it."""
    e = _moe_down(torch, t, 16640, 64, 4)
    print(f"MOE_FRAC moe_down_per_slot {t.name} {e / 1e-3:.2e}")
    assert e < 1e-3, e
