"""fp64 reference and checkers of the MoE expert paths: the prefill routing (softmax, top-k, the
per-expert row lists of the grouped GEMMs), the expert FFN stages, the batched decode step's stacked
experts, and the checks that judge a kernel's output against them - every row by itself, and every
byte outside the written region against the sentinel it held. Needs no GPU, so the checkers have a
CPU self-test (test_moe_ref.py) that plants single defects and shows each one rejected."""
import numpy as np

# bounds on one row against fp64 of the same 2-byte inputs: the dense tests' bounds of the same kernels
# (test_gemm_t16_swiglu_vs_fp32 / test_gemm_t16_vs_fp32, test_gemm_swiglu / test_gemm_mfma,
# test_bmm_swiglu_epilogue_vs_fp32 / test_bmm_rows_vs_fp32)
T16_GU, T16_DN = 3e-3, 2e-3
DQ_GU, DQ_DN = 1e-2, 5e-3
BMM_GU, BMM_DN = 3e-3, 2e-3
# the router bound of test_moe_router_rows_vs_fp64
GW_RTOL, GW_ATOL = 1e-4, 1e-6
# routing precondition: neighbouring probabilities among a token's top k + 1 are exactly equal (a
# deliberate tie, resolved to the lowest index) or differ by this much, relative - far above the f32
# softmax's rounding (~1e-6), so the device's picks are the reference's
MARGIN = 1e-3

NAN16 = 0x7EAB    # f16 quiet NaN with a payload
NANBF = 0x7FAB    # bf16 quiet NaN with a payload
NAN32 = 0x7FC00ABC


def swizzle4(x):
    """The batched kernels' k order inside each 4-group: (0, 2, 1, 3). Its own inverse."""
    x = np.asarray(x)
    return x.reshape(*x.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(x.shape)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---------------------------------------------------------------------------- routing
class Routing:
    """sel / selw [T][k]: each token's picks in rank order and their renormalised weights; cnt_off
    [E + 1]: first gathered row of each expert (cnt_off[E] = T k); tok / gw [T k]: gathered row ->
    token / routing weight, each expert's rows in ascending token order; pos [T k]: token slot
    t k + j -> its gathered row."""

    def __init__(self, sel, selw, cnt_off, tok, gw, pos):
        self.sel, self.selw, self.cnt_off, self.tok, self.gw, self.pos = sel, selw, cnt_off, tok, gw, pos


def softmax64(logits):
    lg = np.asarray(logits, np.float32).astype(np.float64)
    p = np.exp(lg - lg.max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


def route_reference(logits, k, tie_high=False):
    """tie_high: resolve ties to the HIGHEST index (the planted defect of the self-test)."""
    p = softmax64(logits)
    T, E = p.shape
    if tie_high:
        sel = (E - 1 - np.argsort(-p[:, ::-1], axis=1, kind="stable"))[:, :k]
    else:
        sel = np.argsort(-p, axis=1, kind="stable")[:, :k]
    w = np.take_along_axis(p, sel, 1)
    selw = w / w.sum(1, keepdims=True)
    flat = sel.reshape(-1)
    cnt = np.bincount(flat, minlength=E)
    cnt_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    order = np.argsort(flat, kind="stable")      # per expert, ascending slot = ascending token
    tok = order // k
    gw = selw.reshape(-1)[order]
    pos = np.empty(T * k, np.int64)
    pos[order] = np.arange(T * k)
    return Routing(sel, selw, cnt_off, tok, gw, pos)


def route_margin(logits, k):
    """The smallest relative gap between neighbouring probabilities among any token's top k + 1,
    exact ties of the logits left out (the precondition asks it to be >= MARGIN)."""
    lg = np.asarray(logits, np.float32)
    p = softmax64(lg)
    order = np.argsort(-p, axis=1, kind="stable")
    ps = np.take_along_axis(p, order, 1)
    ls = np.take_along_axis(lg, order, 1)
    n = min(k + 1, p.shape[1])
    gap = (ps[:, :n - 1] - ps[:, 1:n]) / ps[:, :n - 1]
    gap = np.where(ls[:, :n - 1] == ls[:, 1:n], np.inf, gap)
    return float(gap.min()) if gap.size else float("inf")


def routing_logits(T, E, k, kind, seed):
    """The routing inputs of the GPU tests (f32 [T][E]). kind: "random" - normal logits, with rows of
    exactly equal logits where T allows (row 3: all equal, so the picks are experts 0 .. k - 1; row 5:
    its two largest equal; row 6: the k-th and (k + 1)-th equal); "empty" - expert 1 far below the
    rest on every row, so its group is empty; "one" - expert E - 2 far above on every row, so it gets
    every token. Rows that miss the margin precondition are redrawn."""
    rng = np.random.default_rng(seed)
    if kind not in ROUTE_KINDS:
        raise ValueError(kind)

    def pin(row):
        if kind == "empty":
            row[1] = -30.0
        elif kind == "one":
            row[E - 2] = 12.0
        return row

    lg = np.empty((T, E), np.float32)
    for t in range(T):
        lg[t] = pin((2.0 * rng.standard_normal(E)).astype(np.float32))
        while route_margin(lg[t:t + 1], k) < 4 * MARGIN:
            lg[t] = pin((2.0 * rng.standard_normal(E)).astype(np.float32))
    if kind == "random":   # (a value raised to its upper neighbour's: the other gaps only grow)
        if T > 3:
            lg[3, :] = np.float32(0.25)
        if T > 5:
            o = np.argsort(-lg[5], kind="stable")
            lg[5, o[1]] = lg[5, o[0]]
        if T > 6 and k < E:
            o = np.argsort(-lg[6], kind="stable")
            lg[6, o[k]] = lg[6, o[k - 1]]
    return lg


ROUTE_KINDS = ["random", "empty", "one"]
ROUTE_SHAPES = [(1, 4, 2), (40, 4, 2), (257, 8, 2), (300, 8, 2), (33, 64, 8), (17, 8, 1)]
ROUTE_CASES = [(T, E, k, kind) for T, E, k in ROUTE_SHAPES for kind in ROUTE_KINDS]


def route_seed(T, E, k, kind):
    return 1000 * T + 10 * E + k + 7 * ROUTE_KINDS.index(kind)


# the grouped GEMM tests' rows per expert (E = 4, k = 2): T -> counts
GROUP_PATTERNS = [(40, (40, 0, 17, 23)), (100, (0, 100, 64, 36)), (300, (129, 171, 300, 0)),
                  (300, (65, 128, 107, 300))]


def logits_for_counts(T, counts, seed):
    """Logits whose top-2 routing gives expert e exactly counts[e] rows (sum = 2 T, each <= T): every
    token takes the two experts with the most rows left; the tokens are then shuffled and which of
    the two ranks first is drawn per token."""
    E = len(counts)
    left = np.array(counts, np.int64)
    assert left.sum() == 2 * T and left.max() <= T
    picks = np.zeros((T, 2), np.int64)
    for t in range(T):
        top = np.argsort(-left, kind="stable")[:2]
        assert np.all(left[top] > 0)
        left[top] -= 1
        picks[t] = top
    rng = np.random.default_rng(seed)
    picks = picks[rng.permutation(T)]
    flip = rng.random(T) < 0.5
    lg = (-4.0 + 0.1 * rng.standard_normal((T, E))).astype(np.float32)
    lg[np.arange(T), np.where(flip, picks[:, 1], picks[:, 0])] = np.float32(4.0)
    lg[np.arange(T), np.where(flip, picks[:, 0], picks[:, 1])] = np.float32(3.0)
    return lg


def check_routing(got, ref, T, E, k):
    """got: dict of the device arrays sel, selw, cnt_off, tok, gw, pos."""
    for name in ("sel", "cnt_off", "tok", "pos"):
        g, r = np.asarray(got[name]).reshape(-1), np.asarray(getattr(ref, name)).reshape(-1)
        bad = np.flatnonzero(g != r)
        assert bad.size == 0, (name, "first mismatch at", int(bad[0]), int(g[bad[0]]), int(r[bad[0]]))
    np.testing.assert_allclose(np.asarray(got["selw"]).reshape(T, k), ref.selw, rtol=GW_RTOL, atol=GW_ATOL)
    np.testing.assert_allclose(np.asarray(got["gw"]).reshape(-1), ref.gw, rtol=GW_RTOL, atol=GW_ATOL)


# ---------------------------------------------------------------------------- checkers
def row_errors(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-30)


def check_rows(got, ref, bound, what=""):
    """Relative error of every row by itself (not one norm over the array: a single wrong row among
    hundreds must fail). Returns the worst row's error as a fraction of the bound."""
    got = np.asarray(got, np.float64)
    assert got.shape == np.asarray(ref).shape, (what, got.shape, np.asarray(ref).shape)
    if got.size == 0:
        return 0.0
    assert np.all(np.isfinite(got)), (what, "non-finite, first row", int(np.argwhere(~np.isfinite(got))[0][0]))
    e = row_errors(got, ref)
    i = int(np.argmax(e))
    assert e[i] < bound, (what, "row", i, "error", float(e[i]), "bound", bound)
    return float(e[i] / bound)


def check_untouched(got, sentinel, written, what=""):
    """Every element outside the boolean mask `written` is bit-identical to the sentinel; names the
    first touched element."""
    bad = (bits(got) != bits(sentinel)) & ~written
    assert not bad.any(), (what, "touched outside the written region, first at",
                           tuple(int(x) for x in np.argwhere(bad)[0]))


def check_group_untouched(got, sentinel, r0, r1, ncol, what=""):
    """A grouped launch may write rows [r0, r1), columns [0, ncol) of got [rows][ld] and nothing else:
    not the other groups' rows, not the slack rows past the last group, not the pad columns."""
    written = np.zeros(got.shape, bool)
    written[r0:r1, :ncol] = True
    check_untouched(got, sentinel, written, what)


def scatter_bound(acc0, terms):
    """Per element bound of acc0 + sum_j terms[j] summed in fp32, with or without fma contraction:
    (k + 1) 2^-23 (|acc0| + sum_j |terms[j]|). terms: [k][...] fp64 products gw_j y_j."""
    k = terms.shape[0]
    return (k + 1) * 2.0 ** -23 * (np.abs(acc0) + np.abs(terms).sum(0))


# ---------------------------------------------------------------------------- expert FFN
def silu_mul(g, u):
    return g / (1.0 + np.exp(-g)) * u


def swiglu_ref(x, Wgu):
    """x [n][d]; Wgu [2F][d], gate / up rows in 32-row groups -> silu(gate) * up [n][F], fp64."""
    pre = np.asarray(x, np.float64) @ np.asarray(Wgu, np.float64).T
    n, F = pre.shape[0], pre.shape[1] // 2
    pre = pre.reshape(n, F // 32, 2, 32)
    return silu_mul(pre[:, :, 0].reshape(n, F), pre[:, :, 1].reshape(n, F))


def down_ref(h, Wd):
    return np.asarray(h, np.float64) @ np.asarray(Wd, np.float64).T


def moe_ffn_ref(x, Wgu, Wd, routing, k):
    """The whole routed FFN of token rows x [T][d] in fp64: sum_j selw[t][j] down(swiglu(x_t))."""
    x = np.asarray(x, np.float64)
    out = np.zeros((x.shape[0], Wd[0].shape[0]))
    for e in range(len(Wgu)):
        for j in range(k):
            rows = np.flatnonzero(routing.sel[:, j] == e)
            if rows.size:
                out[rows] += routing.selw[rows, j][:, None] * down_ref(swiglu_ref(x[rows], Wgu[e]), Wd[e])
    return out


# ---------------------------------------------------------------------------- batched decode experts
def ew_patterns(B, E, seed):
    """The hand-made routing weight rows [B][E] of the batched tests (name, ew)."""
    rng = np.random.default_rng(seed)
    out = []
    ew = np.zeros((B, E), np.float32)
    for b in range(B):
        e = rng.choice(E, 2, replace=False)
        w = 0.2 + 0.6 * rng.random()
        ew[b, e[0]], ew[b, e[1]] = w, 1 - w
    out.append(("top2", ew))
    ew = np.zeros((B, E), np.float32)
    ew[:, 2], ew[:, E - 3] = 0.625, 0.375
    out.append(("same2", ew))
    ew = np.zeros((B, E), np.float32)
    for b in range(B):   # every expert routed by some row; with B < E/2 rows, by wider rows
        for e in range(E):
            if e % B == b or (e + 1) % B == b:
                ew[b, e] = 0.1 + 0.05 * e
    out.append(("all", ew))
    ew = np.zeros((B, E), np.float32)
    ew[:, 0] = 1.0
    out.append(("first", ew))
    ew = np.zeros((B, E), np.float32)
    ew[:, E - 1] = 1.0
    if B > 1:
        ew[B - 1, E - 1] = 0.0   # a row routed nowhere under the active expert
        ew[0, E - 1] = 0.5
    out.append(("last", ew))
    return out


def bmm_gu_ref(x, Wgu, ew):
    """Stacked gate/up: h [B][E F] = ew[b][e] silu(g) u of expert e's features (un-swizzled), fp64;
    columns of experts no row routes to are NaN (the kernel never writes them)."""
    B, E = ew.shape
    F = Wgu[0].shape[0] // 2
    h = np.full((B, E * F), np.nan)
    for e in range(E):
        if np.any(ew[:, e] != 0):
            h[:, e * F:(e + 1) * F] = ew[:, e:e + 1].astype(np.float64) * swiglu_ref(x, Wgu[e])
    return h


def bmm_down_ref(h, Wd, ew, part=None):
    """K-concatenated down over h [B][E F] of the active experts only. part = (e, c0, c1): the planted
    defect - columns [c0, c1) of expert e multiplied by the next expert's weights."""
    B, E = ew.shape
    F = Wd[0].shape[1]
    out = np.zeros((B, Wd[0].shape[0]))
    for e in range(E):
        if np.any(ew[:, e] != 0):
            W = np.asarray(Wd[e], np.float64)
            if part is not None and part[0] == e:
                W = W.copy()
                W[:, part[1]:part[2]] = np.asarray(Wd[(e + 1) % E], np.float64)[:, part[1]:part[2]]
            out += np.asarray(h[:, e * F:(e + 1) * F], np.float64) @ W.T
    return out


def check_bmm_gu(got_bits, sentinel_bits, ref, ew, F, what=""):
    """got_bits / sentinel_bits: uint16 [B][ld] (f16, the kernels' 4-group k order); ref from
    bmm_gu_ref. Returns the worst routed block's error as a fraction of BMM_GU."""
    B, E = ew.shape
    got = got_bits.view(np.float16)
    written = np.zeros(got_bits.shape, bool)
    worst = 0.0
    for e in range(E):
        c = slice(e * F, (e + 1) * F)
        if not np.any(ew[:, e] != 0):
            continue   # stays the sentinel: checked below
        written[:, c] = True
        for b in range(B):
            blk = got[b, c].astype(np.float64)
            if ew[b, e] == 0:
                assert np.all(blk == 0), (what, "row", b, "expert", e, "unrouted block is not zero")
            else:
                worst = max(worst, check_rows(swizzle4(blk)[None], ref[b:b + 1, c], BMM_GU, (what, "row", b, "expert", e)))
    check_untouched(got_bits, sentinel_bits, written, (what, "h_out"))
    return worst
