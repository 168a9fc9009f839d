"""Reference, bound, checker and kernel emulation for the embedding epilogue
(csrc/kernels/misc.hip: pool_rows / pool_finish; kernels.h PoolArgs).

  * ``reference``  - the epilogue in fp64 over arbitrary segment tables: output RMSNorm of every row,
                     pooling per input over the launches of one call, optional L2 normalisation;
                     with it the bound of every output element.
  * ``check``      - a result against that reference, element by element; returns worst error / bound.
  * ``emulate``    - the kernels' arithmetic in fp32 in their own order of additions (groups of 64
                     rows, rows in row order, groups in group order, the accumulator carried from
                     launch to launch), with single defects that can be planted to show ``check``
                     rejects them.
  * ``make_case``  - the GPU test's inputs, shared so the emulation is held to the bound over exactly
                     those inputs (tests/test_pool_ref.py).

A launch is ``(x, segs)``: fp32 rows ``x[rows][ldx]`` and a table of ``(first row, rows, input,
flags, tokens of the whole input)`` with flags FIRST | LAST (the input's first / last piece).

The bound (u = 2^-24, the unit roundoff of fp32; every count is a first-order count, the factor
1.01 covers the higher-order terms, which are below 1e-4 of it at these counts):

  scale of a row, s = rsqrt(sum(x^2) / d + eps). A lane adds ceil(d / 256) float4 groups (three
      additions inside a group, one onto the running sum), six butterfly levels follow, every square
      is rounded once: the sum of squares (all terms positive) has relative error at most
      A u, A = ceil(d / 256) + 3 + 6 + 1. The division by d and the addition of eps add 1 u each, the
      inverse square root halves what it is given and adds its own error, at most 2 ulp = 4 u:
      C_SCALE(d) = (A + 2) / 2 + 4.
  one term t_rc = s_r x_rc w_c: the product with s (or the fused multiply-add that absorbs it) and
      the product with w round once each: C_SCALE + 2. For ``mean`` the reciprocal 1 / n_tokens and
      the multiplication by it add 2 more.
  mean, before L2:   |out_c - ref_c| <= 1.01 (chain + c) u mean_r |t_rc|,  c = C_SCALE(d) + 4,
      chain = the longest chain of sequential additions one element sees = the rows of the
      largest group (at most 64) + the number of groups of the input over all its pieces
      (sequential summation of k terms: error at most (k - 1) u sum |t|, at both levels).
  cls / last / none: |out_c - ref_c| <= 1.01 c1 u |t_c|,  c1 = C_SCALE(d) + 2 (no sum at all: the
      additions onto zero and the multiplication by 1.0 are exact).
  L2-normalised, y = v / ||v|| with v bounded elementwise by b as above: the norm moves by at most
      ||b||_2; the fp32 sum of squares of v has relative error at most A2 u, A2 = ceil(d / 256) + 13
      (a block's threads add ceil(d / 1024) float4 groups, six butterfly levels, three additions over
      the waves; a wave of ``none`` adds ceil(d / 256) groups and six levels; one rounding per
      square), its inverse square root A2 / 2 + 4, the final product 1:
      |y_c - ref_c| <= 1.01 (b_c / ||v|| + |y_c| (||b||_2 / ||v|| + (A2 / 2 + 5) u)).
"""
import math

import numpy as np

SEG_INTS = 5
FIRST, LAST = 1, 2
GROUP = 64
NONE, MEAN, CLS, LAST_MODE = 0, 1, 2, 3
MODES = {"none": NONE, "mean": MEAN, "cls": CLS, "last": LAST_MODE}
U = 2.0 ** -24

DS = (64, 288, 2048, 4096, 8192)
# d = 288: eps is half of every row's mean square (its rows have mean square 1), so a kernel
# that leaves eps out is 22 % off there; the others use the models' values
EPS = {64: 1e-5, 288: 0.5, 2048: 1e-6, 4096: 1e-5, 8192: 1e-5}
CASES = ("five", "three", "carry")


def c_scale(d: int) -> float:
    return (math.ceil(d / 256) + 3 + 6 + 1 + 2) / 2 + 4


def c_l2(d: int) -> float:
    return (math.ceil(d / 256) + 13) / 2 + 5


def groups_of(n: int) -> int:
    return (n + GROUP - 1) // GROUP


def make_case(name: str, d: int, guard: bool = True, seed: int = 0):
    """The inputs of one GPU test case: {"launches": [(x [rows][ldx] fp32, segs)], "w", "eps", "d",
    "n_inputs"}. Behind every segment lies a guard row (NaN when ``guard``, else ordinary values
    that belong to no input); the padding columns of a row (ldx > d) are NaN likewise.
      five  - one launch, five inputs of 1, 63, 64, 65 and 130 rows (n_tokens = 1 among them)
      three - one launch, three segments (65, 1, 130 rows) that start at row 3
      carry - two launches: input 0 arrives as 70 + 60 rows and input 1 as 40 + 30 rows, input 1's
              pieces lying between input 0's; the accumulator rows carry both over
    """
    rng = np.random.default_rng(100003 * seed + 17 * d + CASES.index(name))
    ldx = d + 8 if d in (64, 2048) else d

    def rows(n):
        x = rng.standard_normal((n, ldx)).astype(np.float32)
        if d != 288:   # row magnitudes over two decades: the scales matter
            x *= np.exp(rng.uniform(-2.3, 2.3, (n, 1))).astype(np.float32)
        else:          # mean square 1 exactly enough for EPS[288] to be half of it
            x[:, :d] /= np.sqrt((x[:, :d].astype(np.float64) ** 2).mean(-1, keepdims=True)).astype(np.float32)
        if ldx > d:
            x[:, d:] = np.nan if guard else 7.0
        return x

    def layout(lengths, start):
        segs, row = [], start
        for n in lengths:
            segs.append([row, n])
            row += n + 1          # a guard row behind each segment
        x = rows(row)
        if guard:
            used = np.zeros(row, bool)
            for r0, n in segs:
                used[r0:r0 + n] = True
            x[~used] = np.nan
        return x, segs

    if name == "five":
        x, sg = layout((1, 63, 64, 65, 130), 0)
        launches = [(x, [(r0, n, i, FIRST | LAST, n) for i, (r0, n) in enumerate(sg)])]
        n_inputs = 5
    elif name == "three":
        x, sg = layout((65, 1, 130), 3)
        launches = [(x, [(r0, n, i, FIRST | LAST, n) for i, (r0, n) in enumerate(sg)])]
        n_inputs = 3
    elif name == "carry":
        x1, s1 = layout((70, 40), 1)
        x2, s2 = layout((30, 60), 2)
        launches = [(x1, [(s1[0][0], 70, 0, FIRST, 130), (s1[1][0], 40, 1, FIRST, 70)]),
                    (x2, [(s2[0][0], 30, 1, LAST, 70), (s2[1][0], 60, 0, LAST, 130)])]
        n_inputs = 2
    else:
        raise ValueError(name)
    w = rng.uniform(0.5, 1.5, d).astype(np.float32)
    return {"launches": launches, "w": w, "eps": EPS[d], "d": d, "n_inputs": n_inputs}


def _l2(v, b, d):
    """(y, its bound) of v / ||v|| for v bounded elementwise by b (module docstring)."""
    nv = np.sqrt((v * v).sum(-1, keepdims=True))
    y = v / nv
    by = 1.01 * (b / nv + np.abs(y) * (np.sqrt((b * b).sum(-1, keepdims=True)) / nv + c_l2(d) * U))
    return y, by


def reference(case, mode: int, normalize: bool):
    """fp64: {key: (value, bound)} with key = the input index, or for ``none`` (launch, row)."""
    d, w, eps = case["d"], case["w"].astype(np.float64), float(case["eps"])
    cs = c_scale(d)
    out = {}
    terms = {}     # input -> list of t_rc blocks over its pieces
    pieces = {}    # input -> list of piece lengths
    total = {}
    for li, (x, segs) in enumerate(case["launches"]):
        for (r0, n, dst, flags, n_tok) in segs:
            xr = x[r0:r0 + n, :d].astype(np.float64)
            s = 1.0 / np.sqrt((xr * xr).mean(-1, keepdims=True) + eps)
            t = s * xr * w
            total[dst] = n_tok
            if mode == NONE:
                for r in range(n):
                    v, b = t[r], 1.01 * (cs + 2) * U * np.abs(t[r])
                    out[(li, r0 + r)] = _l2(v, b, d) if normalize else (v, b)
                continue
            if flags & FIRST:
                terms[dst], pieces[dst] = [], []
            terms[dst].append((t, flags))
            pieces[dst].append(n)
    if mode == NONE:
        return out
    for dst, blocks in terms.items():
        if not (blocks[-1][1] & LAST):
            continue
        t = np.concatenate([b for b, _ in blocks])
        assert t.shape[0] == total[dst], "reference: the pieces do not add up to the input"
        if mode == MEAN:
            chain = min(GROUP, max(pieces[dst])) + sum(groups_of(n) for n in pieces[dst])
            v = t.mean(0)
            b = 1.01 * (chain + cs + 4) * U * np.abs(t).mean(0)
        else:
            v = t[0] if mode == CLS else t[-1]
            b = 1.01 * (cs + 2) * U * np.abs(v)
        out[dst] = _l2(v, b, d) if normalize else (v, b)
    return out


def check(got, ref) -> float:
    """Assert every element of ``got`` ({key: vector}) within its bound of ``ref`` (``reference``'s
    result); the keys must be the same. Returns the worst error / bound."""
    assert set(got) == set(ref), f"results for {sorted(got, key=str)} but reference for {sorted(ref, key=str)}"
    worst = 0.0
    for k, (v, b) in ref.items():
        g = np.asarray(got[k], np.float64)
        assert g.shape == v.shape, f"{k}: shape {g.shape}"
        assert np.isfinite(g).all(), f"{k}: non-finite output"
        ratio = np.abs(g - v) / np.maximum(b, 1e-300)
        i = int(ratio.argmax())
        assert ratio[i] <= 1.0, f"{k}: element {i}: {g[i]!r} vs {v[i]!r}, error {abs(g[i] - v[i]):.3g} > bound {b[i]:.3g}"
        worst = max(worst, float(ratio[i]))
    return worst


DEFECTS = ("drop_last_row", "group_twice", "neighbour_row", "div_chunk_rows", "no_eps", "no_weight",
           "l2_before_mean", "last_chunk_row", "no_carry")


def emulate(case, mode: int, normalize: bool, defect: str = None):
    """The kernels' arithmetic in fp32, in their order of additions -> {key: vector}. ``defect``
    plants one error (DEFECTS)."""
    f32 = np.float32
    d, w = case["d"], case["w"].astype(f32)
    eps = f32(0 if defect == "no_eps" else case["eps"])
    if defect == "no_weight":
        w = np.ones_like(w)
    acc, out = {}, {}

    def scale(xr):
        ss = (xr * xr).astype(f32).sum(-1, dtype=f32)
        return (f32(1) / np.sqrt((ss / f32(d) + eps).astype(f32))).astype(f32)

    def l2(v):
        ss = (v * v).astype(f32).sum(-1, keepdims=True, dtype=f32)
        return (v * (f32(1) / np.sqrt(ss)).astype(f32)).astype(f32)

    for li, (x, segs) in enumerate(case["launches"]):
        for (r0, n, dst, flags, n_tok) in segs:
            rows_i = list(range(r0, r0 + n))
            if mode == NONE:
                xr = x[rows_i, :d]
                y = ((scale(xr)[:, None] * xr).astype(f32) * w).astype(f32)
                if normalize:
                    y = l2(y)
                for j, r in enumerate(rows_i):
                    out[(li, r)] = y[j]
                continue
            parts = []
            if mode == MEAN:
                if defect == "neighbour_row":
                    # (a guard row lies between two segments)
                    rows_i.append(r0 + n + 1 if r0 + n + 1 < x.shape[0] else r0 - 2)
                for g0 in range(0, len(rows_i), GROUP):
                    grp = rows_i[g0:g0 + GROUP]
                    if defect == "drop_last_row" and len(grp) > 1:
                        grp = grp[:-1]
                    a = np.zeros(d, f32)
                    for r in grp:   # row order
                        xr = x[r, :d]
                        t = (scale(xr[None])[0] * xr).astype(f32)
                        if defect == "l2_before_mean":
                            t = (l2((t * w).astype(f32)) / w).astype(f32)
                        a = (a + t).astype(f32)
                    parts.append((a * w).astype(f32))
                if defect == "group_twice":
                    parts.append(parts[0])
            elif flags & (FIRST if mode == CLS else LAST):
                r = r0 if mode == CLS else r0 + n - 1
                if defect == "last_chunk_row" and mode == LAST_MODE:
                    r = x.shape[0] - 1
                xr = x[r, :d]
                parts.append(((scale(xr[None])[0] * xr).astype(f32) * w).astype(f32))
            a = np.zeros(d, f32) if (flags & FIRST) or defect == "no_carry" else acc[dst]
            for p in parts:         # group order
                a = (a + p).astype(f32)
            acc[dst] = a
            if flags & LAST:
                inv = f32(1) / f32(n if defect == "div_chunk_rows" else n_tok) if mode == MEAN else f32(1)
                v = (a * inv).astype(f32)
                out[dst] = l2(v) if normalize and defect != "l2_before_mean" else v
    return out
