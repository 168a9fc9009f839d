"""fp64 reference, launch-plan mirror and checkers of the batched decode step's dense FFN chains:
bmm_ffn_chain (SwiGLU gate/up + down in one launch, the down blocks waiting per K part on counters of
the gate/up tiles they read) and bmm_wo_ffn_chain (Wo in front). Needs no GPU, so the checkers have
a CPU self-test (test_ffn_chain_ref.py) that plants single defects and shows each one rejected.

The stages are judged one by one, every row by itself:

  h     the f16 SwiGLU rows the kernel wrote, against silu(g) * u in fp64 of the staged x (f16 rows, or
        the folded norm f16(x * w) * rsqrt(mean(x^2) + eps)), at H_BOUND;
  down  out - resid against the fp64 down projection of the f16 h THAT THE KERNEL WROTE, read back -
        so its bound is the down projection's own (DN_BOUND), not a compound of both stages;
  guard the rows past B of h and out keep their sentinel bits.

The Wo chain's final rows hold resid0 + Wo + down; its staged rows are norm(resid0 + Wo), so they
carry Wo's error: relative delta_b = DN_BOUND |Wo_b| / |resid0_b + Wo_b| per row. The norm is
scale-free and gate and up are linear in x, so a relative delta of x moves g and u by delta each;
|d silu(g) / dg| <= 1.1, so silu(g) u moves by at most (1.1 + 1) delta to first order, rounded up
to WO_H_FACTOR = 2.2: h's bound is H_BOUND + 2.2 delta_b. test_ffn_chain_ref.py perturbs Wo by a random
relative DN_BOUND and finds h moved by less than half of that bound."""
import numpy as np

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from gpu_helpers import make_matrix
from moe_ref import BMM_DN, BMM_GU, NAN16, check_rows, check_untouched, down_ref, silu_mul, swiglu_ref, swizzle4
from qkv_ref import staged_x

# test_bmm_swiglu_epilogue_vs_fp32's and test_bmm_rows_vs_fp32's bounds on one row
H_BOUND, DN_BOUND = BMM_GU, BMM_DN
WO_H_FACTOR = 2.2
EPS = 1e-5
# the counters' layout (kernels.h): parts 0 .. 14 of the down, the last part's counters count the
# gate/up blocks that staged their x, the one before it the finished Wo blocks (bmm_wo_ffn_chain)
MAX_PARTS = 16
STAGED_PART, WO_PART = MAX_PARTS - 1, MAX_PARTS - 2

Q4_K, Q6_K, Q4_0, Q4_1 = GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q4_0, GGMLType.Q4_1


# ---------------------------------------------------------------------------- the launch plan
class ChainPlan:
    """kparts K parts of spp 256-feature steps (the last one shorter when ragged); part_steps /
    part_tiles [kparts]: each part's steps and the gate/up tiles (8 features each) its counter must
    reach; n1: gate/up blocks (one counts itself in the staged part's counter each); n2: blocks of
    the split-K role itself."""

    def __init__(self, kparts, spp, part_steps, n1, n2):
        self.kparts, self.spp, self.part_steps, self.n1, self.n2 = kparts, spp, part_steps, n1, n2
        self.part_tiles = [32 * s for s in part_steps]

    @property
    def ragged(self):
        return self.part_steps[-1] != self.spp


def chain_plan(F, d, cus):
    """The split-K rule of the wave-owned launches (bmm.hip, wt_config) for a d x F projection over
    B <= 8 rows: one 8-wave block per CU, parts = CUs x 8 waves / tiles, at least 2 steps per part."""
    tiles, steps = d // 16, F // 256
    kparts0 = max(1, min(steps // 2, (8 * cus + tiles // 2) // tiles))
    spp = -(-steps // kparts0)
    kparts = -(-steps // spp)
    part_steps = [min(spp, steps - kp * spp) for kp in range(kparts)]
    groups = max(1, min(max(1, cus // kparts), (tiles + 7) // 8))
    return ChainPlan(kparts, spp, part_steps, min(cus, F // 8), groups * kparts)


def chain_takes(plan):
    """bmm_ffn_chain's counters hold the plan (bmm_ffn_chain_supported's part-count condition)."""
    return plan.kparts <= STAGED_PART


def wo_chain_takes(wo_plan, dn_plan):
    return wo_plan.kparts >= 2 and 2 <= dn_plan.kparts <= WO_PART


def counters_per_part(cnt, stride, xcds):
    """The launch's counters [MAX_PARTS][xcds shards][stride ints, the first one used] -> sums per part."""
    c = np.asarray(cnt).reshape(MAX_PARTS, xcds, stride)
    assert not c[:, :, 1:].any(), "a counter line's padding was written"
    return c[:, :, 0].sum(1)


def check_counters(per_part, plan, wo_blocks=None, what=""):
    """Every part counted exactly its producer tiles, the parts past kparts nothing, the staged part
    one per gate/up block (and, the Wo chain, the Wo part one per Wo block)."""
    per_part = [int(v) for v in per_part]
    want = plan.part_tiles + [0] * (MAX_PARTS - plan.kparts)
    want[STAGED_PART] = plan.n1
    if wo_blocks is not None:
        want[WO_PART] = wo_blocks
    assert per_part == want, (what, "counters", per_part, "plan", want)


# ---------------------------------------------------------------------------- inputs
# (K = d, F, folded norm): the bmm_ffn_chain cases; part counts at 256 CUs
CHAIN_SHAPES = [
    (512, 512, False),     # 2 steps: 1 part (the tiny models' only case)
    (512, 1280, False),    # 5: 3, 2
    (512, 3328, False),    # 13: 3, 3, 3, 3, 1
    (512, 7936, False),    # 31: 3 x 10, 1
    (512, 7680, False),    # 30: 2 x 15, the most the counters hold
    (4096, 1280, True),    # 5: 3, 2
    (4096, 2816, True),    # 11: 3, 3, 3, 2
    (4096, 2816, False),
]
TR_SHAPES = [(512, 1280, False), (512, 3328, False)]   # both orientations of the down's epilogue
ROWS = [1, 5, 8]
# (gate/up type, down type, K, F, norm, B, tr; tr -1 = the process default)
CHAIN_CASES = ([(Q4_K, td, K, F, norm, B, tr) for K, F, norm in CHAIN_SHAPES for td in (Q4_K, Q6_K) for B in ROWS
                for tr in ((0, 1) if (K, F, norm) in TR_SHAPES else (-1,))]
               + [(Q4_0, Q4_1, 512, 3328, False, 5, -1), (Q4_1, Q4_0, 512, 3328, False, 5, -1)])
# one per orientation with the down's zero side job
ZERO_CASES = [(Q4_K, Q4_K, 512, 3328, False, 5, 0), (Q4_K, Q6_K, 512, 7936, False, 8, 1)]
# shapes the counters do not hold: the predicate is false, the launcher refuses (K = d, F)
CHAIN_REFUSED = [(512, 8192)]      # 32 steps: 16 parts of 2
# bmm_wo_ffn_chain: (down type, F, Kwo, B), K = 4096 with the folded norm
WO_CASES = [(td, F, Kwo, B) for td in (Q4_K, Q6_K) for F in (1280, 2816) for Kwo in (1024, 4096) for B in (1, 6)]
WO_REFUSED = [(512, 4096)]         # (F, Kwo): a one-part down

_W = {}


def weights(t, R, C, tag):
    """Random blocks of type t for an R x C matrix: (ggml bytes, dequantised fp32). Made once."""
    key = (int(t), R, C, tag)
    if key not in _W:
        rng = np.random.default_rng(7919 * int(t) + 31 * R + C + sum(map(ord, tag)))
        _W[key] = make_matrix(t, R, C, rng)
    return _W[key]


def forget_weights():
    _W.clear()


def chain_rows(K, B, norm, seed):
    """The activation rows X [B][K] (f32; three times as wide under the norm, whose scale is then far
    from 1), the norm weights and the residual rows out starts from (one guard row more)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((B, K)) * (3 if norm else 1)).astype(np.float32)
    nw = (0.5 + rng.random(K)).astype(np.float32)
    resid = rng.standard_normal((B + 1, K)).astype(np.float32)
    return X, nw, resid


def h_reference(X, nw, Wgu, norm, eps=EPS):
    """silu(gate) * up [B][F] in fp64 of the staged rows, features in their natural order."""
    return swiglu_ref(staged_x(X, nw, eps, "folded" if norm else "xh"), Wgu)


def h_values(h_bits):
    """uint16 bits of the kernel's f16 h (its 4-group k order) -> fp64, natural feature order."""
    return swizzle4(np.ascontiguousarray(h_bits).view(np.float16).astype(np.float64))


def h_bits_of(h):
    """fp64 rows -> the bits the kernel would write (f16, 4-group k order)."""
    return swizzle4(np.asarray(h).astype(np.float16)).view(np.uint16)


# ---------------------------------------------------------------------------- checkers
def _guard(h_bits, out, resid, B, what):
    hb = np.asarray(h_bits)
    written = np.zeros(hb.shape, bool)
    written[:B] = True
    check_untouched(hb, np.full(hb.shape, NAN16, np.uint16), written, (what, "h guard rows"))
    written = np.zeros(out.shape, bool)
    written[:B] = True
    check_untouched(np.asarray(out, np.float32), np.asarray(resid, np.float32), written, (what, "out guard rows"))


def check_chain(h_bits, out, resid, h_ref, Wd, what=""):
    """h_bits [B + g][F] uint16: the h buffer after the launch (f16 NaN before it); out / resid
    [B + g][K] f32: the output after / before; h_ref [B][F] from h_reference. Returns the worst row's
    error of h and of the down as fractions of their bounds."""
    B = h_ref.shape[0]
    _guard(h_bits, out, resid, B, what)
    hv = h_values(np.asarray(h_bits)[:B])
    fh = check_rows(hv, h_ref, H_BOUND, (what, "h"))
    delta = np.asarray(out, np.float64)[:B] - np.asarray(resid, np.float64)[:B]
    fd = check_rows(delta, down_ref(hv, Wd), DN_BOUND, (what, "down"))
    return fh, fd


def wo_h_bounds(resid0, wo_ref):
    """The Wo chain's per-row bound on h: H_BOUND + WO_H_FACTOR delta_b."""
    r = np.asarray(resid0, np.float64)
    delta = DN_BOUND * np.linalg.norm(wo_ref, axis=1) / np.linalg.norm(r + wo_ref, axis=1)
    return H_BOUND + WO_H_FACTOR * delta


def wo_h_reference(resid0, wo_ref, nw, Wgu, eps=EPS):
    x = (np.asarray(resid0, np.float64) + wo_ref).astype(np.float32)
    return h_reference(x, nw, Wgu, True, eps)


def check_wo_chain(h_bits, r, resid0, wo_ref, nw, Wgu, Wd, what=""):
    """r / resid0 [B + g][K] f32: the residual rows after / before the launch; wo_ref [B][K]: fp64
    W_o xa. Final rows: |r - resid0 - Wo - down(h_got)| within DN_BOUND (|Wo_b| + |down_b|); h within
    wo_h_bounds of the fp64 SwiGLU of norm(resid0 + Wo). Returns both worst fractions."""
    B = wo_ref.shape[0]
    _guard(h_bits, r, resid0, B, what)
    hv = h_values(np.asarray(h_bits)[:B])
    h_ref = wo_h_reference(np.asarray(resid0)[:B], wo_ref, nw, Wgu)
    bounds = wo_h_bounds(np.asarray(resid0)[:B], wo_ref)
    fh = max(check_rows(hv[b:b + 1], h_ref[b:b + 1], bounds[b], (what, "h row", b)) for b in range(B))
    dn = down_ref(hv, Wd)
    got = np.asarray(r, np.float64)[:B]
    assert np.all(np.isfinite(got)), (what, "non-finite final rows")
    err = np.linalg.norm(got - np.asarray(resid0, np.float64)[:B] - wo_ref - dn, axis=1)
    frac = err / (DN_BOUND * (np.linalg.norm(wo_ref, axis=1) + np.linalg.norm(dn, axis=1)))
    b = int(np.argmax(frac))
    assert frac[b] < 1.0, (what, "final row", b, "error / bound", float(frac[b]))
    return fh, float(frac[b])


def check_zeroed(z_bits, zero_n, poison, what=""):
    """The zero side job: exactly the first zero_n floats are +0.0, the rest keep the poison bits."""
    z = np.asarray(z_bits)
    bad = np.flatnonzero(z[:zero_n] != 0)
    assert bad.size == 0, (what, "zero side job left float", int(bad[0]))
    bad = np.flatnonzero(z[zero_n:] != poison)
    assert bad.size == 0, (what, "zero side job wrote past zero_n, float", zero_n + int(bad[0]))


# ---------------------------------------------------------------------------- CPU emulation
def emulate_chain(X, nw, Wgu, Wd, resid, norm, plan, eps=EPS):
    """The chain in the kernels' number formats on the CPU: f16 staged rows and f16 weights, fp32
    sums, the folded norm's scale applied to the fp32 sums, f16 h, the down's partial sums added to the
    fp32 output part by part. Returns (h bits with one guard row, out)."""
    B = X.shape[0]
    X = np.asarray(X, np.float32)
    if norm:
        xs = (X * nw).astype(np.float16).astype(np.float32)
        cs = (1.0 / np.sqrt((X.astype(np.float64) ** 2).mean(1, keepdims=True) + eps)).astype(np.float32)
    else:
        xs, cs = X.astype(np.float16).astype(np.float32), np.float32(1.0)
    pre = (xs @ np.asarray(Wgu, np.float16).astype(np.float32).T) * cs
    F = pre.shape[1] // 2
    pre = pre.reshape(B, F // 32, 2, 32)
    g, u = pre[:, :, 0].reshape(B, F), pre[:, :, 1].reshape(B, F)
    h = silu_mul(g, u).astype(np.float16)   # (fp32 in, fp32 out)
    hb = np.full((B + 1, F), NAN16, np.uint16)
    hb[:B] = swizzle4(h).view(np.uint16)
    out = np.array(resid, np.float32)
    Wd16 = np.asarray(Wd, np.float16).astype(np.float32)
    s0 = 0
    for ns in plan.part_steps:
        c = slice(256 * s0, 256 * (s0 + ns))
        out[:B] += h[:, c].astype(np.float32) @ Wd16[:, c].T
        s0 += ns
    return hb, out
