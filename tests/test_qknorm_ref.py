"""CPU self-test of the QK-norm Q|K|V reference (qknorm_ref.py) under qkv_ref.check_qkv: the fp64
reference passes under simulated rounding, and each single defect a QK-norm kernel can have is
rejected. Two of them (eps omitted, the row scale dropped in front of the norm) only show when eps
matters, so the case is run with the model's eps and with one of about half a head's mean square -
the GPU tests carry such a case for the same reason."""
import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize
from qknorm_ref import (SK_CASES, SK_K, SK_NCTX, f16_staged_error, head_norm, neox_perm, qknorm_reference,
                        splitk_inputs)
from qkv_ref import NORM_BOUND, _rope_pairs, _rope_table, check_qkv

B, HD, H, HKV, K, N_CTX, N_SLOTS = 3, 64, 4, 2, 256, 64, 5
NQ, NKV = H * HD, HKV * HD
ROW_SCALE = np.array([0.5, 1.0, 2.0])   # standard-normal rows times these: the rows' 1/rms differ from 1


def make_case(big_eps):
    rng = np.random.default_rng(0)
    X = (rng.standard_normal((B, K)) * ROW_SCALE[:, None]).astype(np.float32)
    nw = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    Ws = [rng.standard_normal((R, K)).astype(np.float32) for R in (NQ, NKV, NKV)]
    w_file = (1.0 + 0.5 * rng.standard_normal(2 * HD)).astype(np.float32)   # as the synthetic files draw them
    perm = neox_perm(HD)
    w_kernel = np.concatenate([w_file[:HD][perm], w_file[HD:][perm]])
    pos = np.array([0, N_CTX - 1, 17], np.int32)
    slots = np.array([3, 0, 2], np.int32)
    tab = _rope_table(N_CTX, HD)
    eps = 1e-6
    # a head's mean square is about K (unit-variance inputs and weights)
    qkn_eps = 0.5 * K if big_eps else 1e-6
    ref = qknorm_reference(X, nw, eps, Ws, w_kernel, qkn_eps, pos, slots, tab, N_CTX, HD, staging="folded")
    rs = 1.0 / np.sqrt((X.astype(np.float64) ** 2).mean(1) + eps)
    sentK = rng.standard_normal((N_SLOTS, HKV, N_CTX, HD)).astype(np.float16)
    sentV = rng.standard_normal((N_SLOTS, HKV, N_CTX, HD)).astype(np.float16)
    sentq = rng.standard_normal((B + 1, NQ + 4)).astype(np.float32)
    return dict(ref=ref, w=w_kernel.astype(np.float64), w_file=w_file.astype(np.float64), qkn_eps=qkn_eps, rs=rs,
                pos=pos, slots=slots, tab=tab, sentK=sentK, sentV=sentV, sentq=sentq)


@pytest.fixture(scope="module", params=[False, True], ids=["model_eps", "big_eps"])
def case(request):
    return make_case(request.param)


def simulate(c, defect=None):
    """q_out and the caches as a kernel with the given single defect would leave them: fp64
    arithmetic, relative Gaussian noise of 1e-3, caches cast to f16."""
    ref, w, eps, pos, slots, tab = c["ref"], c["w"], c["qkn_eps"], c["pos"], c["slots"], c["tab"]
    rng = np.random.default_rng(1)
    y = ref.raw
    yq, yk = y[:, :NQ], y[:, NQ:NQ + NKV]
    wq, wk = w[:HD], w[HD:]
    rope = lambda a: np.stack([_rope_pairs(a[b], pos[b], tab) for b in range(B)])
    if defect is None:
        q, k = rope(head_norm(yq, wq, eps, HD)), rope(head_norm(yk, wk, eps, HD))
    elif defect == "no_norm":
        q, k = rope(yq), rope(yk)
    elif defect == "weight_dropped":
        q, k = rope(head_norm(yq, np.ones(HD), eps, HD)), rope(head_norm(yk, np.ones(HD), eps, HD))
    elif defect == "weights_in_file_order":
        q, k = rope(head_norm(yq, c["w_file"][:HD], eps, HD)), rope(head_norm(yk, c["w_file"][HD:], eps, HD))
    elif defect == "norm_after_rotation_pair_swapped":
        sw = np.arange(HD) ^ 1
        q, k = head_norm(rope(yq), wq[sw], eps, HD), head_norm(rope(yk), wk[sw], eps, HD)
    elif defect == "norm_over_whole_row":
        q = rope(head_norm(yq, np.tile(wq, H), eps, NQ))
        k = rope(head_norm(yk, np.tile(wk, HKV), eps, NKV))
    elif defect == "eps_omitted":
        q, k = rope(head_norm(yq, wq, 0.0, HD)), rope(head_norm(yk, wk, 0.0, HD))
    elif defect == "row_scale_dropped":   # the head norm fed the sums without the row's 1/rms
        un = 1.0 / c["rs"][:, None]
        q, k = rope(head_norm(yq * un, wq, eps, HD)), rope(head_norm(yk * un, wk, eps, HD))
    else:
        raise ValueError(defect)
    v = y[:, NQ + NKV:]
    noisy = lambda a: a * (1 + 1e-3 * rng.standard_normal(a.shape))
    got_q = c["sentq"].copy()
    got_q[:B, :NQ] = noisy(q).astype(np.float32)
    got_K, got_V = c["sentK"].copy(), c["sentV"].copy()
    for i in range(B):
        got_K[slots[i], :, pos[i]] = noisy(k[i]).reshape(HKV, HD).astype(np.float16)
        got_V[slots[i], :, pos[i]] = noisy(v[i]).reshape(HKV, HD).astype(np.float16)
    return got_q, got_K, got_V


def _check(c, got):
    return check_qkv(*got, c["ref"], c["sentK"], c["sentV"], sentinel_q=c["sentq"])


def test_reference_with_rounding_noise_passes(case):
    worst = _check(case, simulate(case))
    assert 0 < worst["norm"] < 1 and 0 < worst["elem"] < 1, worst


def test_f16_storage_alone_is_under_half_the_bound(case):
    """The inputs' own f16 cache rounding against fp64, before any kernel: well under half a bound."""
    assert f16_staged_error(case["ref"]) < 0.5 * NORM_BOUND


def test_the_permutation_leaves_a_heads_mean_square(case):
    y = case["ref"].raw[:, :HD]
    assert np.allclose((y ** 2).mean(1), (y[:, neox_perm(HD)] ** 2).mean(1), rtol=1e-12)
    assert sorted(neox_perm(HD)) == list(range(HD)) and list(neox_perm(8)) == [0, 4, 1, 5, 2, 6, 3, 7]


@pytest.mark.parametrize("hd,G,big_eps", SK_CASES)
def test_f16_staging_of_the_gpu_tests_inputs_is_under_half_the_bound(hd, G, big_eps):
    """The inputs of test_qwen3_gpu.py's split-K cases, before any GPU run: the kernels' staging -
    f16(x * norm_w), the tile16 copy's f16-arithmetic weights, f16 K / V rows - against the fp64
    reference on the exact dequantised weights. Past half a bound the inputs would have to change."""
    t = GGMLType.Q4_K
    c = splitk_inputs(hd, G, big_eps, t)
    tab = _rope_table(SK_NCTX, hd)
    run = lambda Ws: qknorm_reference(c["X"], c["nw"], c["eps"], Ws, c["w"], c["qkn_eps"], c["pos"], c["slots"], tab,
                                      SK_NCTX, hd, staging="folded")
    ref = run([m[1] for m in c["mats"]])
    emu = run([np.asarray(dequantize(m[0], t, m[1].size, arith="f16"), np.float64).reshape(m[1].shape) for m in c["mats"]])
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    f16 = lambda a: a.astype(np.float16).astype(np.float64)
    worst = max(max(rel(emu.q[b], ref.q[b]), rel(f16(emu.k[b]), ref.k[b]), rel(f16(emu.v[b]), ref.v[b]))
                for b in range(ref.q.shape[0]))
    print("f16-staged / NORM_BOUND", hd, G, big_eps, worst / NORM_BOUND)
    assert worst < 0.5 * NORM_BOUND, worst
    ms = float((ref.raw[:, :hd] ** 2).mean())
    assert 0.5 * SK_K < ms < 2 * SK_K     # "half a head's mean square" is what the big eps is


ALWAYS = ["no_norm", "weight_dropped", "weights_in_file_order", "norm_after_rotation_pair_swapped",
          "norm_over_whole_row"]
EPS_ONLY = ["eps_omitted", "row_scale_dropped"]


@pytest.mark.parametrize("defect", ALWAYS)
def test_single_defect_is_rejected(case, defect):
    with pytest.raises(AssertionError, match=r"'q', 0"):
        _check(case, simulate(case, defect))


@pytest.mark.parametrize("defect", EPS_ONLY)
def test_eps_defects_show_only_when_eps_matters(defect):
    big, small = make_case(True), make_case(False)
    with pytest.raises(AssertionError, match=r"'q', 0"):
        _check(big, simulate(big, defect))
    _check(small, simulate(small, defect))   # with the model's 1e-6 the same defect is invisible: hence the big-eps case
