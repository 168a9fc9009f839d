"""CPU self-test of the Q|K|V checker (qkv_ref.check_qkv): it accepts the fp64 reference under
simulated rounding and rejects each single defect the engine-level logit comparisons let through."""
import numpy as np
import pytest

from qkv_ref import _rope_pairs, _rope_table, check_qkv, qkv_reference

B, HD, H, HKV, K, N_CTX, N_SLOTS = 3, 64, 4, 2, 256, 64, 5
NQ, NKV = H * HD, HKV * HD


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((B, K)).astype(np.float16)
    Ws = [(rng.standard_normal((R, K)) * 0.05).astype(np.float32) for R in (NQ, NKV, NKV)]
    rms = float(np.sqrt(np.mean((X.astype(np.float64) @ Ws[0].astype(np.float64).T) ** 2)))
    bias = (rng.standard_normal(NQ + 2 * NKV) * 3 * rms).astype(np.float32)   # ~3x the projection's rms
    pos = np.array([0, N_CTX - 1, 17], np.int32)
    slots = np.array([3, 0, 2], np.int32)            # slots 1 and 4 idle
    tab = _rope_table(N_CTX, HD)
    ref = qkv_reference(X, None, 1e-5, Ws, bias, pos, slots, tab, N_CTX, HD)
    sentK = rng.standard_normal((N_SLOTS, HKV, N_CTX, HD)).astype(np.float16)
    sentV = rng.standard_normal((N_SLOTS, HKV, N_CTX, HD)).astype(np.float16)
    sentq = rng.standard_normal((B + 1, NQ + 4)).astype(np.float32)
    return dict(ref=ref, bias=bias.astype(np.float64), pos=pos, slots=slots, tab=tab, sentK=sentK, sentV=sentV,
                sentq=sentq)


def simulate(c, defect=None):
    """What a kernel with the given single defect would leave in q_out and the caches: the fp64
    arithmetic of the reference, relative Gaussian noise of 1e-3, caches cast to f16."""
    ref, bias, pos, slots, tab = c["ref"], c["bias"], c["pos"], c["slots"], c["tab"]
    rng = np.random.default_rng(1)
    y = ref.raw + bias[None, :]
    q = np.stack([_rope_pairs(y[b, :NQ], pos[b], tab) for b in range(B)])
    k = np.stack([_rope_pairs(y[b, NQ:NQ + NKV], pos[b], tab) for b in range(B)])
    v = y[:, NQ + NKV:].copy()
    b = 2                                            # the row at position 17: a rotation far from identity
    kpos, kslot = pos.copy(), slots.copy()
    if defect == "first_pair_unrotated":             # head 1 of q
        q[b, HD:HD + 2] = y[b, HD:HD + 2]
    elif defect == "last_pair_next_head_freq":       # head 0's last pair turned by pair 0's angle
        c0, s0 = float(tab[pos[b], 0, 0]), float(tab[pos[b], 0, 1])
        a0, a1 = y[b, HD - 2], y[b, HD - 1]
        q[b, HD - 2], q[b, HD - 1] = a0 * c0 - a1 * s0, a0 * s0 + a1 * c0
    elif defect == "bias_after_rotation":
        q = np.stack([_rope_pairs(ref.raw[i, :NQ], pos[i], tab) for i in range(B)]) + bias[None, :NQ]
    elif defect == "kv_swapped":
        k[b], v[b] = v[b].copy(), k[b].copy()
    elif defect == "k_at_next_pos":
        kpos[b] += 1
    elif defect == "row_in_other_slot":
        kslot[b] = slots[0]
    elif defect is not None and defect != "idle_slot_element":
        raise ValueError(defect)
    noisy = lambda a: a * (1 + 1e-3 * rng.standard_normal(a.shape))
    got_q = c["sentq"].copy()
    got_q[:B, :NQ] = noisy(q).astype(np.float32)
    got_K, got_V = c["sentK"].copy(), c["sentV"].copy()
    for i in range(B):
        got_K[kslot[i], :, kpos[i]] = noisy(k[i]).reshape(HKV, HD).astype(np.float16)
        got_V[slots[i], :, pos[i]] = noisy(v[i]).reshape(HKV, HD).astype(np.float16)
    if defect == "idle_slot_element":
        got_V[4, 1, 9, 5] = np.float16(float(got_V[4, 1, 9, 5]) + 1.0)
    return got_q, got_K, got_V


def test_reference_with_rounding_noise_passes(case):
    got_q, got_K, got_V = simulate(case)
    worst = check_qkv(got_q, got_K, got_V, case["ref"], case["sentK"], case["sentV"], sentinel_q=case["sentq"])
    assert 0 < worst["norm"] < 1 and 0 < worst["elem"] < 1, worst


# (defect, where check_qkv must report it: segment name and row, or the sentinel check)
DEFECTS = [("first_pair_unrotated", r"'q', 2"), ("last_pair_next_head_freq", r"'q', 2"),
           ("bias_after_rotation", r"'q', 1"), ("kv_swapped", r"'k', 2"),
           ("k_at_next_pos", r"'k', 2"), ("row_in_other_slot", r"'k', 2"),
           ("idle_slot_element", r"'V', \"cache written outside")]


@pytest.mark.parametrize("defect,where", DEFECTS, ids=[d for d, _ in DEFECTS])
def test_single_defect_is_rejected(case, defect, where):
    got_q, got_K, got_V = simulate(case, defect)
    with pytest.raises(AssertionError, match=where):
        check_qkv(got_q, got_K, got_V, case["ref"], case["sentK"], case["sentV"], sentinel_q=case["sentq"])


def test_write_outside_q_rows_is_rejected(case):
    got_q, got_K, got_V = simulate(case)
    got_q[B, 0] += 1.0
    with pytest.raises(AssertionError):
        check_qkv(got_q, got_K, got_V, case["ref"], case["sentK"], case["sentV"], sentinel_q=case["sentq"])
