"""fp64 reference of the device sampler's mirostat path (engine/sampling.py:HostSampler._mirostat is
the specification) and the bounds within which the fp32 kernel may differ from it.

From the fp32 logits, the parameters, the penalty window and mu: the prepared logits (bias, penalties,
/ temperature), the order (value descending, id ascending), k, the kept CDF and u, all in fp64.

Bounds, with e = 2^-24 (one fp32 rounding) and A = the largest |prepared logit|:
  * a prepared logit carries at most 4 roundings (bias, penalty product, penalty difference, division),
    and l - M one more: its exponent is off by <= 6 A e, expf adds 2 e: each term exp(l - M) is within
    r_term = 6 A e + 2 e of the reference's, relatively.
  * a cumulative sum adds at most ceil(V / 256) terms serially per thread, then 6 scan levels and 3
    wave offsets (window path), or 8 reduction levels (bisection path): n_add = ceil(V / 256) + 12
    roundings of partial sums that never exceed Z_k. So every CDF boundary, and u Z_k itself (2 more),
    is within d = Z_k (r_term + (n_add + 2) e) of the reference.
  * v2's threshold M + ln Z - mu ln 2 is compared in logits: 3 roundings of magnitudes <= A + |mu|,
    ln Z within r_term + (n_add + 2) e: a surprise within d_s = (4 (A + |mu|) e + r_term + (n_add + 2) e)
    / ln 2 + 6 A e / ln 2 of mu may count either way.
  * the new mu: ln p_kept within 2 r_term + (n_add + 4) e + 4 (A + ln Z_k) e, times eta / ln 2, plus 4
    roundings of magnitudes <= |mu| + |tau| + surprise.
  * v1's k is computed in fp64 on the device from the fp32 prepared logits. The v1 cases use
    temperature 1, no bias and no penalty, so those are exact and k differs by fp64 rounding only:
    the test asks k to be 1e-6 k away from an integer.
The tests assert, before any launch, that no CDF boundary lies within d of u Z_k and (v2) no surprise
within d_s of mu, so every case has exactly one acceptable token."""
import math

import numpy as np

from llama_fastapi_k8s_gpu_amd.engine.sampling import MIROSTAT_M, philox_uniform

E = 2.0 ** -24


def reference(x, p, window, mu, step, extreme=True):
    """-> dict(token, mu, k, kept ids, margin): `extreme` asserts the kernel cases' logit range; margin = the smallest distance of a decision from its bound, as a
    multiple of the bound (> 1: the case has one acceptable token)."""
    V = x.shape[0]
    l = np.asarray(x, np.float64).copy()
    for t, b in p.logit_bias.items():
        l[t] += np.float64(np.float32(b))
    counts = {}
    for t in list(window)[-p.last_n:]:
        counts[int(t)] = counts.get(int(t), 0) + 1
    for t, c in counts.items():
        v = l[t] * np.float32(p.repeat_penalty) if l[t] <= 0 else l[t] / np.float32(p.repeat_penalty)
        l[t] = v - (c * np.float64(np.float32(p.frequency_penalty)) + np.float32(p.presence_penalty))
    l /= np.float32(p.temperature)
    order = np.lexsort((np.arange(V), -l))
    vals = l[order]
    with np.errstate(over="ignore"):
        assert not extreme or (np.isinf(np.exp(np.float32(vals[0]))) and vals[-1] < -89), \
            "exp(max) must overflow fp32 unless the maximum is subtracted"
    e = np.exp(vals - vals[0])
    A, n_add = float(np.abs(vals).max()), -(-V // 256) + 12
    r_term = 6 * A * E + 2 * E
    margin = math.inf
    if p.mirostat_mode == 2:
        surprise = -np.log2(e / e.sum())
        over = np.nonzero(surprise > mu)[0]
        k = max(int(over[0]) if len(over) else V, 1)
        d_s = (4 * (A + abs(mu)) * E + r_term + (n_add + 2) * E + 6 * A * E) / math.log(2)
        margin = float(np.abs(surprise - mu).min()) / d_s
    else:
        m = min(MIROSTAT_M, V - 1)
        t = np.log((np.arange(m) + 2.0) / (np.arange(m) + 1.0))
        s_hat = float((t * (vals[:m] - vals[1:m + 1])).sum() / (t * t).sum())
        kf = ((s_hat - 1.0) * 2.0 ** mu / (1.0 - float(V) ** (1.0 - s_hat))) ** (1.0 / s_hat)
        k = int(max(1, min(kf, V)))
        if 1 < kf < V:
            margin = min(kf - math.floor(kf), math.ceil(kf) - kf) / (1e-6 * kf)
    c = np.cumsum(e[:k])
    Zk, u = c[-1], philox_uniform(p.seed, step)
    j = min(int(np.searchsorted(c, u * Zk, side="right")), k - 1)
    d = Zk * (r_term + (n_add + 2) * E)
    margin = min(margin, float(np.abs(c[:-1] - u * Zk).min()) / d if k > 1 else math.inf)
    surprise_j = -math.log2(e[j] / Zk)
    mu_new = mu - float(np.float32(p.mirostat_eta)) * (surprise_j - float(np.float32(p.mirostat_tau)))
    d_mu = p.mirostat_eta * (2 * r_term + (n_add + 4) * E + 4 * (A + abs(math.log(Zk))) * E) / math.log(2) \
        + 4 * E * (abs(mu) + abs(p.mirostat_tau) + surprise_j)
    return {"token": int(order[j]), "mu": float(mu_new), "d_mu": d_mu, "k": k, "kept": set(order[:k].tolist()), "margin": margin,
            "cut_in_tie": k < V and vals[k - 1] == vals[k]}
