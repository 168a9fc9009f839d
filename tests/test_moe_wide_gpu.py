"""The wide-MoE kernels (csrc/kernels/moe_wide.hip: 17 .. 256 experts, top-k up to 16) against the fp64
references and checkers of moe_ref.py, over poisoned buffers with sentinels past the written region."""
import os

import numpy as np
import pytest

from gpu_helpers import hip, stream
from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
import moe_ref as mr
from test_moe_paths_gpu import SLACK, _bits, _filled, _stacked_t16, _experts, _values, torch  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
Q4_K, Q6_K, Q8_0 = GGMLType.Q4_K, GGMLType.Q6_K, GGMLType.Q8_0
TAIL = 8
FIGURES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "moe_wide_test_figures.txt")


def _ws(torch, nbytes):
    return torch.zeros(nbytes // 4 + 1, dtype=torch.int32, device="cuda")


def _router_inputs(E, k, d, rows, seed):
    """x [rows][d], w_norm, W [E][d] whose fp64 logits keep moe_ref's margin; rows are redrawn until they
    do. Row 0 then gets one planted exact tie: two router rows are made equal, the lower id must win."""
    rng = np.random.default_rng(seed)
    nw = (0.5 + rng.random(d)).astype(np.float32)
    W = (rng.standard_normal((E, d)) * 2.0 / np.sqrt(d)).astype(np.float32)
    tie = (E - 2, E - 1)
    W[tie[1]] = W[tie[0]]

    def logits(x):
        x = x.astype(np.float64)
        n = x * nw / np.sqrt((x * x).mean(1, keepdims=True) + 1e-5)
        return n @ W.astype(np.float64).T

    x = np.empty((rows, d), np.float32)
    for r in range(rows):
        while True:
            x[r] = rng.standard_normal(d).astype(np.float32) * 3
            lg = logits(x[r:r + 1])
            in_top = lg[0, tie[0]] >= np.sort(lg[0])[-k] if r == 0 else True   # row 0: the tied pair is picked
            if mr.route_margin(lg.astype(np.float32), k) >= 4 * mr.MARGIN and in_top:
                break
    return x, nw, W, logits(x), tie


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("d", [256, 2048])
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("E", [17, 64, 65, 128, 256])
def test_router_wide(torch, E, k, d, rows):
    x, nw, W, lg, tie = _router_inputs(E, k, d, rows, 1000 * E + 10 * k + d + rows)
    ldx = d + 8 if rows > 1 else d
    dx = torch.full((rows, ldx), float("nan"), device="cuda")
    dx[:, :d] = torch.from_numpy(x).cuda()
    dnw, dW = torch.from_numpy(nw).cuda(), torch.from_numpy(W).cuda()
    ws = _ws(torch, hip().moe_router_wide_workspace(rows, E))
    runs = []
    for _ in range(2):   # the second launch runs on the counters the first re-armed
        ids = torch.full((rows * k + TAIL,), -7, dtype=torch.int32, device="cuda")
        w = torch.full((rows * k + TAIL,), -7.0, device="cuda")
        out_lg = torch.full((rows * E + TAIL,), -7.0, device="cuda")
        hip().moe_router_wide(dx.data_ptr(), ldx, rows, dnw.data_ptr(), 1e-5, dW.data_ptr(), d, E, k, ws.data_ptr(),
                              out_lg.data_ptr(), ids.data_ptr(), w.data_ptr(), stream())
        torch.cuda.synchronize()
        runs.append((ids.cpu().numpy(), w.cpu().numpy(), out_lg.cpu().numpy()))
    ids, w, out_lg = runs[0]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(runs[0], runs[1])), "two runs differ"
    assert np.all(ids[rows * k:] == -7) and np.all(w[rows * k:] == -7) and np.all(out_lg[rows * E:] == -7)
    ref = mr.route_reference(lg.astype(np.float32), k)
    assert np.array_equal(ids[:rows * k].reshape(rows, k), ref.sel)
    sel0 = list(ref.sel[0])
    # the planted tie: the lower id is picked first (and alone where the pair straddles the k-th place)
    assert tie[0] in sel0 and (tie[1] not in sel0 or sel0.index(tie[1]) == sel0.index(tie[0]) + 1)
    np.testing.assert_allclose(w[:rows * k].reshape(rows, k), ref.selw, rtol=mr.GW_RTOL, atol=mr.GW_ATOL)
    np.testing.assert_allclose(out_lg[:rows * E].reshape(rows, E), lg, rtol=1e-4, atol=1e-4)


def _group_dev(torch, E, k, lg=None, sel=None, selw=None, ws=None):
    T = (lg if lg is not None else sel).shape[0]
    R, mi = T * k, hip().moe_group_wide_items(T, E, k)
    o = dict(sel=torch.full((R + TAIL,), -7, dtype=torch.int32, device="cuda"), selw=torch.full((R + TAIL,), -7.0, device="cuda"),
             cnt_off=torch.full((E + 1 + TAIL,), -7, dtype=torch.int32, device="cuda"),
             tok=torch.full((R + TAIL,), -7, dtype=torch.int32, device="cuda"), gw=torch.full((R + TAIL,), -7.0, device="cuda"),
             pos=torch.full((R + TAIL,), -7, dtype=torch.int32, device="cuda"),
             items=torch.full((3 * mi + TAIL,), -7, dtype=torch.int32, device="cuda"),
             n_items=torch.full((1 + TAIL,), -7, dtype=torch.int32, device="cuda"))
    lp = 0
    if lg is not None:
        dl = torch.from_numpy(lg).cuda()
        lp = dl.data_ptr()
    else:
        o["sel"][:R] = torch.from_numpy(sel.reshape(-1).astype(np.int32)).cuda()
        o["selw"][:R] = torch.from_numpy(selw.reshape(-1).astype(np.float32)).cuda()
    ws = ws if ws is not None else _ws(torch, hip().moe_group_wide_workspace(T, E))
    for _ in range(2):   # (the second launch: re-armed counter, same result)
        hip().moe_route_group_wide(lp, T, E, k, *(o[n].data_ptr() for n in ("sel", "selw", "cnt_off", "tok", "gw", "pos",
                                                                         "items", "n_items")), ws.data_ptr(), stream())
    torch.cuda.synchronize()
    return o, mi


def _check_group(o, mi, ref, T, E, k):
    R = T * k
    n = dict(sel=R, selw=R, cnt_off=E + 1, tok=R, gw=R, pos=R, n_items=1)
    host = {name: v.cpu().numpy() for name, v in o.items()}
    for name, m in n.items():
        assert np.all(host[name][m:] == -7), (name, "written past its end")
    mr.check_routing({name: host[name][:m] for name, m in n.items()}, ref, T, E, k)
    ni, RT = int(host["n_items"][0]), hip().MOE_ITEM_ROWS
    cnt = np.diff(ref.cnt_off)
    assert ni == int(np.sum((cnt + RT - 1) // RT)) <= mi
    items = host["items"][:3 * ni].reshape(ni, 3)
    assert np.all(host["items"][3 * ni:] == -7), "items written past the count"
    cover = np.zeros(R, int)
    for e, r0, rows in items:
        assert 1 <= rows <= RT and ref.cnt_off[e] <= r0 and r0 + rows <= ref.cnt_off[e + 1], (e, r0, rows)
        cover[r0:r0 + rows] += 1
    assert np.all(cover == 1) and not set(items[:, 0]) & set(np.flatnonzero(cnt == 0))
    return items


def _skewed_logits(T, E, k, seed):
    """Random routing with margin, except that expert E - 1 takes min(T, 70) rows and expert 0 none."""
    lg = mr.routing_logits(T, E, k, "random", seed)
    lg[:, 0] = -30.0
    lg[:, E - 1] = -30.0
    lg[:min(T, 70), E - 1] = 12.0
    return lg


@pytest.mark.parametrize("E", [65, 128])
@pytest.mark.parametrize("T", [1, 6, 63, 65, 130])
def test_route_group_wide(torch, T, E):
    k = 8
    lg = _skewed_logits(T, E, k, 100 * T + E)
    ref = mr.route_reference(lg, k)
    cnt = np.diff(ref.cnt_off)
    assert cnt[0] == 0 and cnt[E - 1] == min(T, 70)
    o, mi = _group_dev(torch, E, k, lg=lg)
    _check_group(o, mi, ref, T, E, k)
    o2, _ = _group_dev(torch, E, k, sel=ref.sel, selw=ref.selw)   # the picks handed in: the top-k is skipped
    _check_group(o2, mi, ref, T, E, k)


def test_one_workspace_serves_launches_of_different_row_counts(torch):
    """As the engine runs them: launches of 5, 40 and 3 rows on the same workspaces (the counters of one
    size must not lie in what another size writes)."""
    E, k, d = 128, 8, 256
    gws, rws = _ws(torch, hip().moe_group_wide_workspace(40, E)), _ws(torch, hip().moe_router_wide_workspace(5, E))
    for T in (5, 40, 3):
        lg = _skewed_logits(T, E, k, 7 * T)
        _check_group(*_group_dev(torch, E, k, lg=lg, ws=gws), mr.route_reference(lg, k), T, E, k)
    for rows in (5, 3, 1):
        x, nw, W, lg, _ = _router_inputs(E, k, d, rows, 50 + rows)
        dx, dnw, dW = (torch.from_numpy(a).cuda() for a in (x, nw, W))
        ids = torch.full((rows, k), -7, dtype=torch.int32, device="cuda")
        w = torch.full((rows, k), -7.0, device="cuda")
        hip().moe_router_wide(dx.data_ptr(), d, rows, dnw.data_ptr(), 1e-5, dW.data_ptr(), d, E, k, rws.data_ptr(), 0,
                              ids.data_ptr(), w.data_ptr(), stream())
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy(), mr.route_reference(lg.astype(np.float32), k).sel), rows


@pytest.mark.parametrize("T", [1, 6, 70])
@pytest.mark.parametrize("F", [256, 768])
@pytest.mark.parametrize("tg,td", [(Q4_K, Q6_K), (Q8_0, Q8_0)])
def test_grouped_one_launch_vs_fp64(torch, tg, td, F, T):
    """Worst row / bound so far (MI355X): see profiles/moe_wide_test_figures.txt."""
    E, k, d = 128, 8, 512
    lg = _skewed_logits(T, E, k, T + F)
    rt = mr.route_reference(lg, k)
    o, mi = _group_dev(torch, E, k, lg=lg)
    items = _check_group(o, mi, rt, T, E, k)
    R = T * k
    exg, exd = _experts(tg, E, d, F), _experts(td, E, d, F)
    gu = _stacked_t16(torch, tg, E, d, F)[0]
    dn = _stacked_t16(torch, td, E, d, F)[1]
    rng = np.random.default_rng(T * 10 + F)
    X = rng.standard_normal((T, d)).astype(np.float16)
    xg = _filled(torch, (R + SLACK, d), torch.float16, mr.NAN16)
    xg[:R] = torch.from_numpy(mr.swizzle4(X)[rt.tok]).cuda()
    h = _filled(torch, (R + SLACK, F), torch.float16, mr.NAN16)
    y = _filled(torch, (R + SLACK, d), torch.float32, mr.NAN32)   # no pre-zeroing: plain stores over NaN
    for w, t, x, out, sw in ((gu, tg, xg, h, True), (dn, td, h, y, False)):
        hip().moe_gemm_grouped(w.data_ptr(), int(t), d, F, E, x.data_ptr(), out.data_ptr(), sw, o["items"].data_ptr(),
                               o["n_items"].data_ptr(), mi, stream())
    torch.cuda.synchronize()
    hb, yb = _bits(torch, h), _bits(torch, y)
    assert np.all(hb[R:] == mr.NAN16) and np.all(yb[R:] == mr.NAN32), "rows past T k written"
    hv, yv = _values(hb[:R], "f16"), y[:R].cpu().numpy()
    worst = [0.0, 0.0]
    xr = X.astype(np.float64)[rt.tok]
    for e in sorted(set(items[:, 0])):
        r0, r1 = int(rt.cnt_off[e]), int(rt.cnt_off[e + 1])
        worst[0] = max(worst[0], mr.check_rows(hv[r0:r1], mr.swiglu_ref(xr[r0:r1], exg["Wgu"][e]), mr.T16_GU, ("swiglu", e)))
        worst[1] = max(worst[1], mr.check_rows(yv[r0:r1], mr.down_ref(hv[r0:r1], exd["Wd"][e]), mr.T16_DN, ("down", e)))
    line = f"grouped {tg.name}/{td.name} F={F} T={T} swiglu {worst[0]:.3f} down {worst[1]:.3f} (worst row / bound)"
    print("MOE_FRAC", line)
    key = line.split(" swiglu")[0]   # one line per case: a rerun replaces its own
    old = open(FIGURES).read().splitlines() if os.path.exists(FIGURES) else []
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("\n".join(sorted([l for l in old if l.split(" swiglu")[0] != key] + [line])) + "\n")
