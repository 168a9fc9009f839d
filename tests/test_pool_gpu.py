"""The embedding epilogue's two launches (pool_rows / pool_finish, csrc/kernels/misc.hip) over raw
buffers, without an engine: results judged by tests/pool_ref.py against fp64 with the derived bound,
every buffer sentinel-filled so that a byte written outside the result region shows.

Inputs (pool_ref.make_case): a NaN guard row behind every segment and NaN padding columns where
ldx > d; the partial, accumulator and output buffers are poisoned before the first launch.
"""
import os

import numpy as np
import pytest

import pool_ref as pr
from gpu_helpers import hip, stream

pytestmark = pytest.mark.gpu

POISON = np.float32(-7.25e33)   # a finite sentinel compares equal to itself (NaN would not)
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _record_figures():
    """With LFK_FIGURES_OUT=<file> set, the worst error / bound of every case that ran is written
    to that file when the module ends (profiles/embed_test_figures.txt is made from it)."""
    _worst.clear()
    yield
    out = os.environ.get("LFK_FIGURES_OUT")
    if out and _worst:
        with open(out, "w") as fh:
            fh.write("".join(f"{k}: {v:.4f}\n" for k, v in sorted(_worst.items())))


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _table(segs):
    return [int(v) for s in segs for v in s]


def run_case(torch, case, mode, normalize, part_rows=None):
    """Both launches over every launch of the case -> ({key: vector}, buffers for the sentinel checks)."""
    d, n_in = case["d"], case["n_inputs"]
    w = torch.from_numpy(case["w"]).cuda()
    need = max(sum(pr.groups_of(s[1]) for s in segs) for _, segs in case["launches"])
    part_rows = part_rows or need + 2
    part = torch.full((part_rows, d), float(POISON), dtype=torch.float32, device="cuda")
    acc = torch.full((n_in + 1, d), float(POISON), dtype=torch.float32, device="cuda")
    pooled = torch.full((n_in + 1, d), float(POISON), dtype=torch.float32, device="cuda")
    got, outs = {}, []
    for li, (x, segs) in enumerate(case["launches"]):
        xd = torch.from_numpy(x).cuda()
        tab = torch.tensor(_table(segs), dtype=torch.int32, device="cuda")
        out = pooled
        if mode == pr.NONE:
            out = torch.full((x.shape[0] + 1, d), float(POISON), dtype=torch.float32, device="cuda")
        hip().pool(xd.data_ptr(), x.shape[0], x.shape[1], w.data_ptr(), float(case["eps"]), d, mode, normalize,
                   tab.data_ptr(), _table(segs), part.data_ptr(), part_rows, acc.data_ptr(), out.data_ptr(), n_in,
                   stream())
        torch.cuda.synchronize()
        assert torch.equal(xd.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)), "the input rows changed"
        if mode == pr.NONE:
            o = out.cpu().numpy()
            used = np.zeros(o.shape[0], bool)
            for (r0, n, *_rest) in segs:
                used[r0:r0 + n] = True
                for r in range(r0, r0 + n):
                    got[(li, r)] = o[r]
            assert (o[~used] == POISON).all(), "none: a row outside every segment was written"
        outs.append(out)
    bufs = {"part": part.cpu().numpy(), "acc": acc.cpu().numpy(), "pooled": pooled.cpu().numpy(), "need": need}
    if mode != pr.NONE:
        for (x, segs) in case["launches"]:
            for (r0, n, dst, flags, n_tok) in segs:
                if flags & pr.LAST:
                    got[dst] = bufs["pooled"][dst]
    return got, bufs


@pytest.mark.parametrize("d", pr.DS)
@pytest.mark.parametrize("name", pr.CASES)
def test_pool_against_fp64(torch_mod, name, d):
    case = pr.make_case(name, d)
    for mname, mode in pr.MODES.items():
        for normalize in (False, True):
            got, bufs = run_case(torch_mod, case, mode, normalize)
            worst = pr.check(got, pr.reference(case, mode, normalize))
            key = f"test_pool_gpu {name} d={d} {mname}{' l2' if normalize else ''}"
            _worst[key] = worst
            print(f"{key}: worst / bound = {worst:.4f}")
            # the sentinel rows: one past the inputs (accumulator, output), past the partial rows used
            assert (bufs["acc"][case["n_inputs"]] == POISON).all() and (bufs["pooled"][case["n_inputs"]] == POISON).all()
            if mode == pr.NONE:   # pool_rows alone writes, and only the rows
                assert (bufs["part"] == POISON).all() and (bufs["acc"] == POISON).all()
                assert (bufs["pooled"] == POISON).all()
            else:
                used = bufs["need"] if mode == pr.MEAN else max(len(s) for _, s in case["launches"])
                assert (bufs["part"][used:] == POISON).all(), "a partial row past the table's groups was written"
                assert np.isfinite(bufs["part"][:1]).all()


@pytest.mark.parametrize("mode", list(pr.MODES.values()))
def test_two_runs_are_bit_equal(torch_mod, mode):
    case = pr.make_case("carry", 4096)
    a, _ = run_case(torch_mod, case, mode, True)
    b, _ = run_case(torch_mod, case, mode, True)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{k}: two runs differ"


def test_unpooled_input_keeps_its_rows(torch_mod):
    """An input whose last piece has not arrived has no output row yet; an input with no piece in a
    launch keeps accumulator and output as they were."""
    torch = torch_mod
    case = pr.make_case("carry", 64)
    first_only = dict(case, launches=case["launches"][:1])
    got, bufs = run_case(torch, first_only, pr.MEAN, False)
    assert got == {} and (bufs["pooled"] == POISON).all()
    assert np.isfinite(bufs["acc"][:2]).all()


@pytest.mark.parametrize("bad", ["d66", "d0", "d_big", "ldx", "rows", "dst", "part", "twice", "mode"])
def test_refused_arguments_touch_nothing(torch_mod, bad):
    torch = torch_mod
    d = 66 if bad == "d66" else 0 if bad == "d0" else 16388 if bad == "d_big" else 64
    dd = max(d, 4)
    x = torch.full((8, dd), 1.0, dtype=torch.float32, device="cuda")
    w = torch.ones(dd, dtype=torch.float32, device="cuda")
    part = torch.full((4, dd), float(POISON), dtype=torch.float32, device="cuda")
    acc = torch.full((2, dd), float(POISON), dtype=torch.float32, device="cuda")
    out = torch.full((8, dd), float(POISON), dtype=torch.float32, device="cuda")
    segs = [0, 4, 0, 3, 4]
    rows, ldx, n_in, part_rows, mode = 8, dd, 2, 4, pr.MEAN
    if bad == "ldx":
        ldx = dd + 2
    elif bad == "rows":
        segs = [6, 4, 0, 3, 4]
    elif bad == "dst":
        segs = [0, 4, 2, 3, 4]
    elif bad == "part":
        segs, part_rows = [0, 8, 0, 3, 8, ], 0
    elif bad == "twice":
        segs = [0, 2, 0, 1, 4, 2, 2, 0, 2, 4]
    elif bad == "mode":
        mode = 4
    tab = torch.tensor(segs, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="pool"):
        hip().pool(x.data_ptr(), rows, ldx, w.data_ptr(), 1e-5, d, mode, True, tab.data_ptr(), segs, part.data_ptr(),
                   part_rows, acc.data_ptr(), out.data_ptr(), n_in, stream())
    torch.cuda.synchronize()
    for buf in (part, acc, out):
        assert (buf.cpu().numpy() == POISON).all(), "a refused call wrote"
    assert (x.cpu().numpy() == 1.0).all()


@pytest.mark.parametrize("mode", list(pr.MODES.values()))
def test_zero_vector_stays_zero_under_l2(torch_mod, mode):
    """A pooled vector (or row) whose sum of squares is 0 - here: an all-zero norm weight - is
    returned as zeros, not as NaN (upstream: norm > 0 ? 1 / norm : 0)."""
    case = pr.make_case("three", 64)
    case = dict(case, w=np.zeros_like(case["w"]))
    got, _ = run_case(torch_mod, case, mode, True)
    assert got and all((v == 0).all() for v in got.values())
