"""The embedding epilogue's reference, bound and checker (tests/pool_ref.py) against themselves:
the fp32 emulation of the kernels' own order of additions stays within HALF the derived bound on
exactly the GPU test's inputs, and every planted single defect is rejected."""
import numpy as np
import pytest

import pool_ref as pr


@pytest.mark.parametrize("d", pr.DS)
@pytest.mark.parametrize("name", pr.CASES)
def test_emulation_within_half_the_bound(name, d):
    case = pr.make_case(name, d)
    for mode in pr.MODES.values():
        for normalize in (False, True):
            ref = pr.reference(case, mode, normalize)
            assert ref, "the case completes no input"
            worst = pr.check(pr.emulate(case, mode, normalize), ref)
            assert worst <= 0.5, f"{name} d={d} mode={mode} normalize={normalize}: worst / bound = {worst:.3f}"


def test_reference_is_the_plain_formula():
    """reference() against the formula written out directly, for one input of one piece."""
    case = pr.make_case("five", 288)
    x, segs = case["launches"][0]
    r0, n, dst = segs[4][:3]
    rows = x[r0:r0 + n, :288].astype(np.float64)
    normed = rows / np.sqrt((rows ** 2).mean(-1, keepdims=True) + case["eps"]) * case["w"].astype(np.float64)
    for mode, want in ((pr.MEAN, normed.mean(0)), (pr.CLS, normed[0]), (pr.LAST_MODE, normed[-1])):
        v, b = pr.reference(case, mode, False)[dst]
        assert np.allclose(v, want, rtol=1e-13, atol=0) and (b > 0).all()
        v, _ = pr.reference(case, mode, True)[dst]
        assert np.allclose(v, want / np.linalg.norm(want), rtol=1e-13, atol=0)
    rowsref = pr.reference(case, pr.NONE, True)
    assert np.allclose(rowsref[(0, r0 + 5)][0], normed[5] / np.linalg.norm(normed[5]), rtol=1e-13, atol=0)
    assert len(rowsref) == 1 + 63 + 64 + 65 + 130


def test_carry_case_adds_both_pieces():
    case = pr.make_case("carry", 64)
    (x1, s1), (x2, s2) = case["launches"]
    rows = np.concatenate([x1[s1[0][0]:s1[0][0] + 70, :64], x2[s2[1][0]:s2[1][0] + 60, :64]]).astype(np.float64)
    normed = rows / np.sqrt((rows ** 2).mean(-1, keepdims=True) + case["eps"]) * case["w"].astype(np.float64)
    assert np.allclose(pr.reference(case, pr.MEAN, False)[0][0], normed.mean(0), rtol=1e-13, atol=0)
    assert np.allclose(pr.reference(case, pr.LAST_MODE, False)[0][0], normed[-1], rtol=1e-13, atol=0)
    assert np.allclose(pr.reference(case, pr.CLS, False)[0][0], normed[0], rtol=1e-13, atol=0)


# (defect, case, d, mode, normalize): where the defect shows - no_eps at the d whose eps is half a
# row's mean square, the chunk / carry defects where an input arrives in two pieces
PLANTED = [
    ("drop_last_row", "five", 64, pr.MEAN, False),
    ("drop_last_row", "three", 4096, pr.MEAN, True),
    ("group_twice", "five", 2048, pr.MEAN, False),
    ("neighbour_row", "five", 64, pr.MEAN, False),
    ("neighbour_row", "three", 288, pr.MEAN, True),
    ("div_chunk_rows", "carry", 64, pr.MEAN, False),
    ("no_eps", "five", 288, pr.MEAN, False),
    ("no_eps", "five", 288, pr.LAST_MODE, False),
    ("no_eps", "three", 288, pr.NONE, False),
    ("no_weight", "five", 64, pr.MEAN, True),
    ("no_weight", "three", 8192, pr.CLS, False),
    ("l2_before_mean", "five", 64, pr.MEAN, True),
    ("last_chunk_row", "carry", 2048, pr.LAST_MODE, False),
    ("last_chunk_row", "three", 64, pr.LAST_MODE, True),
    ("no_carry", "carry", 64, pr.MEAN, False),
    ("no_carry", "carry", 288, pr.CLS, False),
]


@pytest.mark.parametrize("defect,name,d,mode,normalize", PLANTED)
def test_planted_defect_is_rejected(defect, name, d, mode, normalize):
    case = pr.make_case(name, d, guard=False)   # finite guard rows: the defect itself must be seen
    ref = pr.reference(case, mode, normalize)
    assert pr.check(pr.emulate(case, mode, normalize), ref) <= 0.5
    with pytest.raises(AssertionError):
        pr.check(pr.emulate(case, mode, normalize, defect), ref)


def test_every_defect_is_planted():
    assert {p[0] for p in PLANTED} == set(pr.DEFECTS)


def test_non_finite_output_is_rejected():
    case = pr.make_case("five", 64)
    got = pr.emulate(case, pr.MEAN, False)
    got[2] = got[2].copy()
    got[2][7] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        pr.check(got, pr.reference(case, pr.MEAN, False))
