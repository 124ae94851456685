"""The normal-stream cases (stream_cases.py) exercise what they claim, and their CPU
reference is anchored to the reference's own output -- conditions on the inputs of
test_gpu_normal_stream.py, checked with NumPy and the oracle alone."""

import numpy as np
import pytest

import gsparse_oracle as O
import stream_cases as SC
from conftest import bits_equal, load_golden

REQUIRED_SEEDS = (0, 1, 7, 12345, 2 ** 63 + 5)


def test_table_holds_the_required_sizes_and_seeds():
    """need = m * k: 1; 3 * k for a k in 2..7; one below and one above 256; one below and
    one above 1,024; the large one.  Seeds: the required ones and 42."""
    needs = {case: SC.need(case) for case in SC.CASES}
    assert needs[("single_edge", 1)] == 1
    assert any(name == "triangle" and 2 <= k <= 7 and needs[(name, k)] == 3 * k
               for name, k in SC.CASES)
    assert needs[("karate_test", 3)] == 234 and needs[("karate_test", 4)] == 312
    assert needs[("karate_test", 13)] == 1014 and needs[("karate_test", 14)] == 1092
    assert SC.LARGE in SC.CASES and needs[SC.LARGE] == 2_100_400
    assert all(c in SC.CASES for c in SC.AROUND_1024)
    assert set(REQUIRED_SEEDS) <= set(SC.SEEDS) and 42 in SC.SEEDS


@pytest.mark.parametrize("seed", SC.SEEDS, ids=SC.seed_id)
def test_large_case_reaches_the_tail(seed):
    """At least 100 of the large case's normals are tail draws (|x| > kZigR), of both
    signs: the restated log1p and the tail's sign bit decide values the tests see."""
    x = SC.normals(SC.LARGE, seed).ravel()
    tail = x[np.abs(x) > SC.ZIG_R]
    assert len(tail) >= 100, len(tail)
    assert (tail > 0).any() and (tail < 0).any()


def test_reference_is_anchored_to_the_golden_scores():
    """Karate at the reference's own k, seed 42, 500 iterations: the scores of Z_ref are
    the golden's (made by the reference itself), bit for bit."""
    g = load_golden("karate_test")
    k = O.jl_dim(34, 0.3)
    Z, its = SC.reference(("karate_test", k), 42, 500)
    assert Z.shape == (34, k) and its.shape == (k,)
    assert bits_equal(O.er_from_z(g["indptr"], g["indices"], Z), g["scores_approx_er"])


def test_reference_sees_a_sign_flip_that_scores_do_not():
    """Why Z: negating one R column leaves every score as it was and changes Z."""
    case = ("karate_test", 4)
    n, ip, ix, d, m = SC.graph(case[0])
    Z, _ = SC.reference(case, 7)
    Zn = Z.copy()
    Zn[:, 2] = -Zn[:, 2]
    assert bits_equal(O.er_from_z(ip, ix, Zn), O.er_from_z(ip, ix, Z))
    assert not bits_equal(Zn, Z)


def test_reference_is_kept_and_read_only():
    Z, its = SC.reference(("triangle", 5), 1)
    assert SC.reference(("triangle", 5), 1)[0] is Z
    with pytest.raises(ValueError):
        Z[0, 0] = 0.0
