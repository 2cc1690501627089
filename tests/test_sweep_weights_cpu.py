"""chebyshev_weights (EXTENSION, no reference counterpart): the sweep weights of a Chebyshev smoothing schedule are the
reciprocals of the roots of the degree-d Chebyshev polynomial moved to [lo, hi] = [lam_max / ratio, safety * lam_max].
Checked against the closed form and against the property that defines them: over [lo, hi] the error polynomial
prod_j (1 - w_j lam) of d weighted sweeps attains the Chebyshev bound 1 / T_d((hi + lo) / (hi - lo)) and nothing
larger.  No device."""
import numpy as np
import pytest

import agglomerationmultigrid1d_amd as mg


def closed_form(lam, degree, ratio, safety):
    hi, lo = safety * lam, lam / ratio
    return np.array([1.0 / (0.5 * (hi + lo) + 0.5 * (hi - lo) * np.cos(np.pi * (2 * j + 1) / (2 * degree)))
                     for j in range(degree)])


def test_closed_form_and_the_documented_example():
    for lam in (0.3, 1.0, 1.99, 7.5):
        for degree in range(1, 9):
            for ratio in (3.0, 10.0, 30.0):
                for safety in (1.0, 1.05, 1.3):
                    w = mg.chebyshev_weights(lam, degree=degree, ratio=ratio, safety=safety)
                    assert isinstance(w, np.ndarray) and w.dtype == np.float64 and w.shape == (degree,)
                    np.testing.assert_allclose(w, closed_form(lam, degree, ratio, safety), rtol=1e-15, atol=0.0)
    # the defaults: degree 3, ratio 10, safety 1.05 -- the weights DESIGN.md quotes for lam = 1.99
    np.testing.assert_allclose(mg.chebyshev_weights(1.99), [0.509, 0.873, 3.07], rtol=2e-3)
    np.testing.assert_array_equal(mg.chebyshev_weights(1.99), mg.chebyshev_weights(1.99, degree=3, ratio=10.0, safety=1.05))
    # scaling: the weights of c * lam are the weights of lam over c
    np.testing.assert_allclose(mg.chebyshev_weights(4.0), mg.chebyshev_weights(1.0) / 4.0, rtol=1e-15)


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("ratio", [3.0, 10.0, 30.0])
def test_error_polynomial_attains_the_chebyshev_bound(degree, ratio):
    lam, safety = 1.99, 1.05
    hi, lo = safety * lam, lam / ratio
    w = mg.chebyshev_weights(lam, degree=degree, ratio=ratio, safety=safety)
    # a fine grid that holds the end points and, exactly enough, the interior extrema (Chebyshev extrema of the interval)
    grid = np.concatenate([np.linspace(lo, hi, 200001),
                           0.5 * (hi + lo) + 0.5 * (hi - lo) * np.cos(np.pi * np.arange(degree + 1) / degree)])
    poly = np.ones_like(grid)
    for wj in w:
        poly *= 1.0 - wj * grid
    x = (hi + lo) / (hi - lo)
    bound = 1.0 / np.cosh(degree * np.arccosh(x))          # 1 / T_d(x), x > 1
    assert abs(np.max(np.abs(poly)) - bound) <= 1e-12
    # ... and outside the interval, towards zero, it tends to 1: no eigenvalue below lo is amplified
    small = np.linspace(0.0, lo, 1001)
    ps = np.ones_like(small)
    for wj in w:
        ps *= 1.0 - wj * small
    assert np.all(ps <= 1.0 + 1e-15) and np.all(ps >= bound - 1e-12)


def test_order_is_ascending_and_positive():
    for degree in range(1, 9):
        for ratio in (1.5, 3.0, 10.0, 30.0):
            w = mg.chebyshev_weights(2.0, degree=degree, ratio=ratio)
            assert np.all(w > 0.0)
            assert np.all(np.diff(w) > 0.0), "the smallest weight comes first"
            # every weight is the reciprocal of a point of the interval
            assert 1.0 / w[0] <= 1.05 * 2.0 and 1.0 / w[-1] >= 2.0 / ratio


@pytest.mark.parametrize("kw", [dict(lam_max=0.0), dict(lam_max=-1.0), dict(lam_max=float("nan")), dict(lam_max=float("inf")),
                                dict(degree=0), dict(degree=-2), dict(degree=2.5), dict(ratio=1.0), dict(ratio=0.5),
                                dict(ratio=float("nan")), dict(safety=0.9), dict(safety=float("inf"))])
def test_argument_errors(kw):
    args = dict(lam_max=2.0)
    args.update(kw)
    with pytest.raises(mg.ArgumentError):
        mg.chebyshev_weights(**args)
