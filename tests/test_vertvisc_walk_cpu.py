"""The two arithmetic identities the lean coefficient walk of vert_friction.hip (CoefWalk::layer<true>) rests on, as plain IEEE
float64 arithmetic: with H_to_Z == 1.0 the vertical extents dz = H_to_Z * h ARE the thicknesses, so the harmonic mean of the dz is
the harmonic mean of the h in every bit, and the upwinding's z2 = z2_wt * z with z2_wt == 1.0 is z itself."""
import numpy as np

N = 1 << 21


def _operands(seed):
    """Random magnitudes over the whole exponent range next to the edge cases: zeros, subnormals, huge values, equal pairs."""
    rng = np.random.default_rng(seed)
    tiny = np.finfo(np.float64).tiny
    edge = np.array([0.0, -0.0, 5e-324, tiny / 4, tiny, 1e-300, 1e-30, 1e-20, 1e-10, 1e-9, 1.0, 1.0 + 2.0 ** -52, 3.0, 1e10, 1e150,
                     1e300, np.finfo(np.float64).max])
    a = np.concatenate([10.0 ** rng.uniform(-320, 308, N), rng.uniform(0.0, 1.0, N), np.repeat(edge, edge.size)])
    b = np.concatenate([10.0 ** rng.uniform(-320, 308, N), rng.uniform(0.0, 1.0, N), np.tile(edge, edge.size)])
    eq = rng.random(a.size) < 0.05
    b = np.where(eq, a, b)   # h0 == h1: h_delta == 0
    return a, b


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def test_one_times_x_is_x_in_every_bit():
    a, b = _operands(1)
    for x in (a, b, -a, -b, np.array([np.inf, -np.inf])):
        assert np.array_equal(_bits(1.0 * x), _bits(x))
    assert (a == 0).any() and ((a > 0) & (a < np.finfo(np.float64).tiny)).any()


def test_harmonic_mean_of_dz_is_that_of_h_when_H_to_Z_is_one():
    a, b = _operands(2)
    one = np.float64(1.0)
    for n in (1e-30, 1e-37, 0.0):   # H_subroundoff == dZ_subroundoff of an unscaled Boussinesq run (abi.vgrid_default: 1e-30)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
            dz0, dz1 = one * a, one * b
            h_harm = 2. * a * b / (a + b + n)
            dz_harm = 2. * dz0 * dz1 / (dz0 + dz1 + n)
            h_arith, dz_arith = 0.5 * (b + a), 0.5 * (dz1 + dz0)
        assert np.array_equal(_bits(dz_harm), _bits(h_harm))
        assert np.array_equal(_bits(dz_arith), _bits(h_arith))
    assert np.isfinite(h_harm).sum() > N
