"""Host-side premise of the Kronecker-sum tests (tests/kron_problems.py): the environment / MPO form is the Kronecker
sum for bond, one- and two-site centres, its spectrum is the sums of the factor eigenvalues, the shift moves it, and
Kron.expm is exp(dt H) of the dense operator."""
import numpy as np
import scipy.linalg

from oracle import mps_oracle as orc

from kron_problems import _rand, kron_problem   # (tests/kron_problems.py)


def test_kron_forms_and_exponential():
    for dims, cplx, shift in (((5, 3, 4), True, 0.0), ((4, 3, 2, 5), False, 0.0), ((6, 7), True, 0.0),
                              ((3, 2, 4), True, -40.0), ((4, 5), False, 25.0)):
        k = kron_problem(1, dims, cplx, shift=shift)
        h = orc.hop_dense(k.l, k.r, k.cmo)
        x = _rand(np.random.default_rng(0), (k.n,), cplx)
        assert np.abs(h @ x - k.apply(x)).max() < 1e-12 * max(1.0, abs(shift))
        assert np.abs(h - h.conj().T).max() < 1e-12 * max(1.0, abs(shift))
        vals, idx = k.spectrum()
        assert np.abs(np.linalg.eigvalsh(h) - vals).max() < 1e-11 * max(1.0, abs(shift))
        v = k.vector(idx[1])
        assert np.abs(h @ v - vals[1] * v).max() < 1e-11 * max(1.0, abs(shift))
        for dt in (-0.7j, 0.3, -0.3, 0.2 - 0.5j):
            ref = scipy.linalg.expm(dt * h) @ x
            assert np.linalg.norm(k.expm(dt, x) - ref) <= 1e-12 * np.linalg.norm(ref) * max(1.0, abs(dt * shift))


def test_kron_default_problem_unchanged():
    """the helper draws the problems the Davidson tests drew before it moved here: entries [1, 0] of every factor and
    the sum of all |entries|, recorded from the earlier helper"""
    pinned = (
        ((7, (5, 4, 6), True), [-0.06841409056755508 + 0.006969846857547141j, 0.053717873710217565,
                                0.0008430029056729401 + 0.01891290677713454j], 27.074884495995917),
        ((70, (4, 3, 2, 5), False), [-0.13802840251628207, 0.009945046493449745, 0.03592373496999054,
                                     -0.02674283827424899], 13.715175050488453),
    )
    for args, entries, total in pinned:
        k = kron_problem(*args)
        for f, e in zip(k.f, entries):
            assert abs(f[1, 0] - e) <= 1e-15
        assert abs(sum(np.abs(f).sum() for f in k.f) - total) <= 1e-12
