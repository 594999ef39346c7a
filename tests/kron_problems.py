"""Kronecker-sum centre problems with exactly known spectra, shared by the Davidson and Lanczos tests.

H = A x 1 x 1 + 1 x B x 1 + 1 x 1 x R (one site), the two-site form with four factors and the bond form (two factors,
no MPO site) are built from environments and MPO sites, so the engine applies them like any other effective
Hamiltonian, while every eigenpair - and with them exp(dt H) C - follows from the small factors."""
import numpy as np


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return a


def _factor(rng, evals, cplx, eps=0.3, charges=None):
    """Hermitian matrix with the given spectrum, close to diagonal (a rotation by a small random generator); with
    ``charges`` block-diagonal: it only mixes indices of equal charge.  Returns (matrix, its exact eigenvectors as
    columns, eigenvalues) - the eigenvalues are those of the returned matrix to rounding."""
    n = len(evals)
    g = _rand(rng, (n, n), cplx) * (eps / np.sqrt(n))
    g = (g - g.conj().T) / 2                           # anti-Hermitian generator
    if charges is not None:
        g = g * (charges[:, None] == charges[None, :])
    ew, ev = np.linalg.eigh(1j * g)                    # g = -i (i g), i g Hermitian
    u = (ev * np.exp(-1j * ew)) @ ev.conj().T          # exp(g): unitary, real orthogonal for a real g
    if not cplx:
        u = u.real
    m = (u * evals) @ u.conj().T
    m = (m + m.conj().T) / 2
    return m, u, np.asarray(evals, dtype=float)


class Kron:
    """Bond, one- or two-site centre whose effective Hamiltonian is a Kronecker sum of Hermitian factors, one per index
    of the centre: L = (F0, 1, .., 1), the MPO sites diagonal in their channels with F_i in channel i, R = (1, .., F_last).
    The eigenvalues are all sums of factor eigenvalues, the eigenvectors Kronecker products of factor eigenvectors."""

    def __init__(self, factors, cplx_env):
        self.f = [m for m, _, _ in factors]
        self.u = [u for _, u, _ in factors]
        self.ev = [e for _, _, e in factors]
        dims = [m.shape[0] for m in self.f]
        self.shape = tuple(dims)
        nf = len(dims)
        Dl, Dr = dims[0], dims[-1]
        self.l = np.zeros((Dl, nf, Dl), dtype=complex if cplx_env else float)
        self.r = np.zeros((Dr, nf, Dr), dtype=complex if cplx_env else float)
        for ch in range(nf):
            self.l[:, ch, :] = self.f[0] if ch == 0 else np.eye(Dl)
            self.r[:, ch, :] = self.f[-1] if ch == nf - 1 else np.eye(Dr)
        self.cmo = []
        for i, d in enumerate(dims[1:-1]):
            w = np.zeros((nf, d, d, nf))
            for ch in range(nf):
                w[ch, :, :, ch] = self.f[i + 1].real if ch == i + 1 else np.eye(d)
            self.cmo.append(w)
        self.n = int(np.prod(dims))

    def spectrum(self, allowed=None):
        """all eigenvalues with their factor indices, ascending; ``allowed(idx)`` filters the index tuples"""
        grids = np.meshgrid(*self.ev, indexing="ij")
        tot = sum(grids).ravel()
        order = np.argsort(tot, kind="stable")
        idx = np.array(np.unravel_index(order, self.shape)).T
        vals = tot[order]
        if allowed is not None:
            keep = np.array([allowed(t) for t in idx], dtype=bool)
            vals, idx = vals[keep], idx[keep]
        return vals, idx

    def vector(self, ix):
        v = self.u[0][:, ix[0]]
        for u, i in zip(self.u[1:], ix[1:]):
            v = np.kron(v, u[:, i])
        return v

    def diag(self):
        out = 0
        for i, m in enumerate(self.f):
            shp = [1] * len(self.shape)
            shp[i] = self.shape[i]
            out = out + np.real(np.diag(m)).reshape(shp)
        return out.ravel()

    def apply(self, x):
        x = x.reshape(self.shape)
        out = np.zeros_like(x, dtype=np.result_type(x, *self.f))
        for i, m in enumerate(self.f):
            out += np.moveaxis(np.tensordot(m, x, ([1], [i])), 0, i)
        return out.ravel()

    def _each_factor(self, x, mats):
        x = x.reshape(self.shape)
        for i, m in enumerate(mats):
            x = np.moveaxis(np.tensordot(m, x, ([1], [i])), 0, i)
        return x

    def expm(self, dt, x):
        """exp(dt H) x in float64 from the factor eigendecompositions: x goes to the product eigenbasis, each
        component is multiplied by exp(dt * sum of factor eigenvalues), and comes back"""
        y = self._each_factor(np.asarray(x, dtype=complex), [u.conj().T for u in self.u])
        grids = np.meshgrid(*self.ev, indexing="ij")
        y = y * np.exp(complex(dt) * sum(grids))
        return self._each_factor(y, self.u).ravel()


def kron_problem(seed, dims, cplx, degenerate=None, eps=0.3, charges=None, shift=0.0, spacing=None):
    """Kron centre with well separated factor spectra (spacings differ between factors so that low sums do not
    coincide unless ``degenerate`` = (factor, level) repeats a level of that factor on purpose).  ``shift`` is added
    to the eigenvalues of the first factor: H + shift; ``spacing`` replaces the level spacings of the factors."""
    rng = np.random.default_rng(seed)
    spacing = [0.71, 0.43, 0.59, 0.37] if spacing is None else spacing
    fs = []
    for i, n in enumerate(dims):
        ev = np.sort(spacing[i] * np.arange(n) + 0.013 * (i + 1) + rng.uniform(0, 0.05, n) * np.arange(n) / n)
        if degenerate is not None and degenerate[0] == i:
            ev[degenerate[1] + 1] = ev[degenerate[1]]
        if i == 0:
            ev = ev + shift
        # B (the MPO factors) is real; the bond factors follow the environment dtype
        fcplx = cplx and (i == 0 or i == len(dims) - 1)
        fs.append(_factor(rng, ev, fcplx, eps, None if charges is None else charges[i]))
    return Kron(fs, cplx)
