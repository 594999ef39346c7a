"""NumPy references and state builders for the Schmidt weights of the bonds of a chain (``mpse_mps_bond_spectra``),
shared by tests/test_bond_spectra_host.py and tests/test_bond_spectra_gpu.py.  Sites are arrays (D_l, d[, danc], D_r);
an ancilla leg counts as part of the physical one.  Bond k lies between the sites k and k + 1."""
import numpy as np


def _a3(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], -1, a.shape[-1])


def dense_spectra(sites):
    """[p of bond k for k < N - 1], p = sigma^2 in descending order from ``numpy.linalg.svd`` of the dense state
    reshaped at the bond: min(left, right) values each.  The reference for everything else."""
    mats = [_a3(a) for a in sites]
    psi = mats[0]
    for m in mats[1:]:
        psi = np.tensordot(psi, m, axes=(-1, 0))
    psi = psi.reshape(psi.shape[1:-1])
    out, left = [], 1
    for k in range(len(mats) - 1):
        left *= psi.shape[k]
        out.append(np.linalg.svd(psi.reshape(left, -1), compute_uv=False) ** 2)
    return out


def environments(sites):
    """(L, R): L[k] / R[k] the identity-operator environment left / right of bond k, first index from the conjugated
    tensor"""
    mats = [_a3(a) for a in sites]
    left, e = [], np.ones((1, 1))
    for a in mats[:-1]:
        e = np.einsum("bc,bsd,cse->de", e, a.conj(), a, optimize=True)
        left.append(e)
    right, e = [], np.ones((1, 1))
    for a in mats[:0:-1]:
        e = np.einsum("bsd,cse,de->bc", a.conj(), a, e, optimize=True)
        right.append(e)
    return left, right[::-1]


def gram_spectra(sites):
    """The algorithm of the engine restated: per bond L = U Lambda U^H, M = Lambda^(1/2) U^H R^T U Lambda^(1/2), p =
    eig(M) clamped at 0, descending: D_k values each"""
    out = []
    for L, R in zip(*environments(sites)):
        lam, u = np.linalg.eigh((L + L.conj().T) / 2)
        root = np.sqrt(np.clip(lam, 0, None))
        m = root[:, None] * (u.conj().T @ R.T @ u) * root[None, :]
        p = np.linalg.eigvalsh((m + m.conj().T) / 2)
        out.append(np.sort(np.clip(p, 0, None))[::-1])
    return out


def padded(rows, width=None):
    """the rows as one array, each padded with zeros (or cut: what is cut must be zero to 1e-14) to ``width``"""
    width = max(len(r) for r in rows) if width is None else width
    out = np.zeros((len(rows), width))
    for i, r in enumerate(rows):
        r = np.asarray(r)
        assert np.all(np.abs(r[width:]) < 1e-14), r
        out[i, :min(width, len(r))] = r[:width]
    return out


def entropy(p):
    p = np.asarray(p, dtype=float)
    p = p / p.sum()
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def _rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def _isometry(rng, m, n, cplx):
    return np.linalg.qr(_rand(rng, (m, n), cplx))[0]


def scramble(rng, sites, cplx):
    """X and X^-1 inserted at every bond, X = Q1 diag(0.5 .. 2) Q2 with random orthogonal / unitary Q: the state is the
    same, no environment is the identity"""
    sites = [np.array(a, dtype=complex if cplx else float) for a in sites]
    for j in range(len(sites) - 1):
        D = sites[j].shape[-1]
        x = _isometry(rng, D, D, cplx) @ np.diag(rng.uniform(0.5, 2.0, D)) @ _isometry(rng, D, D, cplx)
        sites[j] = np.tensordot(sites[j], x, axes=(-1, 0))
        sites[j + 1] = np.tensordot(np.linalg.inv(x), sites[j + 1], axes=(1, 0))
    return sites


def chain_of_dense(psi, ds, bonds):
    """the dense state psi (all physical legs, in order) as a chain with the bond profile ``bonds``: SVD sweep from the
    left; a bond wider than the rank is padded with exact zeros, one narrower must lose nothing"""
    sites, rest = [], np.asarray(psi).reshape(1, -1)
    for i, d in enumerate(ds[:-1]):
        Dl, Dr = bonds[i], bonds[i + 1]
        u, s, vh = np.linalg.svd(rest.reshape(Dl * d, -1), full_matrices=False)
        assert np.all(s[Dr:] < 1e-13 * s[0]), (i, s)
        keep = min(Dr, len(s))
        a = np.zeros((Dl * d, Dr), dtype=u.dtype)
        a[:, :keep] = u[:, :keep]
        rest = np.zeros((Dr, vh.shape[1]), dtype=u.dtype)
        rest[:keep] = s[:keep, None] * vh[:keep]
        sites.append(a.reshape(Dl, d, Dr))
    sites.append(rest.reshape(bonds[-2], ds[-1], 1))
    return sites


def state_with_spectrum(rng, bonds, ds, cut, p, kind="real", gauge=True):
    """A chain with the bond profile ``bonds`` and physical extents ``ds`` whose dense state has the Schmidt weights
    ``p`` (zeros behind them) at bond ``cut``: random sites, isometries left and right of the cut (QR), and the centre
    matrix U diag(sqrt p) V^H with random orthogonal / unitary U, V between them - psi = sum_ab |a> C[a, b] |b> with
    orthonormal |a>, |b>.  Then the gauge is scrambled at every bond.  kind: "real", "complex", or "mixed" (a real
    state, then a random unitary on the physical leg of every odd site, which leaves every spectrum alone and makes
    those sites complex)."""
    cplx = kind == "complex"
    n, D = len(ds), bonds[cut + 1]
    p = np.asarray(p, dtype=float)
    assert len(p) <= D
    sites = [_rand(rng, (bonds[i], ds[i], bonds[i + 1]), cplx) for i in range(n)]
    for i in range(cut + 1):
        Dl, d, Dr = sites[i].shape
        assert Dl * d >= Dr
        q, r = np.linalg.qr(sites[i].reshape(Dl * d, Dr))
        sites[i] = q.reshape(Dl, d, Dr)
        if i < cut:
            sites[i + 1] = np.tensordot(r, sites[i + 1], axes=(1, 0))
    for i in range(n - 1, cut, -1):
        Dl, d, Dr = sites[i].shape
        assert d * Dr >= Dl
        q, r = np.linalg.qr(sites[i].reshape(Dl, d * Dr).conj().T)
        sites[i] = q.conj().T.reshape(Dl, d, Dr)
        if i > cut + 1:
            sites[i - 1] = np.tensordot(sites[i - 1], r.conj().T, axes=(-1, 0))
    root = np.zeros(D)
    root[:len(p)] = np.sqrt(p)
    centre = (_isometry(rng, D, D, cplx) * root) @ _isometry(rng, D, D, cplx).conj().T
    sites[cut] = np.tensordot(sites[cut], centre, axes=(-1, 0))
    if gauge:
        sites = scramble(rng, sites, cplx)
    if kind == "mixed":
        for j in range(1, len(sites), 2):
            sites[j] = np.einsum("pq,aqb->apb", _isometry(rng, ds[j], ds[j], True), sites[j])
    return [np.ascontiguousarray(a) for a in sites]


def decaying(n, smallest=1e-5):
    """n normalised weights, geometric from 1 down to ``smallest``"""
    p = np.geomspace(1.0, smallest, n) if n > 1 else np.ones(1)
    return p / p.sum()
