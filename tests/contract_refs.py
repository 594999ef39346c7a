"""NumPy statements of the contractions of include/mpsengine.h, written from the index expressions given there and from
nothing else (not from renormalizer_amd/csrc/mpse_plans.h, not from tests/host_emu): tensordot chains in float64 /
complex128, the references of tests/test_unit_channel_gpu.py and tests/test_ft_contract_gpu.py.
tests/test_contract_refs_host.py holds them against the host emulation of the plans at small shapes, without a GPU."""
import numpy as np

UP, DOWN = 0, 1      # MPSE_LEG_UP, MPSE_LEG_DOWN


def rand(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(b).max()))


# ---------------------------------------------------------------------------------------- one MPO layer, one leg
def ref_heff(l, r, ws, c):
    """mpse_heff_apply: 0-site abc,lbk,ck->al ; 1-site abc,bdef,lfk,cek->adl (ancilla cegk->adgl) ; 2-site
    abc,bdef,fghj,ljk,cehk->adgl (ancilla cemhnk->admgnl).  l (bra bond, channel, ket bond), r alike."""
    ns = len(ws)
    t = np.tensordot(l, c, axes=(2, 0))                          # a, b, then the indices of c after its left bond
    if ns == 0:                                                  # t[a, b, k]
        return np.tensordot(t, r, axes=([1, 2], [1, 2]))
    anc = c.ndim == 2 * ns + 2
    if ns == 1 and not anc:                                      # t[a, b, e, k]
        t = np.tensordot(t, ws[0], axes=([1, 2], [0, 2]))        # a, k, d, f
        return np.tensordot(t, r, axes=([3, 1], [1, 2]))         # a, d, l
    if ns == 1:                                                  # t[a, b, e, g, k]
        t = np.tensordot(t, ws[0], axes=([1, 2], [0, 2]))        # a, g, k, d, f
        t = np.tensordot(t, r, axes=([4, 2], [1, 2]))            # a, g, d, l
        return np.ascontiguousarray(t.transpose(0, 2, 1, 3))
    if not anc:                                                  # t[a, b, e, h, k]
        t = np.tensordot(t, ws[0], axes=([1, 2], [0, 2]))        # a, h, k, d, f
        t = np.tensordot(t, ws[1], axes=([4, 1], [0, 2]))        # a, k, d, g, j
        return np.tensordot(t, r, axes=([4, 1], [1, 2]))         # a, d, g, l
    t = np.tensordot(t, ws[0], axes=([1, 2], [0, 2]))            # t[a, b, e, m, h, n, k] -> a, m, h, n, k, d, f
    t = np.tensordot(t, ws[1], axes=([6, 2], [0, 2]))            # a, m, n, k, d, g, j
    t = np.tensordot(t, r, axes=([6, 3], [1, 2]))                # a, m, n, d, g, l
    return np.ascontiguousarray(t.transpose(0, 3, 1, 4, 2, 5))   # a, d, m, g, n, l


def ref_env(dom, env, ket, w, bra=None, bra_conj=True):
    """mpse_env_update: env (bra bond, channel, ket bond); ket (Dl, d[, danc], Dr); W (wl, d, d, wr), its first physical
    leg meets the bra; bra None = the ket; bra_conj False: the buffer holds the conjugated tensor already.
    L: out[p, f, h] = sum env[a, b, c] bra*[a, d, g, p] W[b, d, e, f] ket[c, e, g, h]
    R: out[p, q, h] = sum env[a, b, c] bra*[p, d, g, a] W[q, d, e, b] ket[h, e, g, c]      (g: the traced ancilla)"""
    b = ket if bra is None else bra
    if bra_conj:
        b = b.conj()
    if ket.ndim == 3:
        ket, b = ket[:, :, None, :], b[:, :, None, :]
    if dom == "L":
        x = np.tensordot(env, ket, axes=(2, 0))                  # a, b, e, g, h
        y = np.tensordot(x, w, axes=([1, 2], [0, 2]))            # a, g, h, d, f
        o = np.tensordot(b, y, axes=([0, 1, 2], [0, 3, 1]))      # p, h, f
    else:
        x = np.tensordot(ket, env, axes=(3, 2))                  # h, e, g, a, b
        y = np.tensordot(x, w, axes=([1, 4], [2, 3]))            # h, g, a, q, d
        o = np.tensordot(b, y, axes=([1, 2, 3], [4, 1, 2]))      # p, h, q
    return np.ascontiguousarray(o.transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------- two layers, two legs
def _layer(w, trans):
    """the MPO site as (left bond, leg out, leg in, right bond): W(trans = 0)[., x, y, .] maps leg[y] -> leg'[x]"""
    return w.transpose(0, 2, 1, 3) if trans else w


def _ft_left(l, w1, w2, legs, trans, c):
    """T[d, u', v', j, g, i] = sum L[a, b, c, d] C[a, u, v, j] (layer 1 on its leg) (layer 2 on its leg); c may carry
    trailing batch axes, which end up behind j"""
    a1, a2 = _layer(w1, trans[0]), _layer(w2, trans[1])
    t = np.tensordot(l, c, axes=(0, 0))                          # b, c, d, u, v, j, ...
    p = 3 if legs[0] == UP else 4
    t = np.tensordot(t, a1, axes=([0, p], [0, 2]))               # c, d, (the other leg), j, ..., x, g
    t = np.moveaxis(t, -2, p - 1)                                # c, d, u, v, j, ..., g
    p = 2 if legs[1] == UP else 3
    t = np.tensordot(t, a2, axes=([0, p], [0, 2]))               # d, (the other leg), j, ..., g, y, i
    return np.moveaxis(t, -2, p - 1)                             # d, u, v, j, ..., g, i


def ref_apply_ft(l, r, w1, w2, legs, trans, c):
    """mpse_heff_apply_ft: out[d, u', v', k] = sum L[a, b, c, d] C[a, u, v, j] (layer 1) (layer 2) R[j, g, i, k]; layer 1
    acts first; b / g the bonds of layer 1, c / i those of layer 2.  Trailing axes of c are a batch."""
    t = _ft_left(l, w1, w2, legs, trans, c)
    o = np.tensordot(t, r, axes=([3, -2, -1], [0, 1, 2]))        # d, u, v, ..., k
    return np.ascontiguousarray(np.moveaxis(o, -1, 3))


def ref_env_ft(dom, env, w1, w2, legs, trans, x):
    """mpse_env_update_ft, bra = conj(X); output (ket bond, layer 1, layer 2, bra bond)"""
    xc = x.conj()
    if dom == "L":                                               # env (a, b, c, d) -> (j, g, i, k)
        t = _ft_left(env, w1, w2, legs, trans, x)
        return np.tensordot(t, xc, axes=([0, 1, 2], [0, 1, 2]))
    a1, a2 = _layer(w1, trans[0]), _layer(w2, trans[1])
    s = np.tensordot(x, env, axes=(3, 0))                        # a, u, v, g, i, k
    p = 1 if legs[0] == UP else 2
    s = np.tensordot(s, a1, axes=([p, 3], [2, 3]))               # a, (the other leg), i, k, b, x
    s = np.moveaxis(s, -1, p)                                    # a, u, v, i, k, b
    p = 1 if legs[1] == UP else 2
    s = np.tensordot(s, a2, axes=([p, 3], [2, 3]))               # a, (the other leg), k, b, c, y
    s = np.moveaxis(s, -1, p)                                    # a, u, v, k, b, c
    return np.tensordot(s, xc, axes=([1, 2, 3], [1, 2, 3]))      # a, b, c, d


def dense_ft(l, r, w1, w2, legs, trans, shape, chunk=128):
    """the term as a dense matrix on the centre space of `shape`: the reference applied to every unit vector"""
    n = int(np.prod(shape))
    dt = np.result_type(l.dtype, r.dtype, w1.dtype)
    eye = np.eye(n, dtype=dt)
    cols = []
    for k0 in range(0, n, chunk):
        e = np.ascontiguousarray(eye[:, k0:k0 + chunk]).reshape(tuple(shape) + (-1,))
        cols.append(ref_apply_ft(l, r, w1, w2, legs, trans, e).reshape(n, -1))
    return np.concatenate(cols, axis=1)
