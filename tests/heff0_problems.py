"""Problems for the fused bond / two-level-site matvec (k_heff0_fused, csrc/mpse_heff0.hip), built on the host with numpy
only: operands with an explicit 16 x 16 tile pattern per MPO channel, a census of the structure the kernel's bookkeeping
has to find in them, and the float64 reference ``exp(dt H) c`` by the oracle's Krylov solve over ``hop_apply``.

The operator of a bond matrix is ``H = sum_b L_b (x) R_b`` (abc,lbk,ck->al, mps/hop_expr.py:63-67); it is Hermitian because
its channels are
  ("IH", Rmap)        identity (x) Hermitian,
  ("HI", Lmap)        Hermitian (x) identity,
  ("HH", Lmap, Rmap)  Hermitian (x) Hermitian,
  ("pair", Lmap, Rmap) TWO channels (L, R), (L^H, R^H) - the tile patterns of L and R are then free,
  ("zero",)           a channel of zeros on both sides.
A map is an integer array over the tiles of the matrix: 0 = no data, FULL = random complex entries in the whole tile,
CORNER = one random complex entry at element (15, 15), CORNER_IMAG = the same, purely imaginary.  Entries are scaled by
1 / (4 sqrt(D)) as in test_engine_gpu.py.  A Hermitian block is x + x^H of the block its map gives.

The operator of a one-site centre with a two-level physical index is ``H = sum_{b, f} L_b (x) W[b, :, :, f] (x) R_f``
(abc,bdef,lfk,cek->adl, hop_expr.py:75-79) with every L_b and R_f Hermitian (or the identity) and every 2 x 2 block of the
real MPO site symmetric, so that each summand is Hermitian by itself.

With ``sectors = (sl, sr)`` (an integer per bond index) the centre lives where ``sl[a] == sr[k]`` and the problem carries
the quantum numbers that make ``centre_tile_mask`` say so; the maps of such a case keep that structure (secmap).

The census (``census``) reads the arrays with plain loops and shares no code with the engine.  Units are the kernel's:
(bra tile row at, right channel f, 64-column ket chunk kc, value x of the physical index of the result).
"""
import numpy as np

from oracle import mps_oracle as orc

FULL, CORNER, CORNER_IMAG = 1, 2, 3
OPS = [np.eye(2), np.array([[0.0, 1.0], [1.0, 0.0]]), np.diag([0.0, 1.0]), np.array([[0.3, -0.7], [-0.7, 0.1]])]


# ---------------------------------------------------------------------------------------------------- tile maps

def band(nt, k):
    i = np.arange(nt)
    return (np.abs(i[:, None] - i[None, :]) <= k).astype(int)


def row_counts(nt, counts, stride=1):
    """tile row i holds min(counts[i % len(counts)], nt) tiles, starting at column i * stride (cyclic)"""
    m = np.zeros((nt, nt), int)
    for i in range(nt):
        for j in range(min(counts[i % len(counts)], nt)):
            m[i, (i * stride + j) % nt] = FULL
    return m


def lattice(nt, p, q, r, mod):
    i = np.arange(nt)
    return ((p * i[:, None] + q * i[None, :] + r) % mod == 0).astype(int)


def tile_sectors(sec):
    """sector of each 16-row tile (the sectors of these problems change at multiples of 16 only)"""
    sec = np.asarray(sec)
    t = sec.reshape(-1, 16)
    assert (t == t[:, :1]).all()
    return t[:, 0]


def secmap(sec, shift):
    """tile (i, j) holds data where (sector of rows i + shift) % 2 == sector of columns j"""
    st = tile_sectors(sec)
    return ((st[:, None] + shift) % 2 == st[None, :]).astype(int)


def cut(D, tile):
    """two sectors: 0 below row 16 * tile, 1 from there on"""
    return (np.arange(D) >= 16 * min(max(tile, 1), D // 16 - 1)).astype(int)


# ---------------------------------------------------------------------------------------------------- operands

def _fill(rng, D, tmap):
    tmap = np.asarray(tmap)
    assert tmap.shape == (D // 16, D // 16), (tmap.shape, D)
    x = np.zeros((D, D), complex)
    s = 1.0 / (4 * np.sqrt(D))
    for i, j in zip(*np.nonzero(tmap)):
        mode = tmap[i, j]
        if mode == FULL:
            x[16 * i:16 * i + 16, 16 * j:16 * j + 16] = (rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))) * s
        elif mode == CORNER:
            x[16 * i + 15, 16 * j + 15] = (rng.standard_normal() + 1j * rng.standard_normal()) * s
        else:
            x[16 * i + 15, 16 * j + 15] = 1j * rng.standard_normal() * s
    return x


def _herm(rng, D, tmap):
    x = _fill(rng, D, tmap)
    return x + x.conj().T


class Problem:
    """l (Dl, wl, Dl), r (Dr, wr, Dr), cmo ([] or [real MPO site (wl, 2, 2, wr)]), centre c, dt;
    allowed / qn: where the centre may hold data and the (qnbigl, qnbigr, qntot) of centre_tile_mask, or None;
    census: see ``census``"""

    def __init__(self, l, r, cmo, c, dt, allowed, qn):
        self.l, self.r, self.cmo, self.c, self.dt, self.allowed, self.qn = l, r, cmo, c, dt, allowed, qn
        self.census = census(l, r, cmo[0] if cmo else None, allowed)
        # exp(dt H) c holds c itself: the centre is empty where no unit writes, and so is every vector of the solve
        self.c[self.must_be_zero] = 0.0

    @property
    def must_be_zero(self):
        """elements of every vector of the solve that are exactly 0: output tiles that no unit holds, and everything
        outside the quantum-number blocks"""
        z = np.zeros(self.c.shape, bool)
        for at, lt in self.census["unheld"]:
            z[16 * at:16 * at + 16, ..., 16 * lt:16 * lt + 16] = True
        if self.allowed is not None:
            z |= ~self.allowed
        return z

    def apply(self, y):
        return orc.hop_apply(self.l, self.r, self.cmo, y.reshape(self.c.shape)).ravel()

    def reference(self, margins=None):
        """(exp(dt H) c as a vector, Krylov dimension) by the oracle"""
        return orc.expm_krylov(self.apply, self.dt, self.c.ravel(), margins=margins)

    def dense(self):
        """H[(out indices), (in indices)] assembled by einsum (small clones only)"""
        n = self.c.size
        if self.cmo:
            return np.einsum("abc,bdef,lfk->adlcek", self.l, self.cmo[0], self.r, optimize=True).reshape(n, n)
        return np.einsum("abc,lbk->alck", self.l, self.r, optimize=True).reshape(n, n)


def _centre(rng, shape, sectors):
    c = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if sectors is None:
        return c, None, None
    sl, sr = (np.asarray(s) for s in sectors)
    inner = int(np.prod(shape[1:-1]))
    allowed = np.broadcast_to((sl.reshape((-1,) + (1,) * (len(shape) - 1)) == sr), shape).copy()
    qn = (np.repeat(sl, inner)[:, None], (1 - sr)[:, None], np.array([1]))       # allowed: sl + (1 - sr) == 1
    return c * allowed, allowed, qn


def bond_problem(seed, Dl, Dr, w, pattern, sectors=None, dt=-0.4j):
    rng = np.random.default_rng(seed)
    ls, rs = [], []
    for spec in pattern:
        kind = spec[0]
        if kind == "IH":
            ls.append(np.eye(Dl, dtype=complex)), rs.append(_herm(rng, Dr, spec[1]))
        elif kind == "HI":
            ls.append(_herm(rng, Dl, spec[1])), rs.append(np.eye(Dr, dtype=complex))
        elif kind == "HH":
            ls.append(_herm(rng, Dl, spec[1])), rs.append(_herm(rng, Dr, spec[2]))
        elif kind == "pair":
            a, b = _fill(rng, Dl, spec[1]), _fill(rng, Dr, spec[2])
            ls += [a, a.conj().T]
            rs += [b, b.conj().T]
        elif kind == "zero":
            ls.append(np.zeros((Dl, Dl), complex)), rs.append(np.zeros((Dr, Dr), complex))
        else:
            raise ValueError(kind)
    assert len(ls) == w, (len(ls), w)
    c, allowed, qn = _centre(rng, (Dl, Dr), sectors)
    return Problem(np.stack(ls, axis=1), np.stack(rs, axis=1), [], c, dt, allowed, qn)


def site_problem(seed, Dl, Dr, wl, wr, W, pattern, sectors=None, dt=-0.3j):
    """pattern = {"l": [wl entries], "r": [wr entries]}, an entry "I" (identity) or the map of a Hermitian block"""
    rng = np.random.default_rng(seed)
    W = np.asarray(W, float)
    assert W.shape == (wl, 2, 2, wr) and np.array_equal(W, W.transpose(0, 2, 1, 3))
    assert len(pattern["l"]) == wl and len(pattern["r"]) == wr
    l = np.stack([np.eye(Dl, dtype=complex) if isinstance(m, str) else _herm(rng, Dl, m) for m in pattern["l"]], axis=1)
    r = np.stack([np.eye(Dr, dtype=complex) if isinstance(m, str) else _herm(rng, Dr, m) for m in pattern["r"]], axis=1)
    c, allowed, qn = _centre(rng, (Dl, 2, Dr), sectors)
    return Problem(l, r, [W], c, dt, allowed, qn)


# ---------------------------------------------------------------------------------------------------- census

def census(l, r, wm, allowed):
    """What the arrays hold, in the kernel's units:
    units    {(at, f, kc, x): {"c": live c tiles per term of (f, x), "lts": the output l tiles the unit holds}}
             a c tile of a term (b, e) is live where L[rows at, b, tile] has a non-zero and the centre may have one in
             (tile, e, chunk kc); a unit holds l tile lt when some term of f (of either x - one part mask serves both) has
             a live c tile and R[rows lt, f, chunk kc] has a non-zero
    unheld   {(at, lt)}: output tiles that no unit holds
    nterm    {(f, x): number of non-zero W[b, x, e, f]} (a bond matrix: 1)
    nparts   wr * ceil(Dr / 64)"""
    Dl, wl, Dr, wr = l.shape[0], l.shape[1], r.shape[0], r.shape[1]
    d = 1 if wm is None else wm.shape[1]
    ntl, ntr, nkc = Dl // 16, Dr // 16, -(-Dr // 64)
    FL = [[[bool(np.any(l[16 * at:16 * at + 16, b, 16 * ct:16 * ct + 16] != 0)) for ct in range(ntl)] for b in range(wl)]
          for at in range(ntl)]
    FR = [[[bool(np.any(r[16 * lt:16 * lt + 16, f, 16 * kt:16 * kt + 16] != 0)) for kt in range(ntr)] for f in range(wr)]
          for lt in range(ntr)]
    if allowed is None:
        FC = [[[True] * ntl for _ in range(nkc)] for _ in range(d)]
    else:
        al = np.asarray(allowed).reshape(Dl, d, Dr)
        FC = [[[bool(np.any(al[16 * ct:16 * ct + 16, e, 64 * kc:64 * kc + 64])) for ct in range(ntl)] for kc in range(nkc)]
              for e in range(d)]
    terms = {}
    for f in range(wr):
        for x in range(d):
            if wm is None:
                terms[f, x] = [(f, 0)]
            else:
                terms[f, x] = [(b, e) for b in range(wl) for e in range(d) if wm[b, x, e, f] != 0.0]
    units, held = {}, set()
    for at in range(ntl):
        for f in range(wr):
            for kc in range(nkc):
                live = {x: tuple(sum(1 for ct in range(ntl) if FL[at][b][ct] and FC[e][kc][ct]) for b, e in terms[f, x])
                        for x in range(d)}
                any_c = any(n > 0 for x in range(d) for n in live[x])
                lts = [lt for lt in range(ntr) if any(FR[lt][f][kt] for kt in range(4 * kc, min(4 * kc + 4, ntr)))]
                if not any_c:
                    lts = []
                for lt in lts:
                    held.add((at, lt))
                for x in range(d):
                    units[at, f, kc, x] = {"c": live[x], "lts": tuple(lts)}
    unheld = {(at, lt) for at in range(ntl) for lt in range(ntr)} - held
    return dict(units=units, unheld=unheld, nterm={k: len(v) for k, v in terms.items()}, nparts=wr * nkc, ntl=ntl, ntr=ntr,
                nkc=nkc, d=d, wr=wr)


def live_c_counts(cs):
    """live c tiles per (unit, term) over the units that have output tiles (the others return before step 1)"""
    return {n for u in cs["units"].values() if u["lts"] for n in u["c"]}


def l_tile_counts(cs):
    return {len(u["lts"]) for u in cs["units"].values()}


def wave_loads(cs):
    """l tiles a wave of a working unit gets in step 2: tiles wave, wave + 4, .. of the unit's"""
    return {len(range(wv, len(u["lts"]), 4)) for u in cs["units"].values() if u["lts"] for wv in range(4)}


def channel_terms(cs, f):
    return sum(cs["nterm"][f, x] for x in range(cs["d"]))


# ---------------------------------------------------------------------------------------------------- the cases

def _site_w(wl, wr, entries):
    W = np.zeros((wl, 2, 2, wr))
    for (b, f), blk in entries.items():
        W[b, :, :, f] = blk
    return W


def _ragged(Dl, Dr, seed):
    ntl, ntr, nkc = Dl // 16, Dr // 16, -(-Dr // 64)
    rlast = np.zeros((ntr, ntr), int)          # data only in the columns k of the last (short) ket chunk
    for lt in range(ntr):
        if lt % 3 != 1:
            rlast[lt, 4 * (nkc - 1):] = FULL
    return bond_problem(seed, Dl, Dr, 3, [("pair", row_counts(ntl, [2, 1, 3], 3), rlast), ("IH", band(ntr, 2))])


def _ragged_masked(Dl, Dr):
    sl, sr = cut(Dl, (Dl // 16 + 1) // 2), cut(Dr, Dr // 32 - 1)
    return bond_problem(21, Dl, Dr, 4, [("IH", secmap(sr, 0)), ("pair", secmap(sl, 1), secmap(sr, 1)), ("HI", secmap(sl, 0))],
                        sectors=(sl, sr))


def _rotation(Dl, Dr, counts, seed):
    ntl, ntr = Dl // 16, Dr // 16
    return bond_problem(seed, Dl, Dr, 3, [("pair", row_counts(ntl, counts, 2), band(ntr, 1)), ("IH", band(ntr, 2))])


def _deal(Dl, Dr):
    ntl, ntr, nkc = Dl // 16, Dr // 16, -(-Dr // 64)
    lmap = lattice(ntl, 1, 2, 0, 3) | band(ntl, 0)
    lmap[[2 % ntl, 9 % ntl], :] = 0                 # bra tile rows without data: units with nothing to do
    lmap[:, [5 % ntl, 12 % ntl]] = 0                # (and of the adjoint channel)
    r0 = np.zeros((ntr, ntr), int)                  # chunk kc of the first channel: 1, 2, 5, 9 l tiles
    for kc, n in zip(range(nkc), (1, 2, 5, 9)):
        r0[:min(n, ntr), 4 * kc:4 * kc + 4] = FULL
    r2 = np.zeros((ntr, ntr), int)                  # first chunk of the identity channel: 13 l tiles; the last three
    r2[:min(13, ntr - 1), 0] = FULL                 # l tiles without data in any chunk
    return bond_problem(31, Dl, Dr, 3, [("pair", lmap, r0), ("IH", r2)])


def _many(Dl, Dr, w, seed):
    ntl, ntr = Dl // 16, Dr // 16
    pat = [("IH", band(ntr, 1))]
    npair = (w - 2) // 2
    for p in range(npair):
        pat.append(("pair", lattice(ntl, 3, 5, p, 4), lattice(ntr, 5, 3, p, 4)))
    if 2 + 2 * npair < w:
        pat.append(("HH", band(ntl, 0), lattice(ntr, 1, 1, 0, 3)))
    pat.append(("HI", band(ntl, 1)))
    return bond_problem(seed, Dl, Dr, w, pat)


def _corners(nt, m):
    m = m.copy()
    m[0, nt - 1] = m[nt - 1, 0] = FULL
    return m


def _big_l(Dl, Dr):
    return bond_problem(51, Dl, Dr, 2, [("IH", band(Dr // 16, 1)), ("HI", _corners(Dl // 16, band(Dl // 16, 1)))])


def _big_r(Dl, Dr):
    ntl, ntr = Dl // 16, Dr // 16
    rp = lattice(ntr, 1, 1, 0, 8)
    rp[ntr - 1, ntr - 1] = rp[ntr - 1, 0] = FULL
    return bond_problem(52, Dl, Dr, 4, [("IH", _corners(ntr, band(ntr, 1))), ("pair", lattice(ntl, 1, 1, 0, 2), rp),
                                        ("HI", band(ntl, 1))])


def _padded(Dl, Dr):
    ntl, ntr = Dl // 16, Dr // 16
    return bond_problem(61, Dl, Dr, 4, [("IH", band(ntr, 2)), ("pair", lattice(ntl, 1, 2, 0, 3), lattice(ntr, 2, 1, 0, 3)),
                                        ("zero",)])


def _corner_flags(Dl, Dr):
    ntl, ntr = Dl // 16, Dr // 16
    lm, rm = band(ntl, 1), band(ntr, 1)
    # tile rows whose ONLY data is one corner element (the flag of the row hangs on it), and corner tiles among full ones
    lm[3 % ntl, :] = 0
    lm[3 % ntl, (3 + 5) % ntl] = CORNER
    lm[(7 % ntl), :] = 0
    lm[7 % ntl, (7 + 9) % ntl] = CORNER_IMAG
    lm[0, ntl - 1] = CORNER_IMAG
    rm[5 % ntr, :] = 0
    rm[5 % ntr, (5 + 6) % ntr] = CORNER_IMAG
    rm[(10 % ntr), :] = 0
    rm[10 % ntr, (10 + 3) % ntr] = CORNER
    rm[ntr - 1, 0] = CORNER
    return bond_problem(71, Dl, Dr, 3, [("pair", lm, rm), ("IH", band(ntr, 2))])


def _plain(Dl, Dr):
    ntl, ntr = Dl // 16, Dr // 16
    return bond_problem(81, Dl, Dr, 3, [("pair", lattice(ntl, 1, 1, 0, 2), band(ntr, 2)), ("IH", band(ntr, 3))])


_DENSE = OPS[3]


def _site_table_terms(Dl, Dr):
    ntl, ntr = Dl // 16, Dr // 16
    ent = {(0, 0): OPS[0], (2, 2): OPS[0], (1, 2): OPS[1]}
    for b in range(3):
        ent[b, 1] = (1.0 + 0.25 * b) * _DENSE            # six terms for each x of channel 1
    return site_problem(101, Dl, Dr, 3, 3, _site_w(3, 3, ent),
                        {"l": ["I", band(ntl, 1), lattice(ntl, 1, 1, 0, 2)], "r": [band(ntr, 1), lattice(ntr, 1, 1, 0, 2), "I"]})


def _site_table_tiles(Dl, Dr, masked):
    sl, sr = cut(Dl, Dl // 32 + 1), cut(Dr, Dr // 32 - 1)
    ent = {(b, b): OPS[b % 4] for b in range(3)}
    ent[1, 2] = ent[2, 1] = 0.5 * OPS[3]
    p = site_problem(111, Dl, Dr, 3, 3, _site_w(3, 3, ent),
                     {"l": ["I", secmap(sl, 0), secmap(sl, 0)], "r": [secmap(sr, 0), secmap(sr, 0), "I"]}, sectors=(sl, sr))
    if not masked:
        p.qn = None                   # the same operands and centre, no centre mask given to the solve
        p.census = census(p.l, p.r, p.cmo[0], None)
    return p


def _site_empty(Dl, Dr):
    ntl, ntr = Dl // 16, Dr // 16
    # right channel 2 has no term (its R holds data all the same); channel 1 has terms for x = 0 only
    ent = {(0, 0): OPS[0], (0, 1): 0.8 * np.diag([1.0, 0.0]), (1, 1): -0.6 * np.diag([1.0, 0.0]), (3, 3): OPS[0],
           (1, 3): OPS[3]}
    return site_problem(121, Dl, Dr, 4, 4, _site_w(4, 4, ent),
                        {"l": ["I", band(ntl, 1), band(ntl, 2), lattice(ntl, 1, 1, 0, 2)],
                         "r": [band(ntr, 1), lattice(ntr, 1, 1, 0, 2), band(ntr, 2), "I"]})


def _site_rect(Dl, Dr, wl, wr):
    ntl, ntr = Dl // 16, Dr // 16
    ent = {(b, f): (1.0 + 0.1 * b - 0.2 * f) * OPS[(b + f) % 4] for b in range(wl) for f in range(wr) if (b + f) % 2 == 0}
    return site_problem(131 + wl, Dl, Dr, wl, wr, _site_w(wl, wr, ent),
                        {"l": ["I"] + [lattice(ntl, 1, 1, b, 3) | band(ntl, 0) for b in range(1, wl)],
                         "r": [lattice(ntr, 1, 1, f, 3) | band(ntr, 0) for f in range(wr - 1)] + ["I"]})


def _site_terms(Dl, Dr, nterms):
    ntl, ntr = Dl // 16, Dr // 16
    ent = {(0, 0): OPS[0], (4, 2): OPS[0]}
    for b in range(4):
        ent[b, 1] = (1.0 - 0.2 * b) * _DENSE              # 4 x 4 = 16 terms in channel 1
    if nterms == 17:
        ent[4, 1] = 0.4 * np.diag([1.0, 0.0])
    return site_problem(141, Dl, Dr, 5, 3, _site_w(5, 3, ent),
                        {"l": ["I"] + [lattice(ntl, 1, 1, b, 2) | band(ntl, 0) for b in range(1, 5)],
                         "r": [band(ntr, 1), lattice(ntr, 1, 1, 0, 2), "I"]})


def _site_ragged(Dl, Dr):
    ntl, ntr = Dl // 16, Dr // 16
    ent = {(b, b): OPS[b % 4] for b in range(3)}
    return site_problem(151, Dl, Dr, 3, 3, _site_w(3, 3, ent), {"l": ["I", band(ntl, 1), band(ntl, 2)],
                                                                "r": [band(ntr, 1), band(ntr, 2), "I"]})


# id: (path the solve must take: "bond", "site" or None = refused, builder, shape, shape of the shrunken clone)
CASES = {
    "bond_ragged16": ("bond", lambda Dl, Dr: _ragged(Dl, Dr, 11), (128, 272), (32, 48)),
    "bond_ragged32": ("bond", lambda Dl, Dr: _ragged(Dl, Dr, 12), (128, 288), None),
    "bond_ragged48": ("bond", lambda Dl, Dr: _ragged(Dl, Dr, 13), (128, 304), None),
    "bond_ragged_masked": ("bond", _ragged_masked, (144, 272), (32, 48)),
    "bond_rotation": ("bond", lambda Dl, Dr: _rotation(Dl, Dr, [1, 2, 3, 4, 5, 7], 41), (272, 256), (48, 32)),
    "bond_rotation_compact": ("bond", lambda Dl, Dr: _rotation(Dl, Dr, [1, 2, 3, 4, 5, 6, 7], 42), (256, 256), None),
    "bond_deal": ("bond", _deal, (256, 256), (48, 48)),
    "bond_64_parts": ("bond", lambda Dl, Dr: _many(Dl, Dr, 16, 43), (128, 256), (32, 32)),
    "bond_65_parts": (None, lambda Dl, Dr: _many(Dl, Dr, 13, 44), (128, 272), (32, 48)),
    "bond_1024_l": ("bond", _big_l, (1024, 128), (48, 32)),
    "bond_1024_r": ("bond", _big_r, (128, 1024), (32, 48)),
    "bond_w_padded": ("bond", _padded, (192, 192), (32, 48)),
    "bond_corner_flags": ("bond", _corner_flags, (256, 256), (48, 48)),
    "bond_mask_other_shape": ("bond", _plain, (192, 192), (32, 48)),
    "site_table_terms": ("site", _site_table_terms, (144, 128), (32, 32)),
    "site_table_tiles_masked": ("site", lambda Dl, Dr: _site_table_tiles(Dl, Dr, True), (272, 128), (32, 32)),
    "site_table_tiles": ("site", lambda Dl, Dr: _site_table_tiles(Dl, Dr, False), (272, 128), None),
    "site_empty": ("site", _site_empty, (192, 128), (32, 32)),
    "site_w_rect_3_5": ("site", lambda Dl, Dr: _site_rect(Dl, Dr, 3, 5), (192, 128), (32, 32)),
    "site_w_rect_5_3": ("site", lambda Dl, Dr: _site_rect(Dl, Dr, 5, 3), (192, 128), (32, 32)),
    "site_16_terms": ("site", lambda Dl, Dr: _site_terms(Dl, Dr, 16), (144, 128), (32, 32)),
    "site_17_terms": (None, lambda Dl, Dr: _site_terms(Dl, Dr, 17), (144, 128), (32, 32)),
    "site_dr_ragged": (None, _site_ragged, (192, 144), (32, 32)),
}


def build(case_id, clone=False):
    path, make, shape, small = CASES[case_id]
    return make(*(small if clone else shape))
