"""Tamm-Dancoff approximation: excited states in the first-order tangent space of an optimised MPS (counterpart of
renormalizer/mps/tda.py:18-516, J. Chem. Phys. 140, 024108).

The reference's ``hop`` rebuilds an environment chain for every site that carries coefficients, about N^2 environment
updates per application on host closures.  Here the projected Hamiltonian is an engine handle (``mpse_tda_*``,
include/mpsengine.h): one application is 4 (N - 1) environment updates and 3 N one-site matvecs enqueued on the device,
the preconditioner is formed on the device, and the Davidson iteration is the engine's, on vectors that stay in HBM.

Like the reference, quantum numbers are not used: the roots are not restricted to the sector of the reference state.
``analysis_1ordm`` and ``analysis_dominant_config`` are not provided."""
import ctypes as C
import logging

import numpy as np

from ..engine import get_engine
from ..lib.davidson import check_limits
from .mps import Mps
from .svd_qn import _p64

logger = logging.getLogger(__name__)


def _full_left_factor(eng, c):
    """Full SVD of the site ``c`` (Dl, d, Dr) as the matrix (Dl d, Dr), ONE block through ``mpse_block_svd_full``:
    returns (u (Dl d, Dl d) device, s host, vt (rank, Dr) device), rank = min(rows, cols) as in the reference."""
    nrow, ncol = c.shape[0] * c.shape[1], c.shape[2]
    rank = min(nrow, ncol)
    rows, cols = np.arange(nrow, dtype=np.int64), np.arange(ncol, dtype=np.int64)
    roff, coff = np.array([0, nrow], dtype=np.int64), np.array([0, ncol], dtype=np.int64)
    extra = np.array([abs(nrow - ncol)], dtype=np.int64)
    ku, kv = (nrow, rank) if nrow >= ncol else (rank, ncol)
    u = eng.empty((nrow, ku), c.dtype)
    vt = eng.empty((kv, ncol), c.dtype)
    s = np.zeros(rank)
    eng._check(eng.lib.mpse_block_svd_full(eng.ctx, c.code, c.ptr, nrow, ncol, 1, _p64(rows), _p64(roff), _p64(cols),
                                           _p64(coff), _p64(extra), u.ptr, ku, vt.ptr, kv,
                                           s.ctypes.data_as(C.POINTER(C.c_double)), rank))
    return u, s, vt


def _columns(eng, u, c0, c1):
    out = eng.empty((u.shape[0], c1 - c0), u.dtype)
    eng.copy_sub(out, 0, 0, u, 0, c0, u.shape[0], c1 - c0)
    return out


class TDA(object):
    r"""Tamm-Dancoff approximation (CIS on an MPS reference): the ``nroots`` lowest eigenstates of the Hamiltonian in the
    first-order tangent space of ``mps``.

    model: the model of the system;  hmpo: the Hamiltonian ``Mpo``;  mps: the reference state (it is canonicalised and
    normalised in place);  nroots: number of roots;  algo: ``None`` / ``"davidson"``, the engine's Davidson iteration
    with the reference's settings (``"primme"`` raises: PRIMME is not available)."""

    def __init__(self, model, hmpo, mps, nroots=1, algo=None):
        self.model = model
        self.hmpo = hmpo
        self.mps = mps
        self.nroots = nroots
        self.algo = "davidson" if algo is None else algo
        self.e = None
        # wavefunction: [mps_l_cano, mps_r_cano, tangent_u, tda_coeff_list]; the two Mps live on the device, tangent_u
        # and the coefficients are host arrays (None where a site has no tangent space)
        self.wfn = None
        self.ncycle = None
        self.nmatvec = None

    def _gauges(self, include_psi0):
        """set-up of tda.py:89-121: right-canonical normalised reference, then the left-to-right SVD sweep"""
        eng = get_engine()
        mps = self.mps.ensure_right_canonical().canonicalise().normalize("mps_and_coeff").canonicalise()
        assert mps.to_right
        mps_r_cano = mps.copy()
        site_num = len(mps)
        tangent_u = []
        for ims in range(site_num):
            c = mps[ims]
            shape = list(c.shape)
            u, s, vt = _full_left_factor(eng, c)
            rank = len(s)
            if rank != shape[-1]:
                raise ValueError(f"TDA: bond {ims + 1} of the reference state is redundant ({shape[-1]} states on "
                                 f"{shape[0] * shape[1]} rows)")
            if include_psi0 and ims == site_num - 1:
                tangent_u.append(u.reshape(shape[:-1] + [-1]))
            elif rank < u.shape[1]:
                tangent_u.append(_columns(eng, u, rank, u.shape[1]).reshape(shape[:-1] + [-1]))
            else:
                tangent_u.append(None)
            mps[ims] = _columns(eng, u, 0, rank).reshape(shape[:-1] + [-1])
            if ims < site_num - 1:
                svt = eng.empty((rank, shape[-1]), vt.dtype)
                eng._check(eng.lib.mpse_gather_rows(eng.ctx, vt.code, svt.ptr, vt.ptr, shape[-1],
                                                    _p64(np.arange(rank, dtype=np.int64)),
                                                    s.ctypes.data_as(C.POINTER(C.c_double)), rank))
                nxt = mps[ims + 1]
                mps[ims + 1] = eng.matmul(svt, nxt.reshape(nxt.shape[0], -1)).reshape(nxt.shape)
        mps_l_cano = mps.copy()
        mps_l_cano.to_right = False
        mps_l_cano.qnidx = site_num - 1
        return mps_l_cano, mps_r_cano, tangent_u

    def kernel(self, restart=False, include_psi0=False):
        r"""Calculate the roots.  ``restart``: start from the coefficients of the former call (``include_psi0`` must be
        the same as then);  ``include_psi0``: the basis includes the reference state :math:`\Psi_0` (the first energy
        is then the reference energy).  Returns the energies."""
        if self.algo == "primme":
            logger.error("can not import primme")
            raise ImportError("TDA(algo='primme'): PRIMME is not available; use algo='davidson'")
        if self.algo != "davidson":
            raise ValueError(f"TDA: algo = {self.algo!r}; 'davidson' or 'primme'")
        eng = get_engine()
        mpo = self.hmpo
        site_num = len(mpo)
        if not restart:
            mps_l_cano, mps_r_cano, tu_dev = self._gauges(include_psi0)
            tangent_u = [None if u is None else u.to_host() for u in tu_dev]
            cguess = None
        else:
            mps_l_cano, mps_r_cano, tangent_u, tda_coeff_list = self.wfn
            tu_dev = [None if u is None else eng.asdevice(np.ascontiguousarray(u)) for u in tangent_u]
            cguess = [np.concatenate([c.reshape(-1) for c in coeff if c is not None]) for coeff in tda_coeff_list]
        w_dev = [eng.asdevice(np.ascontiguousarray(mpo[i])) for i in range(site_num)]
        op = eng.tda_operator(list(mps_l_cano), list(mps_r_cano), tu_dev, w_dev)
        try:
            xsize = op.xsize
            logger.debug(f"DMRG-TDA H dimension: {xsize}")
            if self.nroots > xsize:
                raise ValueError(f"TDA: nroots = {self.nroots} roots in a tangent space of dimension {xsize}")
            check_limits(self.nroots)
            if cguess is None:
                cguess = [np.random.random(xsize) - 0.5]
            hdiag = op.hdiag()
            e, c, self.ncycle, self.nmatvec = op.davidson(cguess, hdiag, self.nroots, tol=1e-12, max_cycle=100,
                                                          lindep=1e-14, shift=1e-4)
            logger.debug(f"H*C times: {self.nmatvec}")
            xshape = op.xshape
        finally:
            op.close()
        tda_coeff_list = []
        for iroot in range(self.nroots):
            coeff, off = [], 0
            for shp in xshape:
                if shp is None:
                    coeff.append(None)
                else:
                    coeff.append(c[iroot, off:off + shp[0] * shp[1]].reshape(shp).copy())
                    off += shp[0] * shp[1]
            assert off == xsize
            tda_coeff_list.append(coeff)
        self.e = np.array(e)
        self.wfn = [mps_l_cano, mps_r_cano, tangent_u, tda_coeff_list]
        return self.e

    def dump_wfn(self):
        """Dump the wavefunction for restart and analysis into the working directory (the reference's file names):
        ``mps_l_cano.npz``, ``mps_r_cano.npz``, ``tangent_u.npz``, ``tda_coeff_{iroot}.npz``."""
        mps_l_cano, mps_r_cano, tangent_u, tda_coeff_list = self.wfn
        mps_l_cano.dump("mps_l_cano.npz")
        mps_r_cano.dump("mps_r_cano.npz")
        np.savez("tangent_u.npz", **{f"{i}": mat for i, mat in enumerate(tangent_u) if mat is not None})
        for iroot, tda_coeff in enumerate(tda_coeff_list):
            np.savez(f"tda_coeff_{iroot}.npz", **{f"{i}": mat for i, mat in enumerate(tda_coeff) if mat is not None})

    def load_wfn(self, model):
        """Load what ``dump_wfn`` wrote from the working directory."""
        mps_l_cano = Mps.load(model, "mps_l_cano.npz")
        mps_r_cano = Mps.load(model, "mps_r_cano.npz")
        tangent_u_dict = np.load("tangent_u.npz")
        n = mps_l_cano.site_num
        tangent_u = [tangent_u_dict[str(i)] if str(i) in tangent_u_dict.keys() else None for i in range(n)]
        tda_coeff_list = []
        for iroot in range(self.nroots):
            d = np.load(f"tda_coeff_{iroot}.npz")
            tda_coeff_list.append([d[str(i)] if str(i) in d.keys() else None for i in range(n)])
        self.wfn = [mps_l_cano, mps_r_cano, tangent_u, tda_coeff_list]


def merge(mpsl, mpsr, idx):
    """The sites of ``mpsl`` before ``idx`` and those of ``mpsr`` from ``idx`` on; the other attributes are ``mpsl``'s."""
    mps = mpsl.copy()
    for imps in range(idx, mpsr.site_num):
        mps[imps] = mpsr[imps]
    return mps
