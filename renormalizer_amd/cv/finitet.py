"""Finite-temperature absorption / emission spectra by the correction vector (DDMRG), counterpart of
renormalizer/cv/finitet.py:30-716.

The correction vector X is an operator in MPS form, sites (D_l, d_up, d_down, D_r) like an ``MpDm``.  For one frequency
it minimises L(X) = <X|(omega - Liou)^2 + eta^2|X> - 2 Re<b|X> with Liou X = H X - X H and b = -eta mu rho_beta^(1/2),
and the spectrum is -L_min / (pi eta).  With a = omega - H the square is three terms, each two MPO layers that name the
leg they act on:

    M1 = a a X      both layers on the upper leg          weight 1
    M2 = a X H      one layer per leg, side by side       weight 2
    M3 = X H H      both layers on the lower leg          weight 1

Built from the project's parts instead of the reference's contraction strings: every term is an ``mpse_heff_ft``
descriptor (``Engine.ft_term``), its environments are moved by ``mpse_env_update_ft`` and kept in ``TermEnvirons``, the
overlap of X (bra) with b (ket) is the ``Environ`` of ``zerot.py`` (identity MPO on the upper leg, the lower leg traced),
and the centre system (M1 + 2 M2 + M3 + eta^2) x = b is solved on the device by ``Engine.pcg_sum`` with the diagonal
preconditioner formed on the device from the environment diagonals and per-site factors that are kept per site and
frequency.  The pair of quantum numbers (excitons on the upper leg, excitons on the lower leg) is an ordinary
two-component quantum number of the sweep machinery: ``CvMpDm`` gives the sites the pair labels and a total of (1, 0)
for absorption, (0, 1) for emission, so the mask, the block SVD (``mpse_block_svd_full``) and the basis selection are
those of ``Mps._update_mps``.  Inside a sweep no centre vector, environment or diagonal crosses to the host."""
import logging
import os

import numpy as np

from ..engine import LEG_DOWN, LEG_UP, get_engine
from ..mps.mpdm import MpDm
from ..mps.mpo import Mpo
from ..mps.svd_qn import add_outer, get_qn_mask
from ..utils import CompressConfig, CompressCriteria, EvolveConfig
from .spectra_cv import SpectraCv

logger = logging.getLogger("renormalizer_amd")

WEIGHTS = (1.0, 2.0, 1.0)
# per term: (MPO of layer 1, MPO of layer 2, leg of layer 1, leg of layer 2, layer 1 transposed, layer 2 transposed) with
# "a" = omega - H, "h" = H.  a X multiplies the upper leg by the MPO site as it stands; X H multiplies the lower leg from
# the right, i.e. by the transposed site.  M1 = a a X, M2 = a X H, M3 = X H H.
TERM_SPEC = (("a", "a", LEG_UP, LEG_UP, 0, 0), ("a", "h", LEG_UP, LEG_DOWN, 0, 1), ("h", "h", LEG_DOWN, LEG_DOWN, 1, 1))


class CvMpDm(MpDm):
    """Operator in MPS form whose bonds and legs carry a pair of quantum numbers (upper leg, lower leg)."""

    def _get_sigmaqn(self, idx):
        s = np.asarray(self.model.basis[idx].sigmaqn).reshape(-1)
        zero = np.zeros_like(s)
        return add_outer(np.stack([s, zero], axis=1), np.stack([zero, s], axis=1))

    @classmethod
    def random(cls, model, qntot, m_max, percent=1.0, rng=None):
        """Start vector with the bond structure of the reference's ``Mpo.finiteT_cv`` (mps/mpo.py:157-239): per bond a
        random orthogonal basis inside every block of (bond x leg pair) states whose pair does not exceed ``qntot``,
        ``m_max`` of them kept, the last site random inside the allowed entries."""
        from ..mps.basis_select import select_basis_indices
        if rng is None:
            rng = np.random.default_rng()
        qntot = np.asarray(qntot, dtype=int).reshape(2)
        new = cls()
        new.model = model
        new.qntot = qntot
        qn, dims, arrays = [np.zeros((1, 2), dtype=int)], [1], []
        for i in range(model.nsite - 1):
            qnbig = add_outer(qn[i], new._get_sigmaqn(i)).reshape(-1, 2)
            u_set, s_set, qnset = [], [], []
            for blk in sorted(set(map(tuple, qnbig.tolist()))):
                if np.any(np.array(blk) > qntot):
                    continue
                idx = np.nonzero(np.all(qnbig == np.array(blk), axis=1))[0]
                a = rng.random((len(idx), len(idx))) - 0.5
                s, u = np.linalg.eigh(a + a.T)
                full = np.zeros((len(qnbig), len(idx)))
                full[idx, :] = u
                u_set.append(full)
                s_set.append(s)
                qnset += [blk] * len(idx)
            u_set, s_set = np.concatenate(u_set, axis=1), np.concatenate(s_set)
            keep = select_basis_indices(s_set, qnset, m_max, percent)
            dims.append(len(keep))
            d = model.pbond_list[i]
            arrays.append(u_set[:, keep].reshape(dims[i], d, d, dims[i + 1]))
            qn.append(np.array([qnset[k] for k in keep], dtype=int).reshape(len(keep), 2))
        qn.append(np.zeros((1, 2), dtype=int))
        d = model.pbond_list[-1]
        last = rng.random((dims[-1], d, d, 1)) - 0.5
        mask = get_qn_mask(add_outer(qn[-2], new._get_sigmaqn(model.nsite - 1)), qntot)
        last[~mask.reshape(last.shape[:3])] = 0
        last /= np.linalg.norm(last)
        arrays.append(last)
        return cls.from_arrays(model, arrays, qn, model.nsite - 1, qntot, False)


class TermEnvirons:
    """Environments of the three terms around the correction vector, by bond: ``left[t][i]`` closes everything left of
    site i, ``right[t][i]`` everything right of it; (ket bond, layer 1, layer 2, bra bond).  ``Environ`` caches
    (bra, MPO, ket) stacks; these have a leg pattern of their own, so they live here."""

    def __init__(self, nsite, nterm=3):
        eng = get_engine()
        one = eng.ones((1, 1, 1, 1))
        self.left = [[one] + [None] * (nsite - 1) for _ in range(nterm)]
        self.right = [[None] * (nsite - 1) + [one] for _ in range(nterm)]


class SpectraFtCV(SpectraCv):
    r"""Finite-temperature spectrum in the frequency domain by DDMRG.

    model: the system; spectratype: "abs" or "emi"; m_max: bond dimension of the correction vector; eta: Lorentzian
    broadening (a.u.); temperature: a ``Quantity``; h_mpo: Hamiltonian (default ``Mpo(model)``); method: "1site" (two-site
    sweeps are not implemented at finite temperature, in the reference neither); procedure_cv: percent per sweep;
    rtol: relative tolerance of the spectral value between sweeps; b_mps: the right-hand side
    :math:`-\eta \mu \rho_\beta^{1/2}` (default: prepared for a Holstein model); cv_mps: start vector;
    icompress_config / ievolve_config / insteps: the imaginary-time propagation of the emission's thermal state
    (``insteps`` is required there); dump_dir and job_name: where that state is written and read back.  The MPO sites
    of ``h_mpo`` must be real: the preconditioner's per-site factor (``mpse_site_factor_ft``) takes real sites only."""

    def __init__(self, model, spectratype, m_max, eta, temperature, h_mpo=None, method="1site", procedure_cv=None,
                 rtol=1e-5, b_mps=None, cv_mps=None, icompress_config=None, ievolve_config=None, insteps=None,
                 dump_dir=None, job_name=None):
        if method != "1site":
            raise NotImplementedError("finite-temperature correction vectors sweep one site at a time")
        self.temperature = temperature
        self.evolve_config = EvolveConfig() if ievolve_config is None else ievolve_config
        self.compress_config = icompress_config
        if self.compress_config is None:
            self.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=m_max)
            self.compress_config.set_bonddim(len(model.pbond_list))
        self.insteps = insteps
        self.job_name = job_name
        self.dump_dir = dump_dir
        self.thermal_state_loaded = False
        super().__init__(model, spectratype, m_max, eta, h_mpo=h_mpo, method=method, procedure_cv=procedure_cv,
                         rtol=rtol, b_mps=b_mps, cv_mps=cv_mps)
        if self.b_mps.is_complex and not self.cv_mps.is_complex:
            self.cv_mps = self.cv_mps.to_complex()
            self.cv_mps.compress_config = CompressConfig(CompressCriteria.fixed, max_bonddim=m_max)
        self.a_oper = None
        self._identity = None
        self._w = None            # per site: device copies of the sites of a_oper and h_mpo
        self._factors = None      # per site: the diagonal's per-site factor of each term (kept for one frequency)

    @property
    def cv_mpo(self):
        return self.cv_mps

    @property
    def b_mpo(self):
        return self.b_mps

    @property
    def _defined_output_path(self):
        return self.dump_dir is not None and self.job_name is not None

    @property
    def _thermal_dump_path(self):
        assert self._defined_output_path
        return os.path.join(self.dump_dir, self.job_name + "_impo.npz")

    def init_b_mpo(self):
        """b = -eta * dipole * rho_beta^(1/2) (finitet.py:111-148); Holstein models, 0- / 1-exciton manifold."""
        from ..mps.thermalprop import thermal_state
        beta = self.temperature.to_beta()
        if self.spectratype == "abs":
            dipole_mpo = Mpo.onsite(self.model, r"a^\dagger", dipole=True)
            # no exciton: the Hamiltonian is the sum of the local vibrational ones, propagated exactly
            # and normalised, as the reference's exact thermal propagation does (mps/thermalprop.py:95-103)
            ket = MpDm.max_entangled_gs(self.model).evolve_exact(Mpo(self.model), beta / 2j, "GS")
            ket.normalize("mps_and_coeff")
        elif self.spectratype == "emi":
            dipole_mpo = Mpo.onsite(self.model, "a", dipole=True)
            ket = None
            if self._defined_output_path and os.path.exists(self._thermal_dump_path):
                ket = MpDm.load(self.model, self._thermal_dump_path)
                self.thermal_state_loaded = True
                logger.info(f"thermal state read from {self._thermal_dump_path}")
            if ket is None:
                if self.insteps is None:
                    raise ValueError("emission needs insteps, the number of imaginary-time steps")
                impo = MpDm.max_entangled_ex(self.model)
                impo.compress_config = self.compress_config
                impo.evolve_config = self.evolve_config
                ket, _ = thermal_state(impo, Mpo(self.model), beta / 2j / self.insteps, self.insteps)
                if self._defined_output_path:
                    os.makedirs(self.dump_dir, exist_ok=True)
                    ket.dump(self._thermal_dump_path)
        else:
            raise ValueError("spectratype None needs b_mps")
        return dipole_mpo.apply(ket.scale(-self.eta)), None

    init_b_mps = init_b_mpo

    def init_cv_mpo(self):
        """random start vector with the pair quantum numbers of |1><0| (absorption) or |0><1| (emission)"""
        qntot = {"abs": (1, 0), "emi": (0, 1)}[self.spectratype]
        return CvMpDm.random(self.model, qntot, self.m_max, percent=1.0)

    init_cv_mps = init_cv_mpo

    def oper_prepare(self, omega):
        """a_oper = omega - H (finitet.py:161-163); device copies of the sites; the factors of the old frequency go"""
        eng = get_engine()
        self.a_oper = Mpo.identity(self.model).scale(omega).add(self.h_mpo.scale(-1))
        n = len(self.cv_mps)
        self._w = [(self.a_oper.device(i, eng), self.h_mpo.device(i, eng)) for i in range(n)]
        self._factors = [None] * n

    def _terms(self, i, shape, envs=None):
        """the three terms on site i (``TERM_SPEC``)"""
        eng = get_engine()
        w = dict(zip("ah", self._w[i]))
        out = []
        for t, (k1, k2, l1, l2, t1, t2) in enumerate(TERM_SPEC):
            w1, w2 = w[k1], w[k2]
            L = None if envs is None else envs.left[t][i]
            R = None if envs is None else envs.right[t][i]
            out.append(eng.ft_term(w1, w2, l1, l2, t1, t2, shape, L, R))
        return out

    def _site_factors(self, i, terms):
        if self._factors[i] is None:
            eng = get_engine()
            self._factors[i] = [eng.site_factor_ft(t) for t in terms]
        return self._factors[i]

    def optimize_cv(self, lr_group, isite, percent=0.0):
        """One centre: solve (M1 + 2 M2 + M3 + eta^2) x = b in the projected space and put x into cv_mpo
        (finitet.py:165-360).  Returns the value of the functional L at x."""
        from ..mps.hop_expr import hop_expr
        eng = get_engine()
        envs, overlap = lr_group
        cv, b_mpo = self.cv_mps, self.b_mps
        i = isite - 1
        lmethod, rmethod = ("System", "Enviro") if cv.to_right else ("Enviro", "System")
        conj = cv.conj()
        ov_l = overlap.GetLR("L", i - 1, b_mpo, self._identity, itensor=None, method=lmethod, mps_conj=conj)
        ov_r = overlap.GetLR("R", i + 1, b_mpo, self._identity, itensor=None, method=rmethod, mps_conj=conj)

        qnbigl, qnbigr, qnmat = cv._get_big_qn([i])
        qn_mask = get_qn_mask(qnmat, cv.qntot)
        del qnmat
        xshape = qn_mask.shape
        mask = eng.asdevice(qn_mask.astype(np.float64))
        b_centre = b_mpo[i]
        vec_b = hop_expr(ov_l, ov_r, [self._identity.device(i, eng)], b_centre.shape)(b_centre)
        assert tuple(vec_b.shape) == xshape, (vec_b.shape, xshape)

        terms = self._terms(i, xshape, envs)
        diag = eng.diag_ft_sum(terms, self._site_factors(i, terms), WEIGHTS, self.eta ** 2)
        cplx = cv[i].is_complex or vec_b.is_complex or any(e.is_complex for t in range(3)
                                                            for e in (envs.left[t][i], envs.right[t][i]))
        x = (cv[i].to_complex() if cplx else cv[i]).copy().reshape(xshape)
        if cplx:
            vec_b = vec_b.to_complex()
        res = eng.pcg_sum(terms, WEIGHTS, vec_b, x, diag=diag, mask=mask, shift=self.eta ** 2, tol=1.0e-5,
                          max_iter=500)
        # as at zero temperature: the matvec of the start residual plus one per iteration
        self.hop_time.append(res.iters + 1)
        if res.status != 0:
            logger.info("iteration solver not converged")
        cv._update_mps(x, [i], qnbigl, qnbigr, percent)
        return float(res.lvalue)

    def initialize_LR(self):
        """The environments on the side the sweep moves away from, for the three terms and for the overlap with b
        (finitet.py:585-653)."""
        from ..mps.lib import Environ
        eng = get_engine()
        cv = self.cv_mps
        n = len(cv)
        self._identity = Mpo.identity(self.model)
        envs = TermEnvirons(n)
        order = range(n - 1, 0, -1) if cv.to_right else range(n - 1)
        for i in order:
            x = cv[i]
            terms = self._terms(i, x.shape)
            for t, term in enumerate(terms):
                if cv.to_right:
                    envs.right[t][i - 1] = eng.env_update_ft(term, "R", envs.right[t][i], x)
                else:
                    envs.left[t][i + 1] = eng.env_update_ft(term, "L", envs.left[t][i], x)
        overlap = Environ(self.b_mps, self._identity, "R" if cv.to_right else "L", mps_conj=cv.conj())
        return [envs, overlap]

    def update_LR(self, lr_group, isite):
        """The term environments move over the site just solved (finitet.py:655-716); the overlap environments move
        inside ``optimize_cv``."""
        eng = get_engine()
        envs, _ = lr_group
        cv = self.cv_mps
        i = isite - 1
        x = cv[i]
        terms = self._terms(i, x.shape)
        for t, term in enumerate(terms):
            if cv.to_right:
                envs.left[t][i + 1] = eng.env_update_ft(term, "L", envs.left[t][i], x)
            else:
                envs.right[t][i - 1] = eng.env_update_ft(term, "R", envs.right[t][i], x)
        return lr_group
