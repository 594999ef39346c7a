"""Zero-temperature absorption / emission spectra by the correction vector (DDMRG), counterpart of
renormalizer/cv/zerot.py:25-417.

For one frequency omega the correction vector x minimises L(x) = <x|(H - e0 - omega)^2 + eta^2|x> + 2 eta <x|mu|psi0>
(the right-hand side b = -eta mu psi0 is an MPS), and the spectrum is -L_min / (pi eta).  Built from the parts of the
DMRG sweep instead of the reference's contraction strings: the two-layer environments of (H - e0 - omega)^2 are
``Environ(cv_mps, [a_oper, a_oper])``, the overlap environments between the correction vector (bra) and b (ket) are
``Environ(b_mps, Mpo.identity(model), mps_conj=cv_mps.conj())`` (``Environ`` has no MPO-free form; the identity MPO
has bond dimension 1), and the centre system is solved by the engine's preconditioned conjugate gradients
(``Engine.pcg`` -> ``mpse_pcg``) on device-resident vectors, where the reference calls ``scipy.sparse.linalg.cg`` with
a Python closure per matvec (zerot.py:231-290).  No centre vector, environment or diagonal crosses to the host inside a
sweep: of the solve the host reads the control block.  What it still does per centre is what ``optimize_mps`` does: the
quantum-number mask is built on the host and uploaded, and ``_hdiag`` forms the per-site factor of the diagonal from a host
copy of the centre's MPO sites."""
import collections
import logging

import numpy as np

from ..engine import get_engine
from ..mps.mpo import Mpo
from ..utils import OptimizeConfig
from .spectra_cv import SpectraCv

logger = logging.getLogger("renormalizer_amd")

CentreProblem = collections.namedtuple("CentreProblem", "hop b x diag mask shift tol cidx qnbigl qnbigr")


class SpectraZtCV(SpectraCv):
    r"""Zero-temperature spectrum in the frequency domain by DDMRG.

    model: the system; spectratype: "abs" or "emi"; m_max: bond dimension of the correction vector; eta: Lorentzian
    broadening (a.u.); h_mpo: Hamiltonian (default ``Mpo(model)``); method: "1site" or "2site"; procedure_cv: percent
    per sweep; rtol: relative tolerance of the spectral value between sweeps; b_mps: the right-hand side
    :math:`-\eta \mu \psi_0` and e0: the ground-state energy (default: computed for a Holstein model from its 0- or
    1-exciton ground state); cv_mps: start vector (default: random with the quantum number of b_mps); procedure_gs: the
    ``OptimizeConfig.procedure`` of the ground-state run, default [[10, 0.4], [20, 0.2], [30, 0.1], [40, 0], [40, 0]]
    (not enough for large systems)."""

    def __init__(self, model, spectratype, m_max, eta, h_mpo=None, method="1site", procedure_cv=None, rtol=1e-5,
                 b_mps=None, e0=None, cv_mps=None, procedure_gs=None):
        self.procedure_gs = procedure_gs
        super().__init__(model, spectratype, m_max, eta, h_mpo=h_mpo, method=method, procedure_cv=procedure_cv,
                         rtol=rtol, b_mps=b_mps, e0=e0, cv_mps=cv_mps)
        self.a_oper = None
        self._identity = None

    def init_b_mps(self):
        """b = -eta * dipole * psi0 (zerot.py:79-113); Holstein models, 0- / 1-exciton sector."""
        from ..mps.gs import optimize_mps
        from ..mps.mps import Mps
        if self.spectratype == "abs":
            nexciton, dipoletype = 0, r"a^\dagger"
        elif self.spectratype == "emi":
            nexciton, dipoletype = 1, "a"
        else:
            raise ValueError("spectratype None needs b_mps and e0")
        if self.procedure_gs is None:
            self.procedure_gs = [[10, 0.4], [20, 0.2], [30, 0.1], [40, 0], [40, 0]]
        mps = Mps.random(self.model, nexciton, self.procedure_gs[0][0], percent=1.0)
        mps.optimize_config = OptimizeConfig(procedure=self.procedure_gs)
        mps.optimize_config.method = "2site"
        energies, mps = optimize_mps(mps, self.h_mpo)
        e0 = min(energies)
        dipole_mpo = Mpo.onsite(self.model, dipoletype, dipole=True)
        b_mps = dipole_mpo.apply(mps.scale(-self.eta))
        return b_mps, e0

    def init_cv_mps(self):
        """random start vector with the quantum number of b (zerot.py:115-123)"""
        from ..mps.mps import Mps
        assert self.b_mps is not None
        cv_mps = Mps.random(self.model, self.b_mps.qntot, self.m_max, percent=1.0)
        logger.info(f"cv_mps random guess qntot: {cv_mps.qntot}")
        return cv_mps

    def oper_prepare(self, omega):
        """a_oper = H - (e0 + omega) (zerot.py:125-128)"""
        identity = Mpo.identity(self.model).scale(-self.e0 - omega)
        self.a_oper = self.h_mpo.add(identity)

    def _centre(self, isite):
        """sites of the centre and the environment positions on its two sides (``isite`` counts from 1, zerot.py:147-160)"""
        cidx = [isite - 1] if self.method == "1site" else [isite - 2, isite - 1]
        return cidx, cidx[0] - 1, cidx[-1] + 1

    def optimize_cv(self, lr_group, isite, percent=0.0):
        """One centre: solve ((H - e0 - omega)^2 + eta^2) x = b in the projected space and put x into cv_mps
        (zerot.py:130-302).  Returns the value of the functional L at x.  The composition of the three parts below
        with ``Engine.pcg``; ``cv.batch_run_lockstep`` puts ``Engine.pcg_batch`` over several objects between them."""
        prob = self.centre_problem(lr_group, isite)
        res = get_engine().pcg(prob.hop, prob.b, prob.x, diag=prob.diag, mask=prob.mask, shift=prob.shift, tol=prob.tol)
        return self.centre_install(prob, res, percent)

    def centre_problem(self, lr_group, isite):
        """The centre system at ``isite``: moves the environments there and returns a ``CentreProblem`` (operator,
        right-hand side, start vector, preconditioner diagonal, mask, shift, tolerance and what ``centre_install``
        needs)."""
        from ..mps.hop_expr import hop_expr
        from ..mps.gs import _hdiag
        from ..mps.svd_qn import get_qn_mask
        eng = get_engine()
        first_LR, second_LR = lr_group
        cv, b_mps = self.cv_mps, self.b_mps
        cidx, lidx, ridx = self._centre(isite)
        lmethod, rmethod = ("System", "Enviro") if cv.to_right else ("Enviro", "System")
        two = [self.a_oper, self.a_oper]
        first_L = first_LR.GetLR("L", lidx, cv, two, itensor=None, method=lmethod)
        first_R = first_LR.GetLR("R", ridx, cv, two, itensor=None, method=rmethod)
        conj = cv.conj()
        second_L = second_LR.GetLR("L", lidx, b_mps, self._identity, itensor=None, method=lmethod, mps_conj=conj)
        second_R = second_LR.GetLR("R", ridx, b_mps, self._identity, itensor=None, method=rmethod, mps_conj=conj)

        qnbigl, qnbigr, qnmat = cv._get_big_qn(cidx)
        qn_mask = get_qn_mask(qnmat, cv.qntot)
        del qnmat
        xshape = qn_mask.shape
        mask = eng.asdevice(qn_mask.astype(np.float64))

        def two_site(a, b):
            return eng.matmul(a.reshape(-1, a.shape[-1]), b.reshape(b.shape[0], -1)).reshape(a.shape[:-1] + b.shape[1:])

        if self.method == "1site":
            guess, b_centre = cv[cidx[0]], b_mps[cidx[0]]
        else:
            guess, b_centre = two_site(cv[cidx[0]], cv[cidx[1]]), two_site(b_mps[cidx[0]], b_mps[cidx[1]])
        # right-hand side: the overlap effective operator on the centre of b (the solver reads it through the mask)
        hop_b = hop_expr(second_L, second_R, [self._identity.device(i, eng) for i in cidx], b_centre.shape)
        vec_b = hop_b(b_centre)
        assert tuple(vec_b.shape) == xshape, (vec_b.shape, xshape)

        cmo = [self.a_oper.device(i, eng) for i in cidx]
        hop = hop_expr(first_L, first_R, cmo, xshape, twolayer=True)
        # preconditioner: the diagonal of the projected (H - e0 - omega)^2 plus eta^2 (zerot.py:183-226)
        a_diag = _hdiag(eng, hop.l, hop.r, hop.cmo, twolayer=True)
        eng._check(eng.lib.mpse_axpy(eng.ctx, a_diag.code, a_diag.ptr, eng.ones(a_diag.shape, np.float64).ptr,
                                     a_diag.size, self.eta ** 2, 0.0))
        cplx = hop.operator_is_complex or guess.is_complex or vec_b.is_complex
        x = (guess.to_complex() if cplx else guess).copy().reshape(xshape)
        if cplx:
            vec_b = vec_b.to_complex()
        return CentreProblem(hop, vec_b, x, a_diag, mask, self.eta ** 2, 1.0e-5, cidx, qnbigl, qnbigr)

    def centre_install(self, prob, res, percent=0.0):
        """Puts the solution ``prob.x`` of the solve ``res`` (a ``PcgResult``) into cv_mps; returns the functional."""
        cv = self.cv_mps
        # the reference's count (zerot.py:292, taken before the functional's own matvec at :296) is scipy's matvec of the
        # start residual b - A x0 plus one per iteration
        self.hop_time.append(res.iters + 1)
        if res.status != 0:
            logger.info("iteration solver not converged")
        cv._update_mps(prob.x, prob.cidx, prob.qnbigl, prob.qnbigr, percent)
        if cv.compress_config.ofs is not None:
            raise NotImplementedError("OFS for correction vector not implemented")
        return float(res.lvalue)

    def initialize_LR(self):
        """The environments on the side the sweep moves away from: two-layer ones of a_oper around cv_mps and the
        overlap of cv_mps (bra) with b_mps (ket) (zerot.py:307-350)."""
        from ..mps.lib import Environ
        cv = self.cv_mps
        domain = "R" if cv.to_right else "L"
        self._identity = Mpo.identity(self.model)
        first_LR = Environ(cv, [self.a_oper, self.a_oper], domain)
        second_LR = Environ(self.b_mps, self._identity, domain, mps_conj=cv.conj())
        return [first_LR, second_LR]

    def update_LR(self, lr_group, isite):
        """The environments move inside ``optimize_cv`` (``GetLR`` with method "System" on the side the sweep comes
        from, as ``single_sweep`` does): nothing is left to do here (zerot.py:352-417)."""
        return lr_group
