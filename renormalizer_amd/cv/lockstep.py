"""Several correction-vector frequencies swept in lock-step: the centre systems of up to ``width`` frequencies go to the
engine in one ``Engine.pcg_batch`` call per site, where members of one shape share every launch of the conjugate
gradients (``mpse_pcg_batch``, the one-launch two-layer matvec of mpse_small2.hip).  The frequencies of a spectrum share
the model, ``b_mps``, ``e0`` and ``m_max`` and differ in the numbers inside ``a_oper``: their centres have equal shapes
almost everywhere.

Each frequency is a member with what a worker of the reference's process pool starts from (spectra_cv.py:17-49): its own
copy of ``obj.cv_mps`` as it is on entry, its own ``a_oper``, environments, ``hop_time`` and
``macro_iteration_result``.  A member's sweeps are those of ``SpectraCv.cv_solve``; since the engine returns for a member
the same bits whatever else is in the batch, the spectral value of a frequency does not depend on ``width`` or on the
other frequencies of the list."""
import collections
import copy
import logging

import numpy as np

from ..engine import EngineError, get_engine

logger = logging.getLogger("renormalizer_amd")

# the eligibility rule of the one-launch two-layer matvec (mpse_pcg_batch_plan; the constants of mpse_internal.h)
SM2_WMAX, SM2_DMAX, SM2_BMAX, SM2_LDS_MAX, SM2_NNZ_LDS, SM2_THREADS = 8, 16, 64, 65536, 1024, 256


def small2_plan(Dl, d, Dr, wl, wr, cplx):
    """The launch plan of the one-launch two-layer matvec (mirrors ``small2_plan`` of mpse_small2.hip): None when the
    centre (Dl, d, Dr) with MPO bonds wl, wr does not take it, else (slice width of the ket bond of R, K groups of the
    last step, LDS bytes).  Eligible: every extent within its limit, and beside the sparse W list and the row of L
    the LDS budget holds the intermediates of at least one ket-bond state and the partials of at least one K group."""
    if min(Dl, d, Dr, wl, wr) < 1:
        return None
    if Dl > SM2_BMAX or Dr > SM2_BMAX or d > SM2_DMAX or wl > SM2_WMAX or wr > SM2_WMAX:
        return None
    es = 16 if cplx else 8
    rows, pitch = d * wr, wl * d
    nnz = min(rows * pitch, SM2_NNZ_LDS)
    csr_dbl = ((rows + 2) // 2 + (nnz + 1) // 2 + nnz + 1) & ~1
    len_l = wl * wl * Dl
    avail = (SM2_LDS_MAX - 256 - csr_dbl * 8) // es - len_l
    wmax = max(wl, wr)
    per_j = wmax * wmax * d + wl * d * wr
    if avail < per_j:
        return None
    jh = min(Dr, avail // per_j)
    nslice = -(-Dr // jh)
    jh = -(-Dr // nslice)
    g = min(SM2_THREADS // Dr, jh * wr * wr, avail // (d * Dr))
    if g < 1:
        return None
    return jh, g, csr_dbl * 8 + (len_l + max(per_j * jh, g * d * Dr)) * es


def small2_eligible(Dl, d, Dr, wl, wr, cplx):
    """Whether a two-layer one-site centre takes the batched kernels: a rule on its own shape and dtype."""
    return small2_plan(Dl, d, Dr, wl, wr, cplx) is not None


def group_members(shapes, limit):
    """How ``mpse_pcg_batch`` groups its members.  ``shapes[i]``: (Dl, d, Dr, wl, wr, cplx) of a two-layer one-site
    member, None for any other.  Returns (launch sets, singles): the sets are lists of member positions with one
    shape, at most ``limit`` each, in the order in which a set fills up or, at the end, in which its shape first
    appeared; the singles are the positions handed to ``mpse_pcg``, ascending."""
    sets, open_sets, singles = [], collections.OrderedDict(), []
    for i, shp in enumerate(shapes):
        if shp is None or not small2_eligible(*shp):
            singles.append(i)
            continue
        cur = open_sets.setdefault(tuple(shp), [])
        if len(cur) == limit:
            sets.append(list(cur))
            del cur[:]
        cur.append(i)
    sets.extend(list(v) for v in open_sets.values() if v)
    return sets, singles


def refill(active, pending, width):
    """Members in flight at the next sweep start: those still active keep their order, then the next entries of
    ``pending`` (a deque, consumed from the left) up to ``width``."""
    out = list(active)
    while len(out) < width and pending:
        out.append(pending.popleft())
    return out


def lockstep_schedule(sweeps_needed, width):
    """The order in which the frequencies run: ``sweeps_needed[i]`` sweeps for frequency i.  Returns, per sweep round,
    the list of frequency positions in flight (pure: what ``batch_run_lockstep`` does when frequency i stops after
    ``sweeps_needed[i]`` sweeps)."""
    pending = collections.deque(range(len(sweeps_needed)))
    left = {}
    active, rounds = [], []
    while pending or active:
        active = refill(active, pending, width)
        for i in active:
            left.setdefault(i, sweeps_needed[i])
        rounds.append(list(active))
        for i in active:
            left[i] -= 1
        active = [i for i in active if left[i] > 0]
    return rounds


class _Member:
    """One frequency in flight: a shallow copy of the job with its own correction vector, operator and results."""

    def __init__(self, obj, index, omega):
        o = copy.copy(obj)
        o.cv_mps = obj.cv_mps.copy()
        o.hop_time, o.macro_iteration_result = [], []
        o.a_oper = None
        o._identity = None
        o.oper_prepare(omega)
        self.o, self.index, self.omega = o, index, omega
        self.isweep = 0
        self.lr_group = None
        self.irange, self.micro = None, None
        self.result = None

    def begin_sweep(self):
        o, cv = self.o, self.o.cv_mps
        len_cv = len(cv)
        first = 1 if o.method == "1site" else 2
        if cv.to_right and cv.qnidx == 0:
            self.irange = list(range(first, len_cv + 1))
        elif (not cv.to_right) and cv.qnidx == cv.site_num - 1:
            self.irange = list(range(len_cv, first - 1, -1))
        else:
            assert False
        if self.isweep == 0:
            self.lr_group = o.initialize_LR()
        self.micro = []
        return len(self.irange)

    def install(self, prob, res, step):
        o, cv = self.o, self.o.cv_mps
        isite = self.irange[step]
        l_value = o.centre_install(prob, res, percent=o.procedure_cv[self.isweep])
        at_end = (not cv.to_right and isite == 1) or (cv.to_right and isite == len(cv))
        if not (o.method == "1site" and at_end):
            self.lr_group = o.update_LR(self.lr_group, isite)
        self.micro.append(-1.0 / (np.pi * o.eta) * l_value)

    def end_sweep(self):
        """the stopping rule of ``cv_solve``; True: the member leaves with ``result``"""
        o = self.o
        procedure = o.procedure_cv[self.isweep]
        o.cv_mps.to_right = not o.cv_mps.to_right
        o.macro_iteration_result.append(max(self.micro))
        converged = False
        if self.isweep > 0 and procedure == 0:
            v1, v2 = sorted(o.macro_iteration_result)[-2:]
            converged = abs((v1 - v2) / v1) < o.rtol
        self.isweep += 1
        if not converged and self.isweep < len(o.procedure_cv):
            return False
        if converged:
            logger.info("cv converged!")
        else:
            logger.warning("cv *NOT* converged!")
        self.result = max(o.macro_iteration_result)
        logger.info(f"omega:{self.omega}, sweeps:{self.isweep}, average_hop:{int(np.mean(o.hop_time))},"
                    f"res:{self.result}")
        return True


def _sweep(members, eng):
    nstep = {m.begin_sweep() for m in members}
    assert len(nstep) == 1
    for step in range(nstep.pop()):
        probs = [m.o.centre_problem(m.lr_group, m.irange[step]) for m in members]
        results = [None] * len(members)
        for code in sorted({p.x.code for p in probs}):      # (one working dtype per engine call)
            pos = [i for i, p in enumerate(probs) if p.x.code == code]
            sel = [probs[i] for i in pos]
            res = eng.pcg_batch([p.hop for p in sel], [p.b for p in sel], [p.x for p in sel], [p.diag for p in sel],
                                [p.mask for p in sel], [p.shift for p in sel], sel[0].tol)
            for i, r in zip(pos, res):
                results[i] = r
        for m, p, r in zip(members, probs, results):
            if r.status not in (0, 3):
                raise EngineError(f"pcg_batch: omega = {m.omega}, site {m.irange[step]}: status {r.status} "
                                  f"(operator not positive definite, or a bad preconditioner diagonal)")
            m.install(p, r, step)


def batch_run_lockstep(freq_reg, obj, width=8, filename=None):
    """Spectrum over the frequencies ``freq_reg`` with up to ``width`` of them in flight: all members visit the sites of
    their sweeps together and their centre systems are solved by one ``Engine.pcg_batch`` call per step.  A member that
    meets the stopping rule of ``cv_solve`` leaves, and the next frequency takes its place at the next sweep start.
    Every member starts from ``obj.cv_mps`` as it is on entry (``batch_run`` carries the vector from one frequency to
    the next); ``obj`` itself is left unchanged.  ``filename``: the values in the order of ``freq_reg`` (NaN where a
    frequency has not finished) are saved (``np.save``) whenever a frequency finishes.  Returns the list of spectral
    values in the order of ``freq_reg``.  ``SpectraZtCV`` only."""
    from .zerot import SpectraZtCV
    if not isinstance(obj, SpectraZtCV):
        raise NotImplementedError(f"batch_run_lockstep: {type(obj).__name__} is not supported (its centre systems are "
                                  f"not those of mpse_pcg_batch); use batch_run")
    assert width >= 1
    eng = get_engine()
    freq_reg = list(freq_reg)
    logger.info(f"{len(freq_reg)} total frequency points to do, {width} in lock-step")
    spectra = [float("nan")] * len(freq_reg)
    pending = collections.deque(range(len(freq_reg)))
    active = []
    while pending or active:
        have = {m.index for m in active}
        active = [m if isinstance(m, _Member) else _Member(obj, m, freq_reg[m])
                  for m in refill(active, pending, width) if isinstance(m, _Member) or m not in have]
        _sweep(active, eng)
        still = []
        for m in active:
            if m.end_sweep():
                spectra[m.index] = m.result
                if filename is not None:
                    np.save(f"{filename}", spectra)
            else:
                still.append(m)
        active = still
    return spectra
