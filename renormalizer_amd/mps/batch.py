"""Several trajectories of one model evolved in lock-step (one-site TDVP-PS).

``evolve_batch(states, mpo, dt)[i]`` is bitwise ``states[i].evolve(mpo_i, dt)``.  Per site the forward solves of all
members go to the engine in one ``mpse_expm_lanczos_batch`` call (the small-centre Krylov chain runs with a member index
inside every launch), then every member's QR, environment update and installation, then one
batched call for the bond factors, then every member's absorption - the plain order of ``Mps._evolve_tdvp_ps_sweeps``,
whose pipelined form gives the same tensors bit for bit.  The per-trajectory pieces are those of the single path
(``_PsSweep``)."""
import os
import threading

import numpy as np

from ..engine import get_engine
from ..lib.krylov import expm_krylov_batch
from ..utils import EvolveMethod
from . import mps as _m


def _check_args(states, mpo):
    states = list(states)
    if not states:
        raise ValueError("evolve_batch: empty batch")
    if isinstance(mpo, (list, tuple)):
        mpos = list(mpo)
        if len(mpos) != len(states):
            raise ValueError(f"evolve_batch: {len(mpos)} MPOs for {len(states)} states")
    else:
        mpos = [mpo] * len(states)
    return states, mpos


def _lockstep_ok(states, mpos):
    if len(states) < 2:
        return False
    if os.environ.get("MPSE_QR_OPTIMISTIC", "1") == "0" or os.environ.get("MPSE_DEFER", "1") == "0":
        return False          # (the single path then verifies every decomposition as it happens)
    s0 = states[0]
    for s in states:
        cfg = s.evolve_config
        if cfg.method is not EvolveMethod.tdvp_ps or cfg.adaptive or cfg.ivp_solver != "krylov":
            return False
        if len(s) != len(s0) or s.to_right != s0.to_right or list(s.bond_dims) != list(s0.bond_dims):
            return False
    return True


def _holders(n):
    """the carried environments of the members (``_m._CARRY.slot`` for a batch): one holder per member position"""
    hs = getattr(_m._CARRY, "batch", None)
    if hs is None or len(hs) != n:
        hs = _m._CARRY.batch = [threading.local() for _ in range(n)]
    return hs


def _sweep_step(states, mpos, evolve_dt):
    """one lock-step TDVP-PS step (optimistic block QR); None when a decomposition broke down"""
    eng = get_engine()
    holders = _holders(len(states))
    eng.block_qr_optimistic(True)
    try:
        sws = [_m._PsSweep(s, w, evolve_dt, carry=h) for s, w, h in zip(states, mpos, holders)]
        dt = sws[0].evolve_dt
        for _ in range(2):
            order = list(sws[0].mps.iter_idx_list(full=True))
            centres = [sw.mps[order[0]] for sw in sws]
            ready = [sw.prepare(order[0], list(c.shape)) for sw, c in zip(sws, centres)]
            for imps in order:
                shapes = [list(c.shape) for c in centres]
                res, js = expm_krylov_batch([r[0] for r in ready], -1j * dt / 2, centres)
                for sw, j in zip(sws, js):
                    sw.local_steps.append(j)
                if not ready[0][1]:
                    for sw, t, shape in zip(sws, res, shapes):
                        sw.mps[imps] = t.reshape(shape)
                    continue
                splits = []
                for k, sw in enumerate(sws):
                    hop_b, bond, nbr = sw.split_site(imps, res[k], ready[k], shapes[k])
                    sw.note_qr(imps)
                    ready[k] = sw.prepare(nbr, list(sw.mps[nbr].shape[:-1]) + [bond.shape[1]] if not sw.mps.to_right
                                          else [bond.shape[0]] + list(sw.mps[nbr].shape[1:]))
                    splits.append((hop_b, bond, nbr))
                bres, js = expm_krylov_batch([sp[0] for sp in splits], 1j * dt / 2, [sp[1] for sp in splits])
                for k, sw in enumerate(sws):
                    sw.local_steps.append(js[k])
                    _, bond, nbr = splits[k]
                    centres[k] = sw.mps[nbr] = sw.absorb(bres[k].reshape(bond.shape), nbr)
            for sw in sws:
                sw.mps._switch_direction()
        failed = eng.block_qr_check()
    except Exception:
        if not eng.block_qr_check():      # (as Mps._evolve_tdvp_ps: only a breakdown is the optimistic mode's own)
            raise
        failed = True
    finally:
        eng.block_qr_optimistic(False)
    if failed:
        return None
    return [sw.finish() for sw in sws]


def evolve_batch(states, mpo, evolve_dt, normalize=True):
    """Evolve every state by one step of ``evolve_dt``: ``[s.evolve(mpo_i, evolve_dt, normalize) for s in states]``
    bitwise (site tensors, quantum numbers, ``evolve_config.stat``, the notes of the block QR), the inputs untouched.
    ``mpo``: one ``Mpo`` for all states or a list with one per state.  States that are all one-site TDVP-PS with fixed
    steps and the Krylov solver, of one length, sweep direction and bond dimensions run in lock-step; any other batch
    is evolved state by state."""
    states, mpos = _check_args(states, mpo)
    if not _lockstep_ok(states, mpos):
        return [s.evolve(w, evolve_dt, normalize) for s, w in zip(states, mpos)]
    new = _sweep_step(states, mpos, evolve_dt)
    if new is None:
        # a block QR broke down somewhere in the batch: the step is discarded (the working copies carry their own QR
        # notes, the inputs' are untouched) and every member repeats it through its own Mps.evolve, which makes its
        # own optimistic / verified decision
        _m.clear_evolve_cache()
        _m._OPTIMISTIC_REDONE[0] += 1
        return [s.evolve(w, evolve_dt, normalize) for s, w in zip(states, mpos)]
    if normalize:
        for m in new:
            if np.iscomplex(evolve_dt):
                m.normalize("mps_and_coeff")
            else:
                m.normalize("mps_only")
    return new
