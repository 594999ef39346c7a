"""Operators of the polaron-structure job (counterpart of renormalizer/property/ops.py), as ``Mpo``s keyed by the names
the reference uses."""
import numpy as np

from ..model import HolsteinModel, Model
from ..model.op import Op
from ..mps.mpo import Mpo
from ..utils import Quantity


def _x_over_d(model, imol, kmol, jph):
    """n_imol x_(kmol, jph) / D_(kmol, jph): x = (b^+ + b) / sqrt(2 omega), D the displacement of the mode"""
    ph = model[kmol].ph_list[jph]
    return Mpo.intersite(model, {imol: r"a^\dagger a"}, {(kmol, jph): r"b^\dagger+b"},
                         scale=Quantity(np.sqrt(1.0 / 2.0 / ph.omega[0]) / ph.dis[1]))


def e_ph_static_correlation(model: HolsteinModel, imol: int = 0, jph: int = 0, periodic: bool = False, name: str = "S"):
    r"""The electron-phonon static correlation operators of a polaron (Shi et al., J. Chem. Phys. 142, 174103 (2015);
    Romero et al., J. Lumin. 83-84 (1999) 147).  Returns {name: Mpo}:

    not periodic: for every molecule m, ``"<name>_<imol>_<m>_<jph>"``: x_{m,jph} a^+_imol a_imol / D_{m,jph}
    periodic (a homogeneous ring; ``imol`` is not used): for every distance m, ``"<name>_<m>_<jph>"``:
    sum_n x_{n+m,jph} a^+_n a_n / D_{n+m,jph}

    with D the displacement of the mode between its two potential energy surfaces.  Scheme 4 is not supported."""
    if model.scheme == 4:
        raise NotImplementedError
    nmols = model.mol_num
    prop_mpos = {}
    if not periodic:
        for jmol in range(nmols):
            prop_mpos["_".join([name, str(imol), str(jmol), str(jph)])] = _x_over_d(model, imol, jmol, jph)
    else:
        for dis in range(nmols):
            total = None
            for jmol in range(nmols):
                term = _x_over_d(model, jmol, (jmol + dis) % nmols, jph)
                total = term if total is None else total.add(term)
            prop_mpos["_".join([name, str(dis), str(jph)])] = total
    return prop_mpos


def x_average(model: Model):
    """{"x": [<x> of every vibrational degree of freedom, order of model.v_dofs]}"""
    return {"x": [Mpo(model, Op("x", v_dof)) for v_dof in model.v_dofs]}


def x_square_average(model: Model):
    """{"x^2": [<x^2> of every vibrational degree of freedom, order of model.v_dofs]}.  Deviation from the reference,
    whose function returns the list one level deeper, as {"x^2": {"x": [...]}}, a value ``Property`` cannot take: here
    the list is the value itself."""
    assert isinstance(model, Model)
    return {"x^2": [Mpo(model, Op("x^2", v_dof)) for v_dof in model.v_dofs]}
