"""``Property``: the user-defined operators of a time-stepping job and their recorded expectation values (interface and
result layout of renormalizer/property/property.py).  Whatever a step asks for as ``Mpo``s goes to the state as ONE
``mpo_expectations`` call (``mpse_mps_expect_many``: one engine call, one host read) however many names and lists there
are; complex results need an ``.npz`` dump, as in the reference."""
from typing import Dict, List

import numpy as np

_BRAKET_SELF = ("x", "x^2", "n")     # recorded as [<bra|O|bra>, <ket|O|ket>] by calc_properties_braketpair


def _is_mpo(obj):
    from ..mps.mpo import Mpo
    return isinstance(obj, Mpo)


class Property:
    def __init__(self, prop_strs: List[str], prop_mpos: Dict[str, object]):
        """prop_strs: the names of the properties, in the order they are taken; prop_mpos: {name: Mpo or list of
        Mpo}.  The name "e_rdm" needs no entry: it is the reduced density matrix of the electronic degrees of
        freedom.  ``prop_res[name]`` gains one entry per call."""
        self.prop_strs = prop_strs
        self.prop_mpos = prop_mpos
        self.prop_res = {name: [] for name in prop_strs}

    @staticmethod
    def _gathered(state, entries):
        """the values of ``entries`` (each an Mpo or a list of Mpos) from ONE ``state.mpo_expectations`` call: a scalar
        per Mpo, an array per list"""
        flat, spans = [], []
        for mpo in entries:
            if _is_mpo(mpo):
                spans.append((len(flat), None))
                flat.append(mpo)
            elif isinstance(mpo, list):
                spans.append((len(flat), len(mpo)))
                flat.extend(mpo)
            else:
                raise TypeError(f"a property is an Mpo or a list of Mpos, got {type(mpo).__name__}")
        vals = state.mpo_expectations(flat) if flat else np.array([])
        out = []
        for start, count in spans:
            if count is None:
                v = vals[start]
                out.append(complex(v) if np.iscomplexobj(v) else float(v))
            else:
                out.append(np.array(vals[start:start + count]))
        return out

    def calc_properties(self, mps, mps_conj=None):
        """One more entry of every property for the state ``mps`` (an ``Mps`` or ``MpDm``).  With ``mps_conj`` (an
        already conjugated bra that differs from the state) every Mpo is ``mps.expectation(mpo, mps_conj)`` and lists
        are not taken."""
        named = []
        for name in self.prop_strs:
            if name == "e_rdm":
                continue
            if name not in self.prop_mpos:
                raise NotImplementedError(f"property {name!r} has no operator")
            named.append(name)
        if mps_conj is None:
            values = dict(zip(named, self._gathered(mps, [self.prop_mpos[name] for name in named])))
        else:
            values = {}
            for name in named:
                mpo = self.prop_mpos[name]
                assert _is_mpo(mpo), "a list of operators cannot be taken with a separate bra"
                values[name] = mps.expectation(mpo, mps_conj)
        for name in self.prop_strs:
            self.prop_res[name].append(mps.edof_rdm() if name == "e_rdm" else values[name])

    def calc_properties_braketpair(self, pair):
        """One more entry of every property for a ``BraKetPair``: "x", "x^2" and "n" as [value(s) in the bra, value(s)
        in the ket], one ``mpo_expectations`` call per state; anything else as <bra| mpo |ket> in the convention of
        ``ket.expectation(mpo, bra)`` (the bra as it is, not conjugated), by ``Mps.matrix_element``."""
        bra, ket = pair.bra_mps, pair.ket_mps
        own = [name for name in self.prop_strs if name in _BRAKET_SELF]
        if own:
            entries = [self.prop_mpos[name] for name in own]
            in_bra, in_ket = self._gathered(bra, entries), self._gathered(ket, entries)
        for name in self.prop_strs:
            if name in _BRAKET_SELF:
                k = own.index(name)
                self.prop_res[name].append([in_bra[k], in_ket[k]])
            else:
                val = complex(bra.matrix_element(self.prop_mpos[name], ket, self_is_conj=True))
                self.prop_res[name].append(float(val.real) if np.isclose(val.imag, 0) else val)
