from .backend import backend
from .mpo import Mpo
from .mps import BraKetPair, Mps
from .batch import evolve_batch
from .mpdm import MpDm
from .thermalprop import ThermalProp, thermal_state
from .tda import TDA
