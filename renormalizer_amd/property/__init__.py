"""Job observables (counterpart of renormalizer/property): ``Property`` holds named MPOs and the values a job records
for them after every step, ``ops`` builds the operators of the polaron-structure job."""
from . import ops
from .property import Property
