"""Argument checks of evolve_batch that need no device."""
import pytest

from renormalizer_amd import evolve_batch
from renormalizer_amd.mps.batch import _check_args


def test_evolve_batch_argument_checks():
    with pytest.raises(ValueError, match="empty"):
        _check_args([], None)
    with pytest.raises(ValueError, match="2 MPOs for 3 states"):
        _check_args([object()] * 3, [object()] * 2)
    states, mpos = _check_args((1, 2), "w")
    assert states == [1, 2] and mpos == ["w", "w"]


def test_evolve_batch_rejects_before_any_device_work():
    with pytest.raises(ValueError, match="empty"):
        evolve_batch([], None, 0.1)
    with pytest.raises(ValueError, match="1 MPOs for 2 states"):
        evolve_batch([object(), object()], [object()], 0.1)
