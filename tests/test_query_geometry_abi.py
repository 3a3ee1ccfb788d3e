"""pcnerf_set_query_geometry: a process-wide selector that needs no GPU -- the previous setting comes back, -1 is the
default (each query's own geometry), anything outside -1..3 is refused with a message and changes nothing."""
import pytest


def test_query_geometry_selector_without_gpu():
    from nof import _hip, _ops
    assert _ops.set_query_geometry(1) == -1
    try:
        assert _ops.set_query_geometry(3) == 1
        assert _hip.lib().pcnerf_set_query_geometry(4) == -2
        assert b"query_geometry" in _hip.lib().pcnerf_last_error()
        with pytest.raises(ValueError):
            _ops.set_query_geometry(-2)
        assert _ops.set_query_geometry(0) == 3
    finally:
        _ops.set_query_geometry(-1)
    assert _ops.set_query_geometry(-1) == -1
