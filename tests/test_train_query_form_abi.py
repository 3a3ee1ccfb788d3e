"""pcnerf_set_train_query_form: a process-wide selector that needs no GPU -- the previous setting comes back, -1 is the
default, anything but -1, 0 and 2 (1 included: that form is not built) is refused with a message and changes nothing,
and PCNERF_TRAIN_QUERY_FORM sets it when nof._ops is imported."""
import os
import subprocess
import sys

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pc-nerf_amd")


def test_train_query_form_selector_without_gpu():
    from nof import _hip, _ops
    assert _ops.set_train_query_form(0) == -1
    try:
        assert _ops.set_train_query_form(2) == 0
        for bad in (3, -2, 1):
            assert _hip.lib().pcnerf_set_train_query_form(bad) == -2
            assert b"train_query_form" in _hip.lib().pcnerf_last_error()
        with pytest.raises(ValueError):
            _ops.set_train_query_form(3)
        assert _ops.set_train_query_form(0) == 2   # (the refused calls changed nothing)
        # its own setting: the geometry selector neither reads nor writes it, and still refuses 4
        assert _ops.set_query_geometry(1) == -1
        assert _hip.lib().pcnerf_set_query_geometry(4) == -2
        assert _ops.set_query_geometry(-1) == 1
        assert _ops.set_train_query_form(-1) == 0
    finally:
        _ops.set_train_query_form(-1)
        _ops.set_query_geometry(-1)
    assert _ops.set_train_query_form(-1) == -1
    assert _hip.lib().pcnerf_abi_version() == 1


@pytest.mark.parametrize("value,want", [("0", 0), ("2", 2), ("", -1)])
def test_train_query_form_environment(value, want):
    env = dict(os.environ, PCNERF_TRAIN_QUERY_FORM=value, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from nof import _ops; print(_ops.set_train_query_form(-1))"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    assert int(out.stdout.strip().splitlines()[-1]) == want


def test_train_query_form_environment_refused():
    """A form that is not built stops the import with the selector's message."""
    env = dict(os.environ, PCNERF_TRAIN_QUERY_FORM="1", PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", "from nof import _ops"], env=env, capture_output=True, text=True)
    assert out.returncode != 0
    assert "ValueError" in out.stderr and "train_query_form" in out.stderr
