"""pcnerf_set_train_query_form, form 4 (8 sample blocks per workgroup), without a GPU: 4 is accepted and comes back as
the previous value, PCNERF_TRAIN_QUERY_FORM=4 sets it when nof._ops is imported, and the neighbours that are not built
(3 and 5) are refused with the selector's message and change nothing."""
import os
import subprocess
import sys

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pc-nerf_amd")


def test_form4_accepted_and_returned():
    from nof import _ops
    prev = _ops.set_train_query_form(4)
    try:
        assert prev == -1
        assert _ops.set_train_query_form(2) == 4
        assert _ops.set_train_query_form(4) == 2
        assert _ops.set_train_query_form(0) == 4
    finally:
        _ops.set_train_query_form(prev)
    assert _ops.set_train_query_form(-1) == -1


def test_form4_neighbours_refused():
    from nof import _hip, _ops
    prev = _ops.set_train_query_form(4)
    try:
        for bad in (3, 5):
            assert _hip.lib().pcnerf_set_train_query_form(bad) == -2
            msg = _hip.lib().pcnerf_last_error()
            assert b"train_query_form" in msg and b"4 (8 sample blocks)" in msg
            with pytest.raises(ValueError, match="train_query_form"):
                _ops.set_train_query_form(bad)
        assert _ops.set_train_query_form(4) == 4   # (the refused calls changed nothing)
    finally:
        _ops.set_train_query_form(prev)


def test_form4_environment():
    env = dict(os.environ, PCNERF_TRAIN_QUERY_FORM="4", PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from nof import _ops; print(_ops.set_train_query_form(-1))"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    assert int(out.stdout.strip().splitlines()[-1]) == 4


@pytest.mark.parametrize("value", ["3", "5"])
def test_form_environment_refused(value):
    env = dict(os.environ, PCNERF_TRAIN_QUERY_FORM=value,
               PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", "from nof import _ops"], env=env, capture_output=True, text=True)
    assert out.returncode != 0
    assert "ValueError" in out.stderr and "train_query_form" in out.stderr
