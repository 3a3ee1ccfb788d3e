"""The remat-version pair of nof._ops, which needs no GPU.  The rematerialising backward has one layer kernel
(k_bwd_remat3 with the epilogue on the W waves, "version 4"): get_remat_version() is 4, set_remat_version(4) is
accepted, every other value (2 and 3, the retired forms, included) is refused with a message, the library exports no
selector, and PCNERF_REMAT_VER goes through set_remat_version when nof._ops is imported."""
import os
import subprocess
import sys

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pc-nerf_amd")


def test_remat_version_selector_without_gpu():
    from nof import _hip, _ops
    assert _ops.get_remat_version() == 4
    assert _ops.set_remat_version(4) == 4
    for bad in (2, 3, 0, 5):
        with pytest.raises(RuntimeError, match="remat_version"):
            _ops.set_remat_version(bad)
        assert _ops.get_remat_version() == 4
    assert _hip.lib().pcnerf_abi_version() == 1
    for gone in ("pcnerf_set_remat_version", "pcnerf_debug_rbclk"):   # (the selector and the cycle-stamp diagnostic)
        assert not hasattr(_hip.lib(), gone)


def _import_ops(version):
    env = dict(os.environ, PCNERF_REMAT_VER=version, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from nof import _ops; print(_ops.get_remat_version())"
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


@pytest.mark.parametrize("value", ["4"])
def test_remat_version_environment(value):
    out = _import_ops(value)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == int(value)


def test_remat_version_environment_refused():
    """The retired versions stop the import with the setter's message."""
    for value in ("2", "3"):
        out = _import_ops(value)
        assert out.returncode != 0
        assert "RuntimeError" in out.stderr and "remat_version" in out.stderr and "no longer built" in out.stderr
