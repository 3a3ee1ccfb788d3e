"""pcnerf_set_remat_version: the selector of the rematerialising backward's layer kernel, which needs no GPU.  4
(k_bwd_remat3 with the epilogue on the W waves, the default) and 2 (k_bwd_remat2) are built: the previous setting
comes back.  Everything else (3, the retired D-wave-epilogue form, included) is refused with a message and changes
nothing, and PCNERF_REMAT_VER goes through the selector when nof._ops is imported."""
import os
import subprocess
import sys

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pc-nerf_amd")


def test_remat_version_selector_without_gpu():
    from nof import _hip, _ops
    assert _ops.set_remat_version(4) == 4
    assert _ops.get_remat_version() == 4
    try:
        assert _ops.set_remat_version(2) == 4
        for bad in (3, 5, 0):
            assert _hip.lib().pcnerf_set_remat_version(bad) == -1
            assert b"remat_version" in _hip.lib().pcnerf_last_error()
            with pytest.raises(RuntimeError, match="remat_version"):
                _ops.set_remat_version(bad)
            assert _ops.get_remat_version() == 2   # (the refused calls changed nothing)
        assert _ops.set_remat_version(4) == 2
    finally:
        _ops.set_remat_version(4)
    assert _hip.lib().pcnerf_abi_version() == 1
    assert not hasattr(_hip.lib(), "pcnerf_debug_rbclk")   # (the cycle-stamp diagnostic of k_bwd_remat2 is gone)


def _import_ops(version):
    env = dict(os.environ, PCNERF_REMAT_VER=version, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "from nof import _ops; print(_ops.get_remat_version())"
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


@pytest.mark.parametrize("value", ["4", "2"])
def test_remat_version_environment(value):
    out = _import_ops(value)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == int(value)


def test_remat_version_environment_refused():
    """The retired version stops the import with the selector's message."""
    out = _import_ops("3")
    assert out.returncode != 0
    assert "RuntimeError" in out.stderr and "remat_version" in out.stderr and "no longer built" in out.stderr
