"""The registration entries of the C ABI without a GPU: exported and bound, the ABI version unchanged, argument
errors refused on the host with -1 and a message (none of these calls reaches the device)."""
from nof import _hip

NEW = ("pcnerf_render_depth_jac_fold", "pcnerf_gn_workspace_bytes", "pcnerf_gn_normal_eq")


def test_symbols_exported_and_abi_version_unchanged():
    L = _hip.lib()
    assert set(NEW) <= set(_hip.exported_symbols())
    for n in NEW:
        assert hasattr(L, n), n
    assert L.pcnerf_abi_version() == 1


def test_workspace_bytes_follow_the_ray_count_alone():
    L = _hip.lib()
    # 32 doubles per workgroup of 256 rays, at most 1024 workgroups, at least one
    assert L.pcnerf_gn_workspace_bytes(0) == 256 and L.pcnerf_gn_workspace_bytes(-5) == 256
    assert L.pcnerf_gn_workspace_bytes(256) == 256 and L.pcnerf_gn_workspace_bytes(257) == 512
    assert L.pcnerf_gn_workspace_bytes(100003) == 391 * 256
    assert L.pcnerf_gn_workspace_bytes(1 << 30) == 1024 * 256


def test_render_depth_jac_fold_argument_errors():
    L = _hip.lib()
    f = L.pcnerf_render_depth_jac_fold
    assert f(None, 0, 8, None, 64, None, 1e-10, None, None, None, None, None) == 0   # no rays: a no-op
    for args, word in (((None, -1, 8, None, 64), b"n_rays"), ((None, 4, 5, None, 64), b"ray_stride"),
                       ((None, 4, 8, None, 0), b"n_samples < 1"), ((None, 4, 8, None, 1025), b"n_samples > 1024"),
                       ((None, 0, 8, None, 1025), b"n_samples > 1024"), ((None, 4, 8, None, 64), b"null")):
        assert f(*args, None, 1e-10, None, None, None, None, None) == -1, word
        assert word in L.pcnerf_last_error(), (word, L.pcnerf_last_error())


def test_gn_normal_eq_argument_errors():
    L = _hip.lib()
    f = L.pcnerf_gn_normal_eq
    for args, word in (((None, -1, 8), b"n_rays"), ((None, 4, 5), b"ray_stride"), ((None, 0, 8), b"null"),
                       ((None, 4, 8), b"null")):
        assert f(*args, None, None, None, None, 0.0, 0.5, None, None, None) == -1, word
        assert word in L.pcnerf_last_error(), (word, L.pcnerf_last_error())
