"""CPU: the implicit-feedback entry points (hrec_als_gramian,
hrec_als_half_sweep_implicit) check their arguments before any device work."""
import ctypes

_i64, _dbl, _sz = ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
P = ctypes.c_void_p(256)  # a non-null stand-in: rejected calls never dereference it


def _lib():
    import __graft_entry__ as g
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(g.build_lib())
    lib.hrec_last_error.restype = ctypes.c_char_p
    lib.hrec_als_half_sweep_implicit.restype = ctypes.c_int
    lib.hrec_als_half_sweep_implicit.argtypes = [ctypes.c_void_p] * 3 + [_i64, ctypes.c_void_p, _i64, ctypes.c_int,
                                                                       ctypes.c_int, _dbl, _dbl] + [ctypes.c_void_p] * 3
    lib.hrec_als_gramian.restype = ctypes.c_int
    lib.hrec_als_gramian.argtypes = [ctypes.c_void_p, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_void_p, _sz, ctypes.c_void_p]
    lib.hrec_als_gramian_workspace_bytes.restype = _sz
    lib.hrec_als_gramian_workspace_bytes.argtypes = [_i64, ctypes.c_int]
    return lib


def _sweep(lib, n_rows=1, k=8, kp=16, reg=0.1, alpha=1.0, ptr=P, yty=P):
    return lib.hrec_als_half_sweep_implicit(ptr, ptr, ptr, n_rows, ptr, 5, k, kp, reg, alpha, yty, ptr, None)


def test_implicit_half_sweep_rejects_bad_arguments():
    lib = _lib()
    assert _sweep(lib, alpha=-1.0) != 0
    assert b"alpha must be >= 0" in lib.hrec_last_error()
    for kp in (48, 128):
        assert _sweep(lib, k=8, kp=kp) != 0
        assert b"kp must be 16, 32 or 64" in lib.hrec_last_error()
    assert _sweep(lib, k=17, kp=16) != 0
    assert b"1 <= k <= kp" in lib.hrec_last_error()
    assert _sweep(lib, k=0, kp=16) != 0
    assert _sweep(lib, n_rows=-1) != 0
    assert b"negative size" in lib.hrec_last_error()
    assert _sweep(lib, ptr=None) != 0
    assert b"null" in lib.hrec_last_error()
    assert _sweep(lib, yty=None) != 0
    assert b"null pointer" in lib.hrec_last_error()
    assert _sweep(lib, n_rows=0, ptr=None, yty=None) == 0  # nothing to solve


def test_gramian_rejects_bad_arguments():
    lib = _lib()
    for kp in (48, 128):
        assert lib.hrec_als_gramian(P, 10, 8, kp, P, P, 1 << 30, None) != 0
        assert b"kp must be 16, 32 or 64" in lib.hrec_last_error()
        assert lib.hrec_als_gramian_workspace_bytes(10, kp) == 0
    assert lib.hrec_als_gramian(P, 10, 17, 16, P, P, 1 << 30, None) != 0
    assert b"1 <= k <= kp" in lib.hrec_last_error()
    assert lib.hrec_als_gramian(P, -1, 8, 16, P, P, 1 << 30, None) != 0
    assert b"negative size" in lib.hrec_last_error()
    assert lib.hrec_als_gramian(None, 10, 8, 16, P, P, 1 << 30, None) != 0
    assert b"null source factors" in lib.hrec_last_error()
    assert lib.hrec_als_gramian(P, 10, 8, 16, None, P, 1 << 30, None) != 0
    assert lib.hrec_als_gramian(P, 10, 8, 16, P, None, 1 << 30, None) != 0
    assert b"null output or workspace" in lib.hrec_last_error()
    assert lib.hrec_als_gramian(P, 10, 8, 16, P, P, 8, None) != 0
    assert b"workspace" in lib.hrec_last_error()


def test_gramian_workspace_depends_on_rows_and_kp_only():
    lib = _lib()
    ws = lib.hrec_als_gramian_workspace_bytes
    assert ws(1, 16) == ws(2048, 16) == 256 * 8          # one slab, one tile pair
    assert ws(2049, 64) == 2 * 10 * 256 * 8               # two slabs, ten tile pairs
    assert ws(1_000_000, 64) == 489 * 10 * 256 * 8


def test_abi_version_is_still_7():
    lib = _lib()
    lib.hrec_abi_version.restype = ctypes.c_int
    assert lib.hrec_abi_version() == 7
