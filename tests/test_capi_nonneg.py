"""CPU: the non-negative half-sweep entry point (hrec_als_half_sweep_nonneg)
is exported and checks its arguments before any device work."""
import ctypes

_i64, _dbl = ctypes.c_int64, ctypes.c_double
P = ctypes.c_void_p(256)  # a non-null stand-in: rejected calls never dereference it


def _lib():
    import __graft_entry__ as g
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(g.build_lib())
    lib.hrec_last_error.restype = ctypes.c_char_p
    lib.hrec_als_half_sweep_nonneg.restype = ctypes.c_int
    lib.hrec_als_half_sweep_nonneg.argtypes = [ctypes.c_void_p] * 3 + [_i64, ctypes.c_void_p, _i64, ctypes.c_int,
                                                                     ctypes.c_int, _dbl, ctypes.c_int, _dbl] + \
        [ctypes.c_void_p] * 4
    return lib


def _sweep(lib, n_rows=1, n_src=5, k=8, kp=16, reg=0.1, implicit=0, alpha=1.0, ptr=P, yty=P, iters=None):
    return lib.hrec_als_half_sweep_nonneg(ptr, ptr, ptr, n_rows, ptr, n_src, k, kp, reg, implicit, alpha, yty, ptr,
                                          iters, None)


def test_symbol_is_exported_and_abi_is_still_7():
    lib = _lib()
    assert hasattr(lib, "hrec_als_half_sweep_nonneg")
    lib.hrec_abi_version.restype = ctypes.c_int
    assert lib.hrec_abi_version() == 7
    from src import _hrec

    assert "hrec_als_half_sweep_nonneg" in _hrec._SIGNATURES


def test_nonneg_half_sweep_rejects_bad_arguments():
    lib = _lib()
    for kp in (48, 96, 128):
        assert _sweep(lib, k=8, kp=kp) != 0
        assert b"kp must be 16, 32 or 64" in lib.hrec_last_error()
        assert b"rank <= 64" in lib.hrec_last_error()
    assert _sweep(lib, k=17, kp=16) != 0
    assert b"1 <= k <= kp" in lib.hrec_last_error()
    assert _sweep(lib, k=0, kp=16) != 0
    assert b"1 <= k <= kp" in lib.hrec_last_error()
    assert _sweep(lib, n_rows=-1) != 0
    assert b"negative size" in lib.hrec_last_error()
    assert _sweep(lib, implicit=2) != 0
    assert b"implicit must be 0 or 1" in lib.hrec_last_error()
    for imp in (0, 1):
        assert _sweep(lib, implicit=imp, alpha=-1.0) != 0
        assert b"alpha must be >= 0" in lib.hrec_last_error()
    assert _sweep(lib, reg=-0.1) != 0
    assert b"reg_param must be >= 0" in lib.hrec_last_error()
    assert _sweep(lib, k=64, kp=64, n_src=(1 << 24) + 1) != 0  # 64 floats a row: past 4 GiB
    assert b"4 GiB" in lib.hrec_last_error()
    assert _sweep(lib, ptr=None) != 0
    assert b"null" in lib.hrec_last_error()
    assert _sweep(lib, implicit=1, yty=None) != 0
    assert b"null pointer" in lib.hrec_last_error()
    assert _sweep(lib, n_src=0) != 0
    assert b"null source factors" in lib.hrec_last_error()
    # nothing to solve: no pointer is needed, explicit or implicit
    assert _sweep(lib, n_rows=0, ptr=None, yty=None) == 0
    assert _sweep(lib, n_rows=0, implicit=1, ptr=None, yty=None) == 0
