"""CPU: hrec_als_half_sweep_kernel (the half-sweep with the kernel chosen by
the caller) checks its arguments before any device work."""
import ctypes


def _entry():
    import __graft_entry__ as g

    lib = ctypes.CDLL(g.build_lib())
    f = lib.hrec_als_half_sweep_kernel
    f.restype = ctypes.c_int
    f.argtypes = ([ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p])
    lib.hrec_last_error.restype = ctypes.c_char_p
    return lib, f


def test_half_sweep_kernel_rejects_bad_arguments_without_gpu():
    lib, f = _entry()
    assert f(None, None, None, 1, None, 0, 1, 8, 64, 0.1, 2, None, None) == -1
    assert b"kernel must be 0 (one wave per row) or 1 (pooled)" in lib.hrec_last_error()
    for src_f64 in (0, 1):
        assert f(None, None, None, 1, None, src_f64, 1, 8, 32, 0.1, 1, None, None) == -1
        assert b"kp must be 64" in lib.hrec_last_error()
        assert f(None, None, None, 1, None, src_f64, 1, 65, 64, 0.1, 1, None, None) == -1
        assert b"need 1 <= k <= kp" in lib.hrec_last_error()
        assert f(None, None, None, 1, None, src_f64, 1, 8, 64, 0.1, 1, None, None) == -1
        assert b"null pointer" in lib.hrec_last_error()
        for kernel in (0, 1):
            assert f(None, None, None, 0, None, src_f64, 1, 8, 64, 0.1, kernel, None, None) == 0  # no rows


def test_abi_version_unchanged_by_the_added_entry():
    lib, _ = _entry()
    lib.hrec_abi_version.restype = ctypes.c_int
    assert lib.hrec_abi_version() == 7
