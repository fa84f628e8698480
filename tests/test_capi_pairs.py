"""CPU: the pairwise ALS entries (hrec_als_predict_pairs,
hrec_als_pair_metrics and its workspace query) are exported, bound, and check
their arguments before any device work."""
import ctypes

_i64, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
P = ctypes.c_void_p(256)  # a non-null, 16-B aligned stand-in: rejected calls never dereference it
KP_MSG = b"kp must be 16, 32, 64, 96, 128, 192 or 256"


def _lib():
    import __graft_entry__ as g
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(g.build_lib())
    lib.hrec_last_error.restype = ctypes.c_char_p
    lib.hrec_abi_version.restype = _int
    model = [_vp, _i64, _vp, _i64, _int, _int, _vp, _vp, _i64]
    lib.hrec_als_predict_pairs.restype = _int
    lib.hrec_als_predict_pairs.argtypes = model + [_vp, _vp]
    lib.hrec_als_pair_metrics_workspace_bytes.restype = _sz
    lib.hrec_als_pair_metrics_workspace_bytes.argtypes = [_i64]
    lib.hrec_als_pair_metrics.restype = _int
    lib.hrec_als_pair_metrics.argtypes = model + [_vp, _vp, _vp, _vp, _sz, _vp]
    return lib


def _predict(lib, U=P, n_u=5, V=P, n_v=5, k=8, kp=16, ur=P, ir=P, n=3, out=P):
    return lib.hrec_als_predict_pairs(U, n_u, V, n_v, k, kp, ur, ir, n, out, None)


def _metrics(lib, U=P, n_u=5, V=P, n_v=5, k=8, kp=16, ur=P, ir=P, n=3, labels=P, pred=None, sums=P, ws=P,
             ws_bytes=1 << 20):
    return lib.hrec_als_pair_metrics(U, n_u, V, n_v, k, kp, ur, ir, n, labels, pred, sums, ws, ws_bytes, None)


def test_symbols_are_exported_bound_and_abi_is_still_7():
    lib = _lib()
    from src import _hrec

    for name in ("hrec_als_predict_pairs", "hrec_als_pair_metrics_workspace_bytes", "hrec_als_pair_metrics"):
        assert hasattr(lib, name)
        assert name in _hrec._SIGNATURES
    assert lib.hrec_abi_version() == 7
    assert callable(_hrec.als_predict_pairs) and callable(_hrec.als_pair_metrics)
    assert len(_hrec.PAIR_SUMS) == 10  # HREC_PAIR_SUMS


def test_predict_pairs_rejects_bad_arguments():
    lib = _lib()
    for kp in (0, 8, 48, 512):
        assert _predict(lib, kp=kp) == -1
        assert KP_MSG in lib.hrec_last_error() and b"als_predict_pairs" in lib.hrec_last_error()
    for k, kp in ((0, 16), (17, 16), (-1, 64), (257, 256)):
        assert _predict(lib, k=k, kp=kp) == -1
        assert b"1 <= k <= kp" in lib.hrec_last_error()
    for kw in ({"n": -1}, {"n_u": -1}, {"n_v": -1}):
        assert _predict(lib, **kw) == -1
        assert b"negative size" in lib.hrec_last_error()
    for kw in ({"ur": None}, {"ir": None}, {"out": None}):
        assert _predict(lib, **kw) == -1
        assert b"null pointer" in lib.hrec_last_error()
    for kw in ({"U": None}, {"V": None}):
        assert _predict(lib, **kw) == -1
        assert b"null factors" in lib.hrec_last_error()
    assert _predict(lib, U=ctypes.c_void_p(260)) == -1
    assert b"16-B aligned" in lib.hrec_last_error()


def test_predict_pairs_of_no_pairs_is_a_no_op():
    lib = _lib()
    assert _predict(lib, n=0) == 0
    assert _predict(lib, n=0, U=None, V=None, ur=None, ir=None, out=None) == 0
    assert _predict(lib, n=0, kp=48) == -1  # the model's shape is still checked
    assert KP_MSG in lib.hrec_last_error()


def test_pair_metrics_rejects_bad_arguments():
    lib = _lib()
    assert _metrics(lib, kp=48) == -1
    assert KP_MSG in lib.hrec_last_error() and b"als_pair_metrics" in lib.hrec_last_error()
    assert _metrics(lib, k=17) == -1
    assert b"1 <= k <= kp" in lib.hrec_last_error()
    for kw in ({"n": -1}, {"n_u": -1}, {"n_v": -1}):
        assert _metrics(lib, **kw) == -1
        assert b"negative size" in lib.hrec_last_error()
    for kw in ({"sums": None}, {"ws": None}):
        assert _metrics(lib, **kw) == -1
        assert b"null sums or workspace" in lib.hrec_last_error()
    for kw in ({"ur": None}, {"ir": None}, {"labels": None}):
        assert _metrics(lib, **kw) == -1
        assert b"null pointer" in lib.hrec_last_error()
    assert _metrics(lib, U=None) == -1
    assert b"null factors" in lib.hrec_last_error()
    need = lib.hrec_als_pair_metrics_workspace_bytes(70000)
    assert _metrics(lib, n=70000, ws_bytes=need - 1) == -1
    assert b"workspace" in lib.hrec_last_error() and str(need).encode() in lib.hrec_last_error()


def test_pair_metrics_workspace_query():
    """One partial of 10 doubles per block; the block count grows with n up
    to the grid cap and never overflows."""
    lib = _lib()
    f = lib.hrec_als_pair_metrics_workspace_bytes
    sizes = [f(n) for n in (-5, 0, 1, 256, 257, 70000, 10 ** 6, 5 * 10 ** 8, 2 ** 62)]
    assert all(s >= 80 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes[5] >= (70000 + 255) // 256 * 80  # several blocks take part at n = 70 000
    assert sizes[-1] == sizes[-2] <= 1 << 20      # capped grid
