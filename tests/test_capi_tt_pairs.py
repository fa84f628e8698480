"""CPU: the pairwise two-tower entries (hrec_tt_predict_pairs,
hrec_tt_pair_metrics and its workspace query) are exported, bound, and check
their arguments before any device work."""
import ctypes

_i64, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
P = ctypes.c_void_p(256)  # a non-null, 16-B aligned stand-in: rejected calls never dereference it
NAMES = ("hrec_tt_predict_pairs", "hrec_tt_pair_metrics_workspace_bytes", "hrec_tt_pair_metrics")


def _lib():
    import __graft_entry__ as g
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(g.build_lib())
    lib.hrec_last_error.restype = ctypes.c_char_p
    lib.hrec_abi_version.restype = _int
    model = [_vp, _i64, _vp, _i64, _int, _vp, _vp, _i64]
    lib.hrec_tt_predict_pairs.restype = _int
    lib.hrec_tt_predict_pairs.argtypes = model + [_vp, _vp]
    lib.hrec_tt_pair_metrics_workspace_bytes.restype = _sz
    lib.hrec_tt_pair_metrics_workspace_bytes.argtypes = [_i64]
    lib.hrec_tt_pair_metrics.restype = _int
    lib.hrec_tt_pair_metrics.argtypes = model + [_vp, _vp, _vp, _vp, _sz, _vp]
    return lib


def _predict(lib, U=P, n_u=5, V=P, n_v=5, d=8, ur=P, ir=P, n=3, out=P):
    return lib.hrec_tt_predict_pairs(U, n_u, V, n_v, d, ur, ir, n, out, None)


def _metrics(lib, U=P, n_u=5, V=P, n_v=5, d=8, ur=P, ir=P, n=3, labels=P, pred=None, sums=P, ws=P, ws_bytes=1 << 20):
    return lib.hrec_tt_pair_metrics(U, n_u, V, n_v, d, ur, ir, n, labels, pred, sums, ws, ws_bytes, None)


def test_symbols_are_exported_declared_bound_and_abi_is_still_7():
    import os

    lib = _lib()
    from src import _hrec

    import __graft_entry__ as g

    with open(os.path.join(g.ROOT, "include", "hrec.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(lib, name)
        assert name in _hrec._SIGNATURES and name in _hrec.exported_symbols()
        assert name + "(" in header
    assert lib.hrec_abi_version() == 7
    assert callable(_hrec.tt_predict_pairs) and callable(_hrec.tt_pair_sums)


def test_predict_pairs_rejects_bad_arguments():
    lib = _lib()
    for d in (0, 257, -3):
        assert _predict(lib, d=d) == -1
        assert b"1 <= d <= 256" in lib.hrec_last_error() and b"tt_predict_pairs" in lib.hrec_last_error()
    for kw in ({"n": -1}, {"n_u": -1}, {"n_v": -1}):
        assert _predict(lib, **kw) == -1
        assert b"negative size" in lib.hrec_last_error()
    for kw in ({"ur": None}, {"ir": None}, {"out": None}):
        assert _predict(lib, **kw) == -1
        assert b"null pointer" in lib.hrec_last_error()
    for kw in ({"U": None}, {"V": None}):
        assert _predict(lib, **kw) == -1
        assert b"null vectors" in lib.hrec_last_error()
    # the alignment a width needs: 16 B at d % 4 == 0, 8 B at d % 2 == 0, 4 B otherwise
    for d, addr in ((8, 264), (8, 260), (6, 260), (7, 258)):
        assert _predict(lib, d=d, V=ctypes.c_void_p(addr)) == -1
        assert b"aligned" in lib.hrec_last_error()


def test_predict_pairs_of_no_pairs_is_a_no_op():
    lib = _lib()
    assert _predict(lib, n=0) == 0
    assert _predict(lib, n=0, U=None, V=None, ur=None, ir=None, out=None) == 0
    assert _predict(lib, n=0, d=257) == -1  # the model's shape is still checked


def test_pair_metrics_rejects_bad_arguments():
    lib = _lib()
    for d in (0, 257):
        assert _metrics(lib, d=d) == -1
        assert b"1 <= d <= 256" in lib.hrec_last_error() and b"tt_pair_metrics" in lib.hrec_last_error()
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
    assert b"null vectors" in lib.hrec_last_error()
    need = lib.hrec_tt_pair_metrics_workspace_bytes(70000)
    assert _metrics(lib, n=70000, ws_bytes=need - 1) == -1
    assert b"workspace" in lib.hrec_last_error() and str(need).encode() in lib.hrec_last_error()
    assert _metrics(lib, n=0, ws_bytes=0) == -1  # even no pairs need the (positive) workspace


def test_pair_metrics_workspace_query():
    """One partial of 10 doubles per block; the block count grows with n up
    to the grid cap, is positive at n = 0 and never overflows."""
    lib = _lib()
    f = lib.hrec_tt_pair_metrics_workspace_bytes
    sizes = [f(n) for n in (-5, 0, 1, 256, 257, 70000, 10 ** 6, 5 * 10 ** 8, 2 ** 62)]
    assert all(s >= 80 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes[5] >= (70000 + 255) // 256 * 80  # several blocks take part at n = 70 000
    assert sizes[-1] == sizes[-2] <= 1 << 20      # capped grid
