"""CPU: hrec_tt_fold_in_users is exported, declared, bound, and checks its
arguments before any device work."""
import ctypes

_i64, _int, _vp, _f = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
P = ctypes.c_void_p(256)  # a non-null, 16-B aligned stand-in: rejected calls never dereference it
NAME = "hrec_tt_fold_in_users"


def _lib():
    import __graft_entry__ as g
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(g.build_lib())
    lib.hrec_last_error.restype = ctypes.c_char_p
    lib.hrec_abi_version.restype = _int
    fn = getattr(lib, NAME)
    fn.restype = _int
    fn.argtypes = [_vp, _i64, _int, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _int, _vp, _f, _f, _f, _f, _f, _vp, _vp]
    return lib


def _call(lib, emb=P, n_rows=3, d=8, gamma=P, beta=P, item_vec=P, n_items=5, indptr=P, item_rows=P, ratings=P,
          steps=4, step_lr=P, loss=P):
    return lib.hrec_tt_fold_in_users(emb, n_rows, d, gamma, beta, item_vec, n_items, indptr, item_rows, ratings,
                                     steps, step_lr, 0.9, 0.1, 0.999, 0.001, 1e-7, loss, None)


def test_symbol_is_exported_declared_bound_and_abi_is_still_7():
    import os

    lib = _lib()
    from src import _hrec

    import __graft_entry__ as g

    with open(os.path.join(g.ROOT, "include", "hrec.h")) as f:
        header = f.read()
    assert hasattr(lib, NAME)
    assert NAME in _hrec._SIGNATURES and NAME in _hrec.exported_symbols()
    assert NAME + "(" in header
    assert lib.hrec_abi_version() == 7 and _hrec.ABI_VERSION == 7
    assert callable(_hrec.tt_fold_in_users)
    with open(os.path.join(g.ROOT, "INTEGRATION.md")) as f:
        assert NAME in f.read()


def test_rejects_bad_arguments():
    lib = _lib()
    for d in (0, 257, -3):
        assert _call(lib, d=d) == -1
        assert b"1 <= d <= 256" in lib.hrec_last_error() and b"tt_fold_in_users" in lib.hrec_last_error()
    for kw in ({"n_rows": -1}, {"n_items": -1}, {"steps": -1}):
        assert _call(lib, **kw) == -1
        assert b"negative size" in lib.hrec_last_error()
    for name in ("emb", "gamma", "beta", "indptr", "item_rows", "ratings", "step_lr"):
        assert _call(lib, **{name: None}) == -1, name
        assert b"null pointer" in lib.hrec_last_error()
    assert _call(lib, item_vec=None) == -1
    assert b"null vectors" in lib.hrec_last_error()
    # hrec_tt_predict_pairs' rule: 16 B at d % 4 == 0, 8 B at d % 2 == 0, 4 B otherwise
    for d, addr in ((8, 264), (8, 260), (6, 260), (7, 258)):
        for name in ("emb", "item_vec"):
            assert _call(lib, d=d, **{name: ctypes.c_void_p(addr)}) == -1
            assert b"aligned" in lib.hrec_last_error()


def test_no_rows_is_a_no_op():
    lib = _lib()
    assert _call(lib, n_rows=0) == 0
    assert _call(lib, n_rows=0, emb=None, gamma=None, beta=None, item_vec=None, indptr=None, item_rows=None,
                 ratings=None, step_lr=None, loss=None) == 0
    assert _call(lib, n_rows=0, d=257) == -1  # the shape is still checked
