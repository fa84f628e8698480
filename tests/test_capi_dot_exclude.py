"""CPU: hrec_dot_topk_excluding is declared, exported and bound, additive to
ABI 7, and checks its arguments before any device work."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("hrec_dot_topk_excluding_workspace_bytes", "hrec_dot_topk_excluding")

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _lib():
    import __graft_entry__ as g

    lib_path = g.build_lib()
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(lib_path)
    lib.hrec_last_error.restype = ctypes.c_char_p
    f = lib.hrec_dot_topk_excluding
    f.restype = _i32
    f.argtypes = [_vp, _i32, _vp, _i64, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                  ctypes.c_size_t, _vp]
    for name in ("hrec_dot_topk_workspace_bytes", "hrec_dot_topk_excluding_workspace_bytes"):
        q = getattr(lib, name)
        q.restype = ctypes.c_size_t
        q.argtypes = [_i32, _i64, _i32]
    return lib


def test_symbols_declared_exported_and_bound():
    from src import _hrec

    with open(os.path.join(ROOT, "include", "hrec.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(hrec_[a-z0-9_]+)\s*\(", text))
    lib = _lib()
    for name in NAMES:
        assert name in declared
        assert hasattr(lib, name)
        assert name in _hrec.exported_symbols()
        assert name in _hrec._SIGNATURES
    assert callable(_hrec.dot_topk_excluding)
    lib.hrec_abi_version.restype = _i32
    assert lib.hrec_abi_version() == 7
    assert _hrec.ABI_VERSION == 7


def _call(lib, n_users=4, n_items=100, dk=64, top_k=10, excl=(True, True, True), out_len=True):
    """Never-dereferenced stand-in addresses (16-B aligned): the argument
    checks return before any device work."""
    p = _vp(4096)
    rows, indptr, cols = (p if on else None for on in excl)
    return lib.hrec_dot_topk_excluding(p, n_users, p, n_items, dk, 0, top_k, None, 0, rows, indptr, cols, p, p,
                                       p if out_len else None, p, p, 0, None)


def test_argument_errors_before_device_work():
    lib = _lib()
    for top_k in (0, 1025):
        assert _call(lib, top_k=top_k) == -1
        assert b"top_k must be in [1, 1024]" in lib.hrec_last_error()
    assert _call(lib, dk=48) == -1
    assert b"dk must be 32, 64, 128 or 256" in lib.hrec_last_error()
    for excl, out_len in (((False, True, True), True), ((True, False, True), True), ((True, True, False), True),
                          ((True, True, True), False)):
        assert _call(lib, excl=excl, out_len=out_len) == -1
        assert b"dot_topk_excluding: null exclusion pointer or out_len" in lib.hrec_last_error()
    # nothing to do: no pointer is looked at
    assert lib.hrec_dot_topk_excluding(None, 0, None, 100, 64, 0, 10, None, 0, None, None, None, None, None, None,
                                       None, None, 0, None) == 0


def test_workspace_query_covers_dot_topk():
    lib = _lib()
    for n_users, n_items, top_k in ((1, 10, 5), (3, 300, 10), (130, 16384, 64), (130, 16385, 65), (4096, 100000, 10),
                                    (20, 70000, 1024), (0, 0, 1)):
        assert (lib.hrec_dot_topk_excluding_workspace_bytes(n_users, n_items, top_k)
                >= lib.hrec_dot_topk_workspace_bytes(n_users, n_items, top_k) > 0)
