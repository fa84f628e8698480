"""CPU: hrec_hybrid_model_f1 (with its workspace query) and
hrec_hybrid_lists_rowwise (whose workspace query is hrec_hybrid_lists') are
declared, exported and bound, additive to ABI 7, and both entries check their
arguments before any device work."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("hrec_hybrid_model_f1_workspace_bytes", "hrec_hybrid_model_f1", "hrec_hybrid_lists_rowwise",
         "hrec_hybrid_lists_workspace_bytes")

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _lib():
    import __graft_entry__ as g

    lib_path = g.build_lib()
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(lib_path)
    lib.hrec_last_error.restype = ctypes.c_char_p
    f = lib.hrec_hybrid_model_f1
    f.restype = _i32
    f.argtypes = [_vp, _vp, _i64, _i64, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                  ctypes.c_size_t, _vp]
    h = lib.hrec_hybrid_lists_rowwise
    h.restype = _i32
    h.argtypes = [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                  ctypes.c_size_t, _vp]
    for q in (lib.hrec_hybrid_model_f1_workspace_bytes, lib.hrec_hybrid_lists_workspace_bytes):
        q.restype = ctypes.c_size_t
        q.argtypes = [_i64, _i64, _i32, _i32]
    return lib


def test_symbols_declared_exported_and_bound():
    from src import _hrec

    with open(os.path.join(ROOT, "include", "hrec.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(hrec_[a-z0-9_]+)\s*\(", text))
    lib = _lib()
    for name in NAMES:
        assert name in declared
        assert hasattr(lib, name)
        assert name in _hrec.exported_symbols()
        assert name in _hrec._SIGNATURES
    assert callable(_hrec.hybrid_model_f1) and callable(_hrec.hybrid_lists_rowwise)
    lib.hrec_abi_version.restype = _i32
    assert lib.hrec_abi_version() == 7
    assert _hrec.ABI_VERSION == 7


P = _vp(4096)  # a never-dereferenced stand-in address (16-B aligned): the checks return before any device work


def _f1(lib, als=P, tt=P, n_rows=4, n=100, ld=100, fb=None, k=10, mode=0, labels=(P, P, P, P), default_wins=0,
        out_f1=P, out_wins=P, out_top=None, overflow=P, ws=P, ws_bytes=1 << 40):
    return lib.hrec_hybrid_model_f1(als, tt, n_rows, n, ld, fb, k, mode, *labels, default_wins, out_f1, out_wins,
                                    out_top, overflow, ws, ws_bytes, None)


def _rowwise(lib, als=P, tt=P, n_rows=4, n=100, ld=100, fb=None, row_wins=P, top_k=10, mode=0,
             excl=(None, None, None), out_idx=P, out_val=P, out_len=P, minmax=None, overflow=P, ws=P,
             ws_bytes=1 << 40):
    return lib.hrec_hybrid_lists_rowwise(als, tt, n_rows, n, ld, fb, row_wins, top_k, mode, *excl, out_idx, out_val,
                                         out_len, minmax, overflow, ws, ws_bytes, None)


def _invalid(call, lib, text, **kw):
    assert call(lib, **kw) == -1, kw
    msg = lib.hrec_last_error()
    assert msg and text in msg, (kw, msg)


def test_model_f1_argument_errors_before_device_work():
    lib = _lib()
    for arg in ("als", "tt", "out_f1", "out_wins", "overflow", "ws"):
        _invalid(_f1, lib, b"hybrid_model_f1: null pointer", **{arg: None})
    for k in (0, -1, 1025):
        _invalid(_f1, lib, b"hybrid_model_f1: k must be in [1, 1024]", k=k)
    _invalid(_f1, lib, b"hybrid_model_f1: ld must be >= n", ld=99)
    for n_rows in (65536, 1 << 20):
        _invalid(_f1, lib, b"hybrid_model_f1: at most 65535 rows", n_rows=n_rows)
    for mode in (-1, 2):
        _invalid(_f1, lib, b"hybrid_model_f1: mode must be 0 or 1", mode=mode)
    for mode in (0, 1):
        need = lib.hrec_hybrid_model_f1_workspace_bytes(4, 100, 10, mode)
        for ws_bytes in (0, need - 1):
            _invalid(_f1, lib, b"hybrid_model_f1: workspace", mode=mode, ws_bytes=ws_bytes)
    for mask in range(1, 15):  # some but not all of the four label pointers
        labels = tuple(P if mask >> b & 1 else None for b in range(4))
        _invalid(_f1, lib, b"hybrid_model_f1: the label CSR needs", labels=labels)
    _invalid(_f1, lib, b"hybrid_model_f1: bad shape", n=0, ld=0)
    _invalid(_f1, lib, b"hybrid_model_f1: bad shape", n_rows=-1)
    # nothing to do: no pointer is looked at
    assert lib.hrec_hybrid_model_f1(None, None, 0, 100, 100, None, 10, 0, None, None, None, None, 0, None, None, None,
                                    None, None, 0, None) == 0


def test_rowwise_argument_errors_before_device_work():
    lib = _lib()
    for arg in ("als", "tt", "row_wins", "out_idx", "out_val", "out_len", "overflow", "ws"):
        _invalid(_rowwise, lib, b"hybrid_lists_rowwise: null pointer", **{arg: None})
    for top_k in (0, -1, 1025):
        _invalid(_rowwise, lib, b"hybrid_lists_rowwise: top_k must be in [1, 1024]", top_k=top_k)
    _invalid(_rowwise, lib, b"hybrid_lists_rowwise: ld must be >= n", ld=99)
    for n_rows in (65536, 1 << 20):
        _invalid(_rowwise, lib, b"hybrid_lists_rowwise: at most 65535 rows", n_rows=n_rows)
    for mode in (-1, 2):
        _invalid(_rowwise, lib, b"hybrid_lists_rowwise: mode must be 0 or 1", mode=mode)
    for mode in (0, 1):
        need = lib.hrec_hybrid_lists_workspace_bytes(4, 100, 10, mode)
        for ws_bytes in (0, need - 1):
            _invalid(_rowwise, lib, b"hybrid_lists_rowwise: workspace", mode=mode, ws_bytes=ws_bytes)
    for excl in ((P, None, None), (None, P, None), (None, None, P), (P, P, None), (P, None, P), (None, P, P)):
        _invalid(_rowwise, lib, b"hybrid_lists_rowwise: the exclusion CSR needs", excl=excl)
    _invalid(_rowwise, lib, b"hybrid_lists_rowwise: bad shape", n=0, ld=0)
    _invalid(_rowwise, lib, b"hybrid_lists_rowwise: bad shape", n_rows=-1)
    assert lib.hrec_hybrid_lists_rowwise(None, None, 0, 100, 100, None, None, 10, 0, None, None, None, None, None,
                                         None, None, None, None, 0, None) == 0


def test_workspace_queries():
    lib = _lib()
    q = lib.hrec_hybrid_model_f1_workspace_bytes
    for n, k in ((1, 1), (100, 10), (4096, 1024), (4097, 8), (100_000, 10), (100_000, 1024)):
        for mode in (0, 1):
            prev = 0
            for n_rows in (0, 1, 2, 3, 64, 65, 1000, 65535):
                need = q(n_rows, n, k, mode)
                assert need >= prev > 0 or (prev == 0 and need > 0)
                prev = need
                if mode == 1:
                    assert need >= 16 * n_rows * n
                # the rowwise lists run in hrec_hybrid_lists' workspace: the shared query is monotone too
                assert lib.hrec_hybrid_lists_workspace_bytes(n_rows, n, k, mode) <= \
                    lib.hrec_hybrid_lists_workspace_bytes(n_rows + 1, n, k, mode)
