"""CPU: hrec_user_metrics (with its workspace query) is declared, exported and
bound, additive to ABI 7, and checks its arguments before any device work."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("hrec_user_metrics_workspace_bytes", "hrec_user_metrics")

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _lib():
    import __graft_entry__ as g

    lib_path = g.build_lib()
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(lib_path)
    lib.hrec_last_error.restype = ctypes.c_char_p
    f = lib.hrec_user_metrics
    f.restype = _i32
    f.argtypes = [_vp, _i64, _i32, _vp, _i64, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp,
                  _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
    q = lib.hrec_user_metrics_workspace_bytes
    q.restype = ctypes.c_size_t
    q.argtypes = [_i64]
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
    assert _hrec._SIGNATURES["hrec_user_metrics"][1] == lib.hrec_user_metrics.argtypes
    assert callable(_hrec.user_metrics)
    lib.hrec_abi_version.restype = _i32
    assert lib.hrec_abi_version() == 7
    assert _hrec.ABI_VERSION == 7
    # the names of the status bits and of the sums follow the header
    defs = dict(re.findall(r"#define (HREC_UM_[A-Z0-9_]+) (\d+)", raw))
    assert int(defs["HREC_UM_MAX_K"]) == _hrec.UM_MAX_K
    assert int(defs["HREC_UM_STATUS_BITS"]) == len(_hrec.UM_STATUS)
    for b, s in enumerate(_hrec.UM_STATUS):
        assert int(defs["HREC_UM_" + s.upper()]) == 1 << b == getattr(_hrec, "UM_" + s.upper())
    for s, v in _hrec.UM_SOURCES.items():
        assert int(defs["HREC_UM_SRC_" + s.upper()]) == v
    ks = (5, 10, 15, 20)
    assert _hrec.um_columns(ks)[:2] == ["Precision@5", "Precision@10"] and _hrec.um_columns(ks)[-3:] == \
        ["NDCG", "MAE", "RMSE"]
    assert len(_hrec.um_sums(ks)) == 2 * (2 * len(ks) + 3) + len(_hrec.UM_STATUS)


P = _vp(4096)  # a never-dereferenced stand-in address: the checks return before any device work
ACT = (P, P, P, P, P)


def _um(lib, ranked=P, ranked_ld=20, list_n=20, list_len=None, n_rows=4, n=100, ks=(5, 10, 15, 20), n_k=None,
        ndcg_k=10, cs=P, act=ACT, source=0, scores=P, tt=None, ld=100, fb=None, minmax=None, wins=None, per_row=P,
        status=P, sums=P, ws=P, ws_bytes=1 << 40):
    k_arr = (ctypes.c_int32 * max(len(ks), 1))(*ks) if ks is not None else None
    return lib.hrec_user_metrics(ranked, ranked_ld, list_n, list_len, n_rows, n,
                                 ctypes.cast(k_arr, _vp) if k_arr is not None else None,
                                 len(ks) if n_k is None else n_k, ndcg_k, cs, *act, source, scores, tt, ld, fb, minmax,
                                 wins, per_row, status, sums, ws, ws_bytes, None)


def _invalid(lib, text, **kw):
    assert _um(lib, **kw) == -1, kw
    msg = lib.hrec_last_error()
    assert msg and text in msg, (kw, msg)


def test_argument_errors_before_device_work():
    lib = _lib()
    for arg in ("ranked", "cs", "scores", "per_row", "status", "sums", "ws"):
        _invalid(lib, b"user_metrics: null pointer", **{arg: None})
    _invalid(lib, b"user_metrics: null pointer", ks=None, n_k=4)
    for k in (0, -1, 1025):
        _invalid(lib, b"user_metrics: k must be in [1, 1024]", ks=(5, k))
        _invalid(lib, b"user_metrics: ndcg_k must be in [1, 1024]", ndcg_k=k)
    _invalid(lib, b"user_metrics: n_k must be in [1, 8]", ks=tuple(range(1, 10)))
    _invalid(lib, b"user_metrics: n_k must be in [1, 8]", ks=(), n_k=0)
    _invalid(lib, b"user_metrics: ld must be >= n", ld=99)
    _invalid(lib, b"user_metrics: ranked_ld must be >= list_n", ranked_ld=19)
    for list_n in (-1, 1025):
        _invalid(lib, b"user_metrics: list_n must be in [0, 1024]", list_n=list_n, ranked_ld=2048)
    for n_rows in (65536, 1 << 20):
        _invalid(lib, b"user_metrics: at most 65535 rows", n_rows=n_rows)
    for source in (-1, 4):
        _invalid(lib, b"user_metrics: source must be in [0, 3]", source=source)
    for mask in range(1, 31):  # some but not all of the five CSR pointers
        act = tuple(P if mask >> b & 1 else None for b in range(5))
        _invalid(lib, b"user_metrics: the actual CSR needs", act=act)
    for missing in ("tt", "minmax", "wins"):
        kw = {"tt": P, "minmax": P, "wins": P}
        kw[missing] = None
        _invalid(lib, b"user_metrics: the fused source needs", source=3, **kw)
    need = lib.hrec_user_metrics_workspace_bytes(4)
    for ws_bytes in (0, need - 1):
        _invalid(lib, b"user_metrics: workspace", ws_bytes=ws_bytes)
    _invalid(lib, b"user_metrics: bad shape", n=0, ld=0)
    _invalid(lib, b"user_metrics: bad shape", n_rows=-1)
    # nothing to do: no device pointer is looked at
    assert _um(lib, ranked=None, n_rows=0, cs=None, act=(None,) * 5, scores=None, per_row=None, status=None,
               sums=None, ws=None, ws_bytes=0) == 0


def test_workspace_query_is_monotone():
    lib = _lib()
    prev = 0
    for n_rows in (0, 1, 2, 3, 4, 5, 64, 65, 1000, 65535):
        need = lib.hrec_user_metrics_workspace_bytes(n_rows)
        assert need >= prev and need > 0
        # one partial per block of four rows and slot
        assert need >= ((n_rows + 3) // 4) * (2 * (2 * 8 + 3) + 5) * 8
        prev = need
