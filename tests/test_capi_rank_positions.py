"""CPU: hrec_rank_positions (with its workspace query) is declared, exported and
bound, additive to ABI 7, and checks its arguments before any device work."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("hrec_rank_positions_workspace_bytes", "hrec_rank_positions")

_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _lib():
    import __graft_entry__ as g

    lib_path = g.build_lib()
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(lib_path)
    lib.hrec_last_error.restype = ctypes.c_char_p
    f = lib.hrec_rank_positions
    f.restype = _i32
    f.argtypes = [_i64, _i64, _i32, _vp, _vp, _i64] + [_vp] * 15 + [ctypes.c_size_t, _vp]
    q = lib.hrec_rank_positions_workspace_bytes
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
    assert _hrec._SIGNATURES["hrec_rank_positions"][1] == lib.hrec_rank_positions.argtypes
    assert callable(_hrec.rank_positions)
    lib.hrec_abi_version.restype = _i32
    assert lib.hrec_abi_version() == 7
    assert _hrec.ABI_VERSION == 7
    defs = dict(re.findall(r"#define (HREC_RP_[A-Z0-9_]+) (\d+)", raw))
    assert int(defs["HREC_RP_CHUNK"]) == _hrec.RP_CHUNK
    assert int(defs["HREC_RP_SUMS"]) == len(_hrec.RP_SUMS)
    assert len(_hrec.RP_ROW) == 4 and len(_hrec.RP_ROW_N) == 3


P = _vp(4096)  # a never-dereferenced stand-in address: the checks return before any device work
LAB = (P, P, P)


def _rp(lib, n_rows=4, n=100, source=0, scores=P, tt=None, ld=100, fb=None, minmax=None, wins=None, lab=LAB,
        weight=None, excl=(None, None, None), out_rank=P, out_row=P, out_row_n=P, sums=P, ws=P, ws_bytes=1 << 40):
    return lib.hrec_rank_positions(n_rows, n, source, scores, tt, ld, fb, minmax, wins, *lab, weight, *excl, out_rank,
                                   out_row, out_row_n, sums, ws, ws_bytes, None)


def _invalid(lib, text, **kw):
    assert _rp(lib, **kw) == -1, kw
    msg = lib.hrec_last_error()
    assert msg and text in msg, (kw, msg)


def test_argument_errors_before_device_work():
    lib = _lib()
    for arg in ("scores", "out_row", "out_row_n", "sums", "ws"):
        _invalid(lib, b"rank_positions: null pointer", **{arg: None})
    _invalid(lib, b"rank_positions: ld must be >= n", ld=99)
    for source in (-1, 4):
        _invalid(lib, b"rank_positions: source must be in [0, 3]", source=source)
    for missing in ("tt", "minmax", "wins"):
        kw = {"tt": P, "minmax": P, "wins": P}
        kw[missing] = None
        _invalid(lib, b"rank_positions: the fused source needs", source=3, **kw)
    for mask in range(1, 7):  # some but not all of a CSR's three pointers
        part = tuple(P if mask >> b & 1 else None for b in range(3))
        _invalid(lib, b"rank_positions: the label CSR needs", lab=part)
        _invalid(lib, b"rank_positions: the exclusion CSR needs", excl=part)
    _invalid(lib, b"rank_positions: label_weight without a label CSR", lab=(None,) * 3, weight=P)
    need = lib.hrec_rank_positions_workspace_bytes(4)
    for ws_bytes in (0, need - 1):
        _invalid(lib, b"rank_positions: workspace", ws_bytes=ws_bytes)
    _invalid(lib, b"rank_positions: bad shape", n=0, ld=0)
    _invalid(lib, b"rank_positions: bad shape", n_rows=-1)
    _invalid(lib, b"rank_positions: bad shape", n=1 << 31, ld=1 << 31)
    # nothing to do: no device pointer is looked at
    assert _rp(lib, n_rows=0, scores=None, lab=(None,) * 3, out_rank=None, out_row=None, out_row_n=None, sums=None,
               ws=None, ws_bytes=0) == 0


def test_workspace_query_is_monotone():
    lib = _lib()
    prev = 0
    for n_rows in (0, 1, 255, 256, 257, 1000, 65535, 65536, 1 << 20):
        need = lib.hrec_rank_positions_workspace_bytes(n_rows)
        assert need >= prev and need > 0
        assert need >= ((n_rows + 255) // 256) * 10 * 8  # one partial per block of 256 rows and slot
        prev = need
