"""CPU: hrec_row_inv_norms, hrec_list_quality and the workspace query are
declared, exported and bound; every argument error is reported before any
device work (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NAMES = ("hrec_row_inv_norms", "hrec_list_quality_workspace_bytes", "hrec_list_quality")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from src import _hrec

    handle = ctypes.CDLL(g.build_lib())
    for name in NAMES + ("hrec_last_error", "hrec_abi_version"):
        res, args = _hrec._SIGNATURES[name]
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


def _header():
    with open(os.path.join(ROOT, "include", "hrec.h")) as f:
        return f.read()


def test_declared_exported_and_bound(lib):
    from src import _hrec

    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name)
        assert name in _hrec.exported_symbols()
    assert lib.hrec_abi_version() == 7 and _hrec.ABI_VERSION == 7
    assert "#define HREC_ABI_VERSION 7" in _header()
    assert "#define HREC_LQ_MAX_TABLES 4" in _header() and _hrec.LQ_MAX_TABLES == 4


def test_signatures_match_the_header():
    """_SIGNATURES' argtypes against the parameter types the header declares."""
    from src import _hrec

    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t

    def ctype(param):
        param = param.strip()
        if "*" in param:
            return vp
        return {"int64_t": i64, "int": i32, "size_t": sz}[param.rsplit(" ", 1)[0].strip()]

    for name in NAMES:
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % name, code)
        res, args = _hrec._SIGNATURES[name]
        assert [ctype(p) for p in m.group(2).split(",")] == list(args), name
        assert {"int": i32, "size_t": sz}[m.group(1)] is res, name


def _lq(lib, **kw):
    """hrec_list_quality with nothing but the shape (every pointer NULL)."""
    a = dict(lists_ld=10, list_n=10, n_rows=3, n=100, d=8, ld=8, n_tab=0, ws=0)
    a.update(kw)
    return lib.hrec_list_quality(None, a["lists_ld"], a["list_n"], None, a["n_rows"], a["n"], None, a["d"], a["ld"],
                                 None, None, None, None, None, a["n_tab"], None, None, None, None, None, a["ws"],
                                 None)


@pytest.mark.parametrize("kw,msg", [
    (dict(d=0), b"d must be in [1, 256] (got 0)"),
    (dict(d=257, ld=300), b"d must be in [1, 256] (got 257)"),
    (dict(d=50, ld=49), b"ld must be >= d"),
    (dict(list_n=-1), b"list_n must be in [0, 1024] (got -1)"),
    (dict(list_n=1025, lists_ld=2000), b"list_n must be in [0, 1024] (got 1025)"),
    (dict(list_n=10, lists_ld=9), b"lists_ld must be >= list_n"),
    (dict(n_tab=-1), b"n_tab must be in [0, 4] (got -1)"),
    (dict(n_tab=5), b"n_tab must be in [0, 4] (got 5)"),
    (dict(n=2 ** 31), b"n must be in [1, 2^31)"),
    (dict(n=0), b"n must be in [1, 2^31)"),
    (dict(ws=0), b"workspace 0 < 256"),
    (dict(n_rows=9, ws=256), b"workspace 256 < 512"),
])
def test_list_quality_argument_errors(lib, kw, msg):
    assert _lq(lib, **kw) == -1
    assert msg in lib.hrec_last_error(), lib.hrec_last_error()


def test_list_quality_history_needs_all_three(lib):
    rc = lib.hrec_list_quality(None, 10, 10, None, 3, 100, None, 8, 8, None, ctypes.c_void_p(256), None, None, None, 0,
                               None, None, None, None, None, 0, None)
    assert rc == -1 and b"hist_rows, hist_indptr and hist_cols" in lib.hrec_last_error()


def test_no_rows_is_ok_and_null_pointers_are_not(lib):
    assert _lq(lib, n_rows=0) == 0
    assert _lq(lib, n_rows=0, list_n=0, lists_ld=0, n_tab=4) == 0
    assert _lq(lib, ws=4096) == -1
    assert b"null pointer" in lib.hrec_last_error()


def test_workspace_query(lib):
    q = lib.hrec_list_quality_workspace_bytes
    assert q(0) == q(1) == q(4) == 256  # one block: 12 slots of 8 bytes, rounded to 256
    assert q(5) == 256 and q(11) == 512
    assert q(1 << 20) >= (1 << 18) * 12 * 8


@pytest.mark.parametrize("args,msg", [
    ((None, 10, 0, 8, None, None), b"d must be in [1, 256] (got 0)"),
    ((None, 10, 300, 300, None, None), b"d must be in [1, 256] (got 300)"),
    ((None, 10, 50, 49, None, None), b"ld must be >= d"),
    ((None, 2 ** 31, 8, 8, None, None), b"n must be in [0, 2^31)"),
    ((None, 10, 8, 8, None, None), b"null pointer"),
])
def test_row_inv_norms_argument_errors(lib, args, msg):
    assert lib.hrec_row_inv_norms(*args) == -1
    assert msg in lib.hrec_last_error()


def test_row_inv_norms_no_rows(lib):
    assert lib.hrec_row_inv_norms(None, 0, 8, 8, None, None) == 0
