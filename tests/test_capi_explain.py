"""CPU: hrec_als_explain is declared, exported and bound with the header's
signature; every argument error is reported before any device work (no GPU
needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NAME = "hrec_als_explain"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from src import _hrec

    handle = ctypes.CDLL(g.build_lib())
    for name in (NAME, "hrec_last_error", "hrec_abi_version"):
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
    assert re.search(r"\b%s\s*\(" % NAME, code)
    assert hasattr(lib, NAME)
    assert NAME in _hrec.exported_symbols()
    assert lib.hrec_abi_version() == 7 and _hrec.ABI_VERSION == 7  # additive
    assert "#define HREC_ABI_VERSION 7" in _header()
    assert "#define HREC_EXPLAIN_MAX_TOP 32" in _header()
    assert _hrec.EXPLAIN_MAX_TOP == 32 and _hrec.EXPLAIN_LIST_MAX == 1024
    assert "-> hrec_als_explain" in _header()  # the "replaces" table


def test_signature_matches_the_header():
    from src import _hrec

    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double

    def ctype(param):
        param = param.strip()
        if "*" in param:
            return vp
        return {"int64_t": i64, "int": i32, "double": dbl}[param.rsplit(" ", 1)[0].strip()]

    m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % NAME, code)
    res, args = _hrec._SIGNATURES[NAME]
    assert [ctype(p) for p in m.group(2).split(",")] == list(args)
    assert m.group(1) == "int" and res is i32
    names = [p.strip().rsplit(" ", 1)[1].lstrip("*") for p in m.group(2).split(",")]
    assert names == ["lists", "lists_ld", "list_n", "list_len", "n_rows", "hist_rows", "hist_indptr", "hist_cols",
                     "hist_vals", "item_factors", "n_items", "k", "kp", "reg_param", "implicit", "alpha", "yty",
                     "top_m", "out_total", "out_pos", "out_val", "out_len", "out_row", "stream"]


def _explain(lib, **kw):
    """hrec_als_explain with nothing but the shape (every pointer NULL, or a
    stand-in address that is never dereferenced where the argument checks need one)."""
    a = dict(lists_ld=10, list_n=10, n_rows=3, n_items=100, k=10, kp=16, reg=0.1, implicit=0, alpha=0.0, yty=None,
             top_m=5)
    a.update(kw)
    return lib.hrec_als_explain(None, a["lists_ld"], a["list_n"], None, a["n_rows"], None, None, None, None, None,
                                a["n_items"], a["k"], a["kp"], a["reg"], a["implicit"], a["alpha"], a["yty"],
                                a["top_m"], None, None, None, None, None, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(kp=8), b"kp must be 16, 32 or 64"),
    (dict(kp=96, k=70), b"kp must be 16, 32 or 64 (explanations support rank <= 64; got kp 96)"),
    (dict(kp=128, k=100), b"kp must be 16, 32 or 64"),
    (dict(k=17), b"need 1 <= k <= kp (k=17 kp=16)"),
    (dict(k=0), b"need 1 <= k <= kp (k=0 kp=16)"),
    (dict(top_m=0), b"top_m must be in [1, 32] (got 0)"),
    (dict(top_m=33), b"top_m must be in [1, 32] (got 33)"),
    (dict(list_n=-1), b"list_n must be in [0, 1024] (got -1)"),
    (dict(list_n=1025, lists_ld=2000), b"list_n must be in [0, 1024] (got 1025)"),
    (dict(lists_ld=9), b"lists_ld must be >= list_n"),
    (dict(implicit=2), b"implicit must be 0 or 1"),
    (dict(alpha=-0.5), b"alpha must be >= 0"),
    (dict(alpha=float("nan")), b"alpha must be >= 0"),
    (dict(reg=-1e-3), b"reg_param must be >= 0"),
    (dict(reg=float("nan")), b"reg_param must be >= 0"),
    (dict(n_rows=-1), b"negative size"),
    (dict(n_rows=2 ** 31), b"too many rows"),
    (dict(kp=64, k=64, n_items=2 ** 24 + 1), b"exceed the 4 GiB a gather resource spans"),
    (dict(implicit=1), b"implicit needs yty"),
    (dict(), b"null pointer"),
    (dict(implicit=1, yty=ctypes.c_void_p(256)), b"null pointer"),
])
def test_argument_errors(lib, kw, msg):
    assert _explain(lib, **kw) == -1
    assert msg in lib.hrec_last_error(), lib.hrec_last_error()


def test_nothing_to_do_is_ok(lib):
    assert _explain(lib, n_rows=0) == 0
    assert _explain(lib, list_n=0, lists_ld=0) == 0
    assert _explain(lib, n_rows=0, kp=64, k=64, top_m=32, list_n=1024, lists_ld=1024, implicit=1,
                    yty=ctypes.c_void_p(256)) == 0
    assert _explain(lib, n_rows=0, top_m=0) == -1  # the shape is checked first
    assert _explain(lib, n_rows=0, implicit=1) == -1  # and so is the missing Gramian


def test_model_checks_need_no_device():
    from src.als_model import ALSModel

    with pytest.raises(ValueError, match="top"):
        ALSModel._explain_top(0)
    with pytest.raises(ValueError, match="top"):
        ALSModel._explain_top(33)
    assert ALSModel._explain_top(5) == 5
