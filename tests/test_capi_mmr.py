"""CPU: hrec_mmr_rerank is declared, exported and bound with the header's
signature; every argument error is reported before any device work (no GPU
needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NAMES = ("hrec_mmr_rerank",)


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
    assert not hasattr(lib, "hrec_mmr_rerank_workspace_bytes")  # the kernel needs no workspace
    assert lib.hrec_abi_version() == 7 and _hrec.ABI_VERSION == 7  # additive
    assert "#define HREC_ABI_VERSION 7" in _header()
    assert _hrec.MMR_POOL_MAX == 1024


def test_signature_matches_the_header():
    from src import _hrec

    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    vp, i64, i32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double

    def ctype(param):
        param = param.strip()
        if "*" in param:
            return vp
        return {"int64_t": i64, "int": i32, "double": dbl}[param.rsplit(" ", 1)[0].strip()]

    m = re.search(r"(\w+)\s+hrec_mmr_rerank\s*\(([^)]*)\)", code)
    res, args = _hrec._SIGNATURES["hrec_mmr_rerank"]
    assert [ctype(p) for p in m.group(2).split(",")] == list(args)
    assert m.group(1) == "int" and res is i32
    names = [p.strip().rsplit(" ", 1)[1].lstrip("*") for p in m.group(2).split(",")]
    assert names == ["pool", "pool_ld", "pool_n", "pool_len", "scores", "scores_f64", "scores_ld", "n_rows", "n",
                     "vectors", "d", "ld", "inv_norm", "lambda", "top_n", "out_pos", "out_len", "out_value", "stream"]


def _mmr(lib, **kw):
    """hrec_mmr_rerank with nothing but the shape (every pointer NULL)."""
    a = dict(pool_ld=100, pool_n=100, f64=0, scores_ld=100, n_rows=3, n=1000, d=8, ld=8, lam=0.5, top_n=10)
    a.update(kw)
    return lib.hrec_mmr_rerank(None, a["pool_ld"], a["pool_n"], None, None, a["f64"], a["scores_ld"], a["n_rows"],
                               a["n"], None, a["d"], a["ld"], None, a["lam"], a["top_n"], None, None, None, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(d=0), b"d must be in [1, 256] (got 0)"),
    (dict(d=257, ld=300), b"d must be in [1, 256] (got 257)"),
    (dict(d=50, ld=49), b"ld must be >= d"),
    (dict(pool_n=0), b"pool_n must be in [1, 1024] (got 0)"),
    (dict(pool_n=1025, pool_ld=2000, scores_ld=2000), b"pool_n must be in [1, 1024] (got 1025)"),
    (dict(top_n=0), b"top_n must be in [1, pool_n] (got 0)"),
    (dict(top_n=101), b"top_n must be in [1, pool_n] (got 101)"),
    (dict(pool_ld=99), b"pool_ld must be >= pool_n"),
    (dict(scores_ld=99), b"scores_ld must be >= pool_n"),
    (dict(f64=2), b"scores_f64 must be 0 or 1"),
    (dict(lam=-0.01), b"lambda must be in [0, 1]"),
    (dict(lam=1.01), b"lambda must be in [0, 1]"),
    (dict(lam=float("nan")), b"lambda must be in [0, 1]"),
    (dict(n=0), b"n must be in [1, 2^31)"),
    (dict(n=2 ** 31), b"n must be in [1, 2^31)"),
    (dict(n_rows=-1), b"bad shape"),
    (dict(n_rows=2 ** 31), b"bad shape"),
    (dict(), b"null pointer"),
])
def test_argument_errors(lib, kw, msg):
    assert _mmr(lib, **kw) == -1
    assert msg in lib.hrec_last_error(), lib.hrec_last_error()


def test_no_rows_is_ok(lib):
    assert _mmr(lib, n_rows=0) == 0
    assert _mmr(lib, n_rows=0, pool_n=1024, pool_ld=1024, scores_ld=1024, top_n=1024, d=256, ld=256, f64=1) == 0
    assert _mmr(lib, n_rows=0, top_n=0) == -1  # the shape is checked first


def test_mmr_class_and_wrapper_checks():
    from src import ranked_lists

    m = ranked_lists.MMR()
    assert (m.lambda_, m.pool) == (0.7, 100)
    assert ranked_lists.MMR(0, 1).pool == 1 and ranked_lists.MMR(1, 1024).lambda_ == 1.0
    for bad in (dict(lambda_=-0.1), dict(lambda_=1.5), dict(lambda_=float("nan")), dict(pool=0), dict(pool=1025)):
        with pytest.raises(ValueError):
            ranked_lists.MMR(**bad)
    with pytest.raises(TypeError):
        ranked_lists.check_mmr(0.5)
