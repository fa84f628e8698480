"""CPU: the five new names (hrec_cosine_topk, hrec_cosine_items, their two
size queries and the diagnostic hrec_cosine_topk_counts) are declared,
exported and bound with the header's signatures; every argument error is
reported before any device work; the Python mirrors of the library's constants
agree with its source (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NAMES = ("hrec_cosine_topk", "hrec_cosine_items", "hrec_cosine_items_bytes", "hrec_cosine_topk_workspace_bytes",
         "hrec_cosine_topk_counts")


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
    assert lib.hrec_abi_version() == 7 and _hrec.ABI_VERSION == 7  # additive
    assert "#define HREC_ABI_VERSION 7" in _header()
    assert _hrec.COSINE_TOP_MAX == 1024
    assert _hrec.COSINE_MODES == {"auto": 0, "exhaustive": 1, "pruned": 2}


HEADER_NAMES = {
    "hrec_cosine_topk": ["vectors", "n", "d", "ld", "inv_norm", "query_rows", "n_q", "top_k", "skip_self", "min_sim",
                         "mode", "items", "out_idx", "out_val", "out_len", "overflow", "workspace",
                         "workspace_bytes", "stream"],
    "hrec_cosine_items": ["vectors", "n", "d", "ld", "inv_norm", "out", "stream"],
    "hrec_cosine_items_bytes": ["n", "d"],
    "hrec_cosine_topk_workspace_bytes": ["n_q", "n", "top_k", "d", "mode"],
    "hrec_cosine_topk_counts": ["workspace", "n_q", "n", "top_k", "d", "out", "stream"],
}


@pytest.mark.parametrize("name", NAMES)
def test_signature_matches_the_header(name):
    from src import _hrec

    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    vp, i64, i32, dbl, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_size_t

    def ctype(param):
        param = param.strip()
        if "*" in param:
            return vp
        return {"int64_t": i64, "int": i32, "double": dbl, "size_t": sz}[param.rsplit(" ", 1)[0].strip()]

    m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % name, code)
    res, args = _hrec._SIGNATURES[name]
    assert [ctype(p) for p in m.group(2).split(",")] == list(args)
    assert {"int": i32, "size_t": sz}[m.group(1)] is res
    names = [p.strip().rsplit(" ", 1)[1].lstrip("*") for p in m.group(2).split(",")]
    assert names == HEADER_NAMES[name]


def _topk(lib, **kw):
    """hrec_cosine_topk with nothing but the shape (every pointer NULL)."""
    a = dict(n=1000, d=8, ld=8, n_q=3, top_k=10, skip_self=1, min_sim=float("-inf"), mode=0)
    a.update(kw)
    return lib.hrec_cosine_topk(None, a["n"], a["d"], a["ld"], None, None, a["n_q"], a["top_k"], a["skip_self"],
                                a["min_sim"], a["mode"], None, None, None, None, None, None, 0, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(d=0), b"cosine_topk: d must be in [1, 256] (got 0)"),
    (dict(d=257, ld=300), b"cosine_topk: d must be in [1, 256] (got 257)"),
    (dict(d=50, ld=49), b"cosine_topk: ld must be >= d"),
    (dict(n=0), b"cosine_topk: n must be in [1, 2^31)"),
    (dict(n=2 ** 31), b"cosine_topk: n must be in [1, 2^31)"),
    (dict(n_q=-1), b"cosine_topk: n_q must be in [0, 65536)"),
    (dict(n_q=65536), b"cosine_topk: n_q must be in [0, 65536)"),
    (dict(top_k=0), b"cosine_topk: top_k must be in [1, 1024] (got 0)"),
    (dict(top_k=1025), b"cosine_topk: top_k must be in [1, 1024] (got 1025)"),
    (dict(skip_self=2), b"cosine_topk: skip_self must be 0 or 1"),
    (dict(skip_self=-1), b"cosine_topk: skip_self must be 0 or 1"),
    (dict(min_sim=float("nan")), b"cosine_topk: min_sim must not be NaN"),
    (dict(mode=3), b"cosine_topk: mode must be 0, 1 or 2"),
    (dict(mode=-1), b"cosine_topk: mode must be 0, 1 or 2"),
    (dict(), b"cosine_topk: null pointer"),
    (dict(mode=1), b"cosine_topk: null pointer"),
    (dict(mode=2), b"cosine_topk: null pointer"),
])
def test_topk_argument_errors(lib, kw, msg):
    assert _topk(lib, **kw) == -1
    assert msg in lib.hrec_last_error(), lib.hrec_last_error()


def test_topk_order_of_the_checks(lib):
    assert _topk(lib, d=0, top_k=0) == -1 and b"d must be" in lib.hrec_last_error()  # the shape first
    assert _topk(lib, top_k=0, mode=9) == -1 and b"top_k must be" in lib.hrec_last_error()  # ranges in order
    assert _topk(lib, n_q=0, top_k=0) == -1  # ranges before the empty call
    assert _topk(lib, n_q=0, min_sim=float("nan")) == -1


def test_no_queries_is_ok(lib):
    for mode in (0, 1, 2):
        assert _topk(lib, n_q=0, mode=mode) == 0
    assert _topk(lib, n_q=0, n=2 ** 31 - 1, d=256, ld=256, top_k=1024, skip_self=0, min_sim=0.5) == 0


def _items(lib, **kw):
    a = dict(n=1000, d=8, ld=8)
    a.update(kw)
    return lib.hrec_cosine_items(None, a["n"], a["d"], a["ld"], None, None, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(d=0), b"cosine_items: d must be in [1, 256] (got 0)"),
    (dict(d=257, ld=257), b"cosine_items: d must be in [1, 256] (got 257)"),
    (dict(ld=7), b"cosine_items: ld must be >= d"),
    (dict(n=-1), b"cosine_items: n must be in [0, 2^31)"),
    (dict(n=2 ** 31), b"cosine_items: n must be in [0, 2^31)"),
    (dict(), b"cosine_items: null pointer"),
])
def test_items_argument_errors(lib, kw, msg):
    assert _items(lib, **kw) == -1
    assert msg in lib.hrec_last_error(), lib.hrec_last_error()


def test_items_empty_is_ok_and_sizes(lib):
    assert _items(lib, n=0) == 0
    # bf16 rows padded to 32, 64, 128 or 256 columns (+ a 256-B tail)
    for d, dk in ((1, 32), (32, 32), (33, 64), (50, 64), (64, 64), (65, 128), (128, 128), (129, 256), (256, 256)):
        assert lib.hrec_cosine_items_bytes(1000, d) == ((1000 * dk * 2 + 255) // 256) * 256 + 256
    assert lib.hrec_cosine_items_bytes(0, 64) == 256


def test_counts_argument_errors(lib):
    counts = lib.hrec_cosine_topk_counts
    assert counts(None, 0, 1000, 10, 64, None, None) == 0
    assert counts(None, 3, 1000, 10, 64, None, None) == -1 and b"cosine_topk_counts: null pointer" in lib.hrec_last_error()
    for bad in ((3, 0, 10, 64), (3, 1000, 0, 64), (3, 1000, 10, 257), (65536, 1000, 10, 64)):
        assert counts(None, *bad, None, None) == -1 and b"cosine_topk_counts: bad shape" in lib.hrec_last_error()


def test_workspace_sizes(lib):
    ws = lib.hrec_cosine_topk_workspace_bytes
    # the exhaustive arm holds a sub-batch of f64 sim rows: at least one row, never much more than 512 MiB of them
    assert ws(1, 100000, 10, 64, 1) >= 100000 * 8
    assert ws(4096, 100000, 10, 64, 1) < (3 << 28)
    assert ws(4096, 1 << 27, 10, 64, 1) >= (1 << 27) * 8  # one row is 1 GiB: a sub-batch of one query
    # auto covers whichever arm it may take
    for n in (100, 5000, 100000):
        assert ws(256, n, 10, 64, 0) >= ws(256, n, 10, 64, 1)
    assert ws(256, 100000, 10, 64, 0) >= ws(256, 100000, 10, 64, 2)
    assert ws(0, 1000, 10, 64, 0) > 0


def test_python_constants_mirror_the_library_source():
    from src import _hrec

    with open(os.path.join(ROOT, "hybrid-als-twotower-recommender_amd", "csrc", "cosine_topk.hip")) as f:
        src = f.read()

    def const(name):
        return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))

    assert _hrec.COSINE_AUTO_CUT == const("kCosAutoCut")
    assert _hrec.COSINE_CAP == const("kCosCap")
    assert _hrec.COSINE_TOP_MAX == const("kCosTopMax")


def test_wrapper_checks():
    from src import ranked_lists

    for bad in (0, 1025, -3):
        with pytest.raises(ValueError):
            ranked_lists.check_num(bad, ranked_lists.SIMILAR_MAX)
    assert ranked_lists.SIMILAR_MAX == 1024 and ranked_lists.SIMILAR_BATCH == 4096
