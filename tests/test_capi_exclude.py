"""CPU: the seen-item exclusion entries of the C-ABI (hrec_als_score_topk_excluding,
its workspace query, hrec_mask_rows_f32) are exported and bound, check their
arguments before any device work. (The host exclusion builder:
tests/test_exclusion_host.py.)"""
import ctypes

import numpy as np
import pytest

NEW = ("hrec_als_score_topk_excluding", "hrec_als_score_topk_excluding_workspace_bytes", "hrec_mask_rows_f32")
I32, I64, VP, SZ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    handle = ctypes.CDLL(g.build_lib())
    handle.hrec_last_error.restype = ctypes.c_char_p
    f = handle.hrec_als_score_topk_excluding
    f.restype = I32
    f.argtypes = [VP, VP, I32, VP, I64, I64, I32, I32, I32, VP, VP, VP, VP, VP, VP, VP, SZ, VP]
    m = handle.hrec_mask_rows_f32
    m.restype = I32
    m.argtypes = [VP, I64, I64, I64, VP, VP, VP, ctypes.c_float, VP, VP]
    for name in ("hrec_als_score_topk_excluding_workspace_bytes", "hrec_als_score_topk_workspace_bytes"):
        q = getattr(handle, name)
        q.restype = SZ
        q.argtypes = [I32, I64, I32]
    return handle


def test_symbols_are_exported_and_bound(lib):
    from src import _hrec

    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _hrec.exported_symbols(), name
    assert callable(_hrec.als_score_topk_excluding) and callable(_hrec.mask_rows)
    lib.hrec_abi_version.restype = I32
    assert lib.hrec_abi_version() == 7 and _hrec.ABI_VERSION == 7


def test_excluding_argument_checks(lib):
    f = lib.hrec_als_score_topk_excluding
    P = VP(256)  # a non-null stand-in: every call below fails its checks before any pointer is used

    def call(n_users=4, ld=104, n_items=100, k=10, kp=16, top_k=5, ptr=P, indptr=P, cols=P, out_len=P, ws=P,
             ws_bytes=1 << 40):
        return f(ptr, ptr, n_users, ptr, ld, n_items, k, kp, top_k, indptr, cols, ptr, ptr, out_len, ptr, ws, ws_bytes,
                 None)

    for kwargs, msg in (
            (dict(kp=48), b"als_score_topk_excluding: kp must be 16, 32, 64, 96, 128, 192 or 256"),
            (dict(k=17), b"als_score_topk_excluding: need 1 <= k <= kp"),
            (dict(k=0), b"als_score_topk_excluding: need 1 <= k <= kp"),
            (dict(n_users=65536), b"als_score_topk_excluding: bad shape"),
            (dict(n_users=-1), b"als_score_topk_excluding: bad shape"),
            (dict(ld=96), b"als_score_topk_excluding: ld_items must be >= n_items, % 4 and < 2^29"),
            (dict(ld=102), b"als_score_topk_excluding: ld_items must be >= n_items, % 4 and < 2^29"),
            (dict(ld=1 << 29, n_items=10), b"als_score_topk_excluding: ld_items must be >= n_items, % 4 and < 2^29"),
            (dict(top_k=0), b"als_score_topk_excluding: top_k must be in [1, 1024]"),
            (dict(top_k=1025), b"als_score_topk_excluding: top_k must be in [1, 1024]"),
            (dict(ptr=None), b"als_score_topk_excluding: null pointer"),
            (dict(ws=None), b"als_score_topk_excluding: null pointer"),
            (dict(indptr=None), b"als_score_topk_excluding: null exclusion or out_len"),
            (dict(cols=None), b"als_score_topk_excluding: null exclusion or out_len"),
            (dict(out_len=None), b"als_score_topk_excluding: null exclusion or out_len"),
            (dict(ws_bytes=16), b"als_score_topk_excluding: workspace 16 < ")):
        assert call(**kwargs) == -1, kwargs
        assert msg in lib.hrec_last_error(), (kwargs, lib.hrec_last_error())
    assert call(n_users=0, ptr=None, indptr=None, cols=None, out_len=None, ws=None) == 0  # nothing to rank
    assert call(n_items=0, ld=0, ptr=None, indptr=None, cols=None, out_len=None, ws=None) == 0


def test_mask_rows_argument_checks(lib):
    m = lib.hrec_mask_rows_f32
    P = VP(256)
    nan = ctypes.c_float(float("nan"))
    for args, msg in (((P, -1, 10, 10, P, P, P, nan, P, None), b"mask_rows_f32: bad shape"),
                      ((P, 2, -1, 10, P, P, P, nan, P, None), b"mask_rows_f32: bad shape"),
                      ((P, 2, 10, 9, P, P, P, nan, P, None), b"mask_rows_f32: bad shape"),
                      ((P, 2, 1 << 31, 1 << 31, P, P, P, nan, P, None), b"mask_rows_f32: n and n_rows must be < 2^31"),
                      ((P, 1 << 31, 10, 10, P, P, P, nan, P, None), b"mask_rows_f32: n and n_rows must be < 2^31"),
                      ((None, 2, 10, 10, P, P, P, nan, P, None), b"mask_rows_f32: null pointer"),
                      ((P, 2, 10, 10, None, P, P, nan, P, None), b"mask_rows_f32: null pointer"),
                      ((P, 2, 10, 10, P, None, P, nan, P, None), b"mask_rows_f32: null pointer"),
                      ((P, 2, 10, 10, P, P, None, nan, P, None), b"mask_rows_f32: null pointer"),
                      ((P, 2, 10, 10, P, P, P, nan, None, None), b"mask_rows_f32: null pointer")):
        assert m(*args) == -1, args
        assert msg in lib.hrec_last_error(), (args, lib.hrec_last_error())
    assert m(None, 0, 10, 10, None, None, None, nan, None, None) == 0  # no rows


def test_workspace_query(lib):
    q, base = lib.hrec_als_score_topk_excluding_workspace_bytes, lib.hrec_als_score_topk_workspace_bytes
    for n_items in (29, 2048, 2049, 100_000):
        for top_k in (1, 10, 64, 65, 1024):
            prev = 0
            for n_users in (0, 1, 5, 1024, 4096, 65535):
                need = q(n_users, n_items, top_k)
                assert need >= base(n_users, n_items, top_k) > 0
                assert need >= prev
                prev = need
