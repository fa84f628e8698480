"""CPU: the bf16-pruned seen-item exclusion entry of the C-ABI
(hrec_als_score_topk_pruned_excluding and its workspace query) is declared in
include/hrec.h, exported and bound, checks its arguments before any device
work (the argument checks of hrec_als_score_topk_excluding and the operand
checks of hrec_als_score_topk_pruned), and its workspace query covers both of
those entries' needs."""
import ctypes
import os
import re

import pytest

NEW = ("hrec_als_score_topk_pruned_excluding", "hrec_als_score_topk_pruned_excluding_workspace_bytes")
I32, I64, VP, SZ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    handle = ctypes.CDLL(g.build_lib())
    handle.hrec_last_error.restype = ctypes.c_char_p
    f = handle.hrec_als_score_topk_pruned_excluding
    f.restype = I32
    f.argtypes = [VP, VP, I32, VP, I64, VP, I64, VP, I64, I32, I32, I32, VP, VP, VP, VP, VP, VP, VP, SZ, VP]
    for name in ("hrec_als_score_topk_pruned_excluding_workspace_bytes", "hrec_als_score_topk_pruned_workspace_bytes"):
        q = getattr(handle, name)
        q.restype = SZ
        q.argtypes = [I32, I64, I32, I32]
    q = handle.hrec_als_score_topk_excluding_workspace_bytes
    q.restype = SZ
    q.argtypes = [I32, I64, I32]
    return handle


def test_symbols_are_declared_exported_and_bound(lib):
    from src import _hrec

    with open(os.path.join(ROOT, "include", "hrec.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in _hrec.exported_symbols(), name
    assert callable(_hrec.als_score_topk_pruned_excluding)
    lib.hrec_abi_version.restype = I32
    assert lib.hrec_abi_version() == 7 and _hrec.ABI_VERSION == 7
    assert "#define HREC_ABI_VERSION 7" in header


def test_argument_checks(lib):
    f = lib.hrec_als_score_topk_pruned_excluding
    P = VP(256)  # a non-null, 256-B aligned stand-in: every call below fails its checks before any pointer is used

    def call(n_users=4, ld=104, n_items=100, k=10, kp=16, top_k=5, ptr=P, vt=P, v=P, ld_v=16, bf=P, indptr=P, cols=P,
             out_len=P, flag=P, ws=P, ws_bytes=1 << 40):
        return f(ptr, ptr, n_users, vt, ld, v, ld_v, bf, n_items, k, kp, top_k, indptr, cols, ptr, ptr, out_len, flag,
                 ws, ws_bytes, None)

    pre = b"als_score_topk_pruned_excluding: "
    for kwargs, msg in (
            (dict(kp=48), b"kp must be 16, 32, 64, 96, 128, 192 or 256"),
            (dict(k=17), b"need 1 <= k <= kp"),
            (dict(k=0), b"need 1 <= k <= kp"),
            (dict(n_users=65536), b"bad shape"),
            (dict(n_users=-1), b"bad shape"),
            (dict(n_items=-1, ld=0), b"bad shape"),
            (dict(ld=96), b"ld_items must be >= n_items, % 4 and < 2^29"),
            (dict(ld=102), b"ld_items must be >= n_items, % 4 and < 2^29"),
            (dict(ld=1 << 29, n_items=10), b"ld_items must be >= n_items, % 4 and < 2^29"),
            (dict(ld_v=9), b"ld_v must be >= k"),
            (dict(top_k=0), b"top_k must be in [1, 1024]"),
            (dict(top_k=1025), b"top_k must be in [1, 1024]"),
            (dict(ptr=None), b"null pointer"),
            (dict(vt=None), b"null pointer"),
            (dict(v=None), b"null pointer"),
            (dict(bf=None), b"null pointer"),
            (dict(flag=None), b"null pointer"),
            (dict(ws=None), b"null pointer"),
            (dict(indptr=None), b"null exclusion or out_len"),
            (dict(cols=None), b"null exclusion or out_len"),
            (dict(out_len=None), b"null exclusion or out_len"),
            (dict(bf=VP(384)), b"items_bf16 must be 256-B aligned"),
            (dict(bf=VP(257)), b"items_bf16 must be 256-B aligned"),
            (dict(ws_bytes=16), b"workspace 16 < "),
            (dict(ws_bytes=16, n_items=100_000, ld=100_000), b"workspace 16 < ")):
        assert call(**kwargs) == -1, kwargs
        assert pre + msg in lib.hrec_last_error(), (kwargs, lib.hrec_last_error())
    # nothing to rank: OK with null pointers
    nulls = dict(ptr=None, vt=None, v=None, bf=None, indptr=None, cols=None, out_len=None, flag=None, ws=None,
                 ws_bytes=0)
    assert call(n_users=0, **nulls) == 0
    assert call(n_items=0, ld=0, **nulls) == 0


def test_workspace_query(lib):
    q = lib.hrec_als_score_topk_pruned_excluding_workspace_bytes
    pruned, fused = lib.hrec_als_score_topk_pruned_workspace_bytes, lib.hrec_als_score_topk_excluding_workspace_bytes
    for n_items in (29, 2048, 2049, 8192, 8193, 100_000):
        for top_k in (1, 8, 9, 64, 65, 1024):
            for k in (10, 65, 256):
                prev = 0
                for n_users in (0, 1, 5, 1024, 4096, 65535):
                    need = q(n_users, n_items, top_k, k)
                    assert need >= pruned(n_users, n_items, top_k, k) > 0
                    assert need >= fused(n_users, n_items, top_k) > 0
                    assert need >= prev
                    prev = need


def test_the_pruned_entry_keeps_its_workspace_and_messages(lib):
    """The unfiltered entry shares the launch function: its texts and its need are its own."""
    f = lib.hrec_als_score_topk_pruned
    f.restype = I32
    f.argtypes = [VP, VP, I32, VP, I64, VP, I64, VP, I64, I32, I32, I32, VP, VP, VP, VP, SZ, VP]
    P = VP(256)
    assert f(P, P, 4, P, 104, P, 9, P, 100, 10, 16, 5, P, P, P, P, 1 << 40, None) == -1
    assert b"als_score_topk_pruned: ld_v must be >= k" in lib.hrec_last_error()
    assert f(P, P, 4, P, 104, P, 16, VP(384), 100, 10, 16, 5, P, P, P, P, 1 << 40, None) == -1
    assert b"als_score_topk_pruned: items_bf16 must be 256-B aligned" in lib.hrec_last_error()
    need = lib.hrec_als_score_topk_pruned_workspace_bytes(4, 100_000, 5, 10)
    assert f(P, P, 4, P, 100_000, P, 16, P, 100_000, 10, 16, 5, P, P, P, P, need - 1, None) == -1
    assert b"als_score_topk_pruned: workspace %d < %d" % (need - 1, need) in lib.hrec_last_error()
