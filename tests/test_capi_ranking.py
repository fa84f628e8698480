"""CPU: the ranking-metrics entries (hrec_ranking_metrics and its workspace
query) are exported, bound, and check their arguments before any device
work."""
import ctypes

_i64, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
P = ctypes.c_void_p(256)  # a non-null stand-in: rejected calls never dereference it


def _lib():
    import __graft_entry__ as g
    import torch  # noqa: F401  (binds libamdhip64 first, as the product does)

    lib = ctypes.CDLL(g.build_lib())
    lib.hrec_last_error.restype = ctypes.c_char_p
    lib.hrec_abi_version.restype = _int
    lib.hrec_ranking_metrics_workspace_bytes.restype = _sz
    lib.hrec_ranking_metrics_workspace_bytes.argtypes = [_i64]
    lib.hrec_ranking_metrics.restype = _int
    lib.hrec_ranking_metrics.argtypes = [_vp, _i64, _int, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _sz, _vp]
    return lib


def _call(lib, pred=P, pred_ld=16, len_max=10, pred_len=None, indptr=P, labels=P, n_rows=3, k=10, gain=P, idcg=P,
          per_row=None, sums=P, unsorted=P, ws=P, ws_bytes=1 << 20):
    return lib.hrec_ranking_metrics(pred, pred_ld, len_max, pred_len, indptr, labels, n_rows, k, gain, idcg, per_row,
                                    sums, unsorted, ws, ws_bytes, None)


def test_symbols_are_exported_bound_and_abi_is_still_7():
    lib = _lib()
    from src import _hrec

    for name in ("hrec_ranking_metrics_workspace_bytes", "hrec_ranking_metrics"):
        assert hasattr(lib, name)
        assert name in _hrec._SIGNATURES
    assert lib.hrec_abi_version() == 7 and _hrec.ABI_VERSION == 7
    assert callable(_hrec.ranking_metrics)
    assert len(_hrec.RANK_SUMS) == 8  # HREC_RANK_SUMS
    assert [len(a) for a in _hrec.rank_tables(7)] == [7, 8]


def test_ranking_metrics_rejects_bad_arguments():
    lib = _lib()

    def rejected(msg, **kw):
        assert _call(lib, **kw) == -1, kw
        err = lib.hrec_last_error()
        assert err.startswith(b"ranking_metrics:") and msg in err, (kw, err)

    rejected(b"negative n_rows", n_rows=-1)
    for k in (0, -3, 1025):
        rejected(b"k must be in [1, 1024]", k=k)
    for len_max in (-1, 1025):
        rejected(b"pred_len_max must be in [0, 1024]", len_max=len_max, pred_ld=4096)
    rejected(b"pred_ld must be >= pred_len_max", pred_ld=9, len_max=10)
    for name in ("pred", "indptr", "labels", "gain", "idcg"):
        rejected(b"null pointer", **{name: None})
    for name in ("sums", "unsorted", "ws"):
        rejected(b"null sums, unsorted flag or workspace", **{name: None})
    need = lib.hrec_ranking_metrics_workspace_bytes(70000)
    rejected(b"workspace", n_rows=70000, ws_bytes=need - 1)
    assert str(need).encode() in lib.hrec_last_error()
    # the shape is checked before the row count decides that there is nothing to do
    rejected(b"k must be in [1, 1024]", n_rows=0, k=0)


def test_workspace_query():
    """One partial of 8 doubles per block of four rows; the block count grows
    with n_rows up to the grid cap and never overflows."""
    lib = _lib()
    f = lib.hrec_ranking_metrics_workspace_bytes
    sizes = [f(n) for n in (-5, 0, 1, 4, 5, 70000, 10 ** 6, 2 ** 62)]
    assert all(s >= 64 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes[5] >= min((70000 + 3) // 4, 2048) * 64  # many blocks take part at 70 000 rows
    assert sizes[5] > sizes[4] >= sizes[3]
    assert sizes[-1] == sizes[-2] <= 1 << 20  # capped grid
