"""GPU: the shared exclusion walk, mask kernel and drop kernel
(csrc/exclusion.h, csrc/exclusion.hip) at the shapes where a walk of 64 lanes
per stride can go wrong. Every expectation is a numpy oracle written here;
nothing has a tolerance (ids, score bits, lengths and masked matrices are
compared exactly).

Already covered elsewhere and not repeated: short raw segments with
duplicates, negative and out-of-range columns and gathered row ids
(tests/test_gpu_als_exclude.py::test_raw_csr_with_duplicates_and_out_of_range_columns),
random / own-top / everything-but-three patterns on every ALS route (the same
file), and hrec_dot_topk_excluding at N = 16385 (step 2) with random and odd
patterns, negative excl_rows, refinement and fallback
(tests/test_gpu_dot_exclude.py). Added here: segment lengths on the 64-lane
stride boundaries, the distinct rule read across a stride, a walk whose
in-range part ends on a boundary, row_stride > n, n = 1, a strided mask whose
segment names multiples of the step, non-multiples and a column with
c / step >= S, and the drop kernel with and without out_len on candidate lists
whose length is no multiple of its 256-thread block.

Scores are exact in f32 by construction (operands are multiples of 1/4 with
|x| <= 3 and at most 32 terms: every product and partial sum is a multiple of
1/16 below 2^9), so the numpy scores have the device's bits in any summation
order."""
import numpy as np
import pytest
import torch
from test_gpu_dot_exclude import _assert_lists, _cap, _raw, _sample, _survivors

pytestmark = pytest.mark.gpu

FILL = np.float32(-7.5)


def _mask_oracle(vals, n, row_ids, segs, fill):
    """(masked copy, kept): row i loses the columns in [0, n) of segs[row_ids[i]]."""
    exp, kept = vals.copy(), np.zeros(len(row_ids), np.int32)
    for i, r in enumerate(row_ids):
        live = sorted({c for c in (segs[r] if r >= 0 else []) if 0 <= c < n})
        exp[i, live] = fill
        kept[i] = n - len(live)
    return exp, kept


def _csr(segs, device):
    for s in segs:
        assert list(s) == sorted(s), "a segment is ascending"
    indptr = np.cumsum([0] + [len(s) for s in segs]).astype(np.int64)
    cols = np.array([c for s in segs for c in s], np.int32)
    return torch.as_tensor(indptr, device=device), torch.as_tensor(cols, device=device)


def _run_mask(device, n, stride, segs, row_ids):
    from src import _hrec

    rng = np.random.default_rng(7 * n + len(segs))
    big = rng.standard_normal((len(row_ids), stride)).astype(np.float32)
    dev = torch.as_tensor(big, device=device)
    kept = _hrec.mask_rows(dev[:, :n], torch.as_tensor(np.asarray(row_ids, np.int64), device=device),
                           *_csr(segs, device), fill=float(FILL))
    exp, exp_kept = _mask_oracle(big, n, row_ids, segs, FILL)  # columns n .. stride - 1 stay as they were
    np.testing.assert_array_equal(kept.cpu().numpy(), exp_kept)
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), exp.view(np.uint32))


def test_mask_rows_on_the_stride_boundaries(device):
    """n = 200, row_stride = 211. Segments of 0, 1, 63, 64, 65, 128 and 129
    distinct columns; a duplicate pair on positions 63 / 64 and on 127 / 128
    (the distinct rule reads the last lane of the previous stride); leading
    negative columns, three of them and a whole stride of them; in-range parts
    of exactly 64 and 128 columns followed by columns >= n; a column >= n in
    the last lane of a stride; row ids permuted, repeated and -1."""
    n, big = 200, 1 << 30
    segs = [list(range(3, 3 + L)) for L in (0, 1, 63, 64, 65, 128, 129)]
    segs += [list(range(63)) + [100, 100] + list(range(101, 120)),            # 7: duplicates on 63 / 64
             list(range(127)) + [150, 150, 151],                              # 8: duplicates on 127 / 128
             [5] * 64 + [5, 6],                                               # 9: one column over a whole stride and on
             [-9, -9, -1] + list(range(0, 122, 2)),                           # 10: 3 negatives + 61 = one stride
             [-4] * 64 + [0, 0, 7],                                           # 11: a stride of negatives, then column 0
             list(range(100, 164)) + [n, n, n + 5, big],                      # 12: 64 in range, then >= n
             list(range(20, 148)) + [n],                                      # 13: 128 in range, then >= n
             list(range(63)) + [n] + [n + 1] * 70,                            # 14: >= n in lane 63, more strides after
             [n, big]]                                                        # 15: nothing in range
    row_ids = [15, 14, 13, 12, 11, 10, 9, 8, 7, -1, 6, 5, 4, 3, 2, 1, 0, 7, -1, 12, 4]
    _run_mask(device, n, 211, segs, row_ids)


def test_mask_rows_with_one_column(device):
    """n = 1 (row_stride 3): only column 0 can be masked or counted."""
    segs = [[], [0], [0, 0], [-1, 0, 1], [1, 2], [-2, -1], [0] * 65]
    _run_mask(device, 1, 3, segs, [0, 1, 2, 3, 4, 5, 6, -1, 1])


def _exact_vecs(n, d, seed):
    return (np.clip(np.round(4 * np.random.default_rng(seed).standard_normal((n, d))), -12, 12) / 4).astype(np.float32)


def _exact_scores(U, V):
    s = U.astype(np.float64) @ V.astype(np.float64).T
    assert np.array_equal(s, s.astype(np.float32))
    return s.astype(np.float32)


def _expected(scores, per_q, kk):
    """The filtered stable ranking: (idx, val, lens) as the library gives them."""
    B, N = scores.shape
    idx, val, lens = np.zeros((B, kk), np.int64), np.zeros((B, kk), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        gone = np.zeros(N, bool)
        gone[[c for c in per_q[b] if 0 <= c < N]] = True
        o = np.argsort(-scores[b].astype(np.float64), kind="stable")
        o = o[~gone[o]][:kk]
        idx[b, :len(o)], val[b, :len(o)], lens[b] = o, scores[b, o], len(o)
    return idx, val, lens


def _top_patterns(scores, N, step):
    """Per query, ascending column lists made of its best items: they all reach
    any bound, so only the exclusion can take them out."""
    order = np.argsort(-scores.astype(np.float64), axis=1, kind="stable")
    even = [o[o % step == 0] for o in order]
    odd = [o[o % step != 0] for o in order]
    big = 1 << 30
    return [[],                                                                   # an empty segment
            sorted(order[1, :40].tolist()),                                       # both kinds, as they come
            sorted(order[2, :63].tolist() + [N - 1]),                             # 64 columns: one whole stride
            sorted(even[3][:32].tolist() + odd[3][:32].tolist() + [N - 1]),       # 65: one lane into the next
            sorted([-3, int(order[4, 0]), int(order[4, 0]), int(odd[4][0]), N - 1, N - 1, N, big]),
            sorted(odd[5][:129].tolist())]                                        # 129 columns outside the sample


@pytest.mark.parametrize("kk", [10, 100])
def test_dot_strided_mask_and_drop_without_out_len(device, kk):
    """N = 16385 is the smallest catalogue hrec_dot_topk samples with step >=
    2 (dot_sample: N > 16384 gives S = max(8192, ceil(4 kk N / cap)) = 8192 at
    both kk, step = N / S = 2). Item 16384 is a multiple of the step with
    c / step = 8192 >= S: excluded, it must touch no sample column. One call
    of the entry, no overflow: the strided mask forms the bound and out_len,
    the drop kernel (out_len null) empties the excluded candidates, among them
    the odd items no sample column stands for. kk = 100: lists of more than
    one block of the drop kernel."""
    from src import _hrec as h

    N, B, d = 16385, 7, 32
    S, step = _sample(N, kk)
    assert (S, step) == (8192, 2) and _sample(N - 1, kk)[1] == 1 and (N - 1) // step >= S
    U, V = _exact_vecs(B, d, 11), _exact_vecs(N, d, 12)
    scores = _exact_scores(U, V)
    per_q = _top_patterns(scores, N, step) + [[]]
    surv = _survivors(scores, [np.asarray(c, np.int64) for c in per_q], kk)
    assert surv.max() <= _cap(kk) and (surv % 256 != 0).all(), "no overflow; lists end inside a block of the drop kernel"
    rows = torch.as_tensor(np.array([0, 1, 2, 3, 4, 5, -1], np.int64), device=device)  # the last query: no row at all
    Ud, Vd = (h.dot_operand(torch.as_tensor(x, device=device)) for x in (U, V))
    oi, ov, on, flag = _raw(h, Ud, Vd, kk, rows, *_csr(per_q[:6], device))
    assert flag == 0
    _assert_lists((oi, ov, on), _expected(scores, per_q, kk), "dot, step 2")


@pytest.mark.parametrize("kk", [10, 200])
def test_als_drop_with_out_len(device, kk):
    """hrec_als_score_topk_excluding at 2500 items (sample = the first 2048,
    filter, drop kernel with out_len, top-k), rank 32, the dot test's
    exclusion patterns. Before the call the oracle forms the bound
    the library forms (kk <= 64: the kk-th of the 64 lane maxima of the masked
    sample; above: its kk-th best) and counts each query's candidates: within the 4096 cap and no
    multiple of 256 (kk = 200: more than one block of the drop kernel)."""
    from src import _hrec as h

    N, B, k = 2500, 6, 32
    U, V = _exact_vecs(B, k, 21), _exact_vecs(N, k, 22)
    scores = _exact_scores(U, V)  # the JVM chain's sums are exact too
    per_q = _top_patterns(scores, N, 2)
    for b in range(B):
        s = scores[b, :2048].copy()
        s[[c for c in per_q[b] if 0 <= c < 2048]] = -np.inf
        bound = np.sort(s.reshape(32, 64).max(axis=0) if kk <= 64 else s)[::-1][kk - 1]
        count = np.count_nonzero(scores[b] >= bound)
        assert count <= 4096 and count % 256 != 0
    Ud, Vd = torch.as_tensor(U, device=device), torch.as_tensor(V, device=device)
    flag = torch.ones(1, dtype=torch.int32, device=device)
    got = h.als_score_topk_excluding(Ud, torch.arange(B, device=device), h.transpose(Vd), N, k, kk,
                                     *_csr(per_q, device), overflow_out=flag)
    assert int(flag.item()) == 0
    _assert_lists(got, _expected(scores, per_q, kk), "ALS exact")
