"""CPU: TwoTowerModel._exclusion_csr (pure numpy) against a brute-force set
construction, over a candidate frame that is a permutation of the itemIds
(frame row != sorted position)."""
import numpy as np

from src.two_tower_model import TwoTowerModel


def _case(seed=11):
    rng = np.random.default_rng(seed)
    n_items = 97
    item_ids = rng.permutation(np.arange(1000, 1000 + 3 * n_items, 3)).astype(np.int64)  # frame order, unsorted
    assert not np.array_equal(item_ids, np.sort(item_ids))
    users = np.array([2, 5, 7, 11, 40], np.int64)  # queried, ascending; user 11 gets no pair, user 40 every item
    eu, ei = [], []
    for u in (2, 5, 7):
        picks = rng.choice(item_ids, size=30, replace=True)  # duplicates
        eu += [u] * len(picks)
        ei += picks.tolist()
    eu += [40] * n_items
    ei += item_ids.tolist()
    eu += [3, 99, -1, 6]          # users that are not queried
    ei += [int(item_ids[0])] * 4
    eu += [2, 5, 7, 40]           # items outside the frame (between, below and above the ids)
    ei += [1001, 5, 10 ** 6, -7]
    eu += eu[:20]                 # repeated pairs
    ei += ei[:20]
    order = rng.permutation(len(eu))
    return users, item_ids, np.asarray(eu, np.int64)[order], np.asarray(ei, np.int64)[order]


def test_exclusion_csr_matches_brute_force():
    users, item_ids, eu, ei = _case()
    indptr, cols = TwoTowerModel._exclusion_csr(users, item_ids, eu, ei)
    assert indptr.dtype == np.int64 and cols.dtype == np.int32
    assert indptr.shape == (len(users) + 1,) and indptr[0] == 0 and indptr[-1] == len(cols)
    assert np.all(np.diff(indptr) >= 0)
    row_of = {int(v): r for r, v in enumerate(item_ids.tolist())}
    for q, u in enumerate(users.tolist()):
        want = sorted({row_of[i] for uu, i in zip(eu.tolist(), ei.tolist()) if uu == u and i in row_of})
        got = cols[indptr[q]: indptr[q + 1]]
        assert got.tolist() == want
        assert np.all(np.diff(got) > 0)  # ascending and distinct
    assert indptr[4] - indptr[3] == 0              # user 11: no pairs
    assert indptr[5] - indptr[4] == len(item_ids)  # user 40: every item
    # a frame row differs from the sorted position somewhere in the result
    pos_sorted = np.searchsorted(np.sort(item_ids), item_ids[cols[: indptr[1]]])
    assert not np.array_equal(pos_sorted, cols[: indptr[1]])


def test_exclusion_csr_empty_inputs():
    users, item_ids, eu, ei = _case()
    z = np.zeros(0, np.int64)
    for args in ((z, item_ids, eu, ei), (users, z, eu, ei), (users, item_ids, z, z)):
        indptr, cols = TwoTowerModel._exclusion_csr(*args)
        assert indptr.tolist() == [0] * (len(args[0]) + 1) and cols.size == 0
    # only unknown users / items
    indptr, cols = TwoTowerModel._exclusion_csr(users, item_ids, np.array([3, 2]), np.array([int(item_ids[0]), 1]))
    assert indptr.tolist() == [0] * (len(users) + 1) and cols.size == 0
