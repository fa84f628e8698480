"""CPU: the shared host exclusion builder (src/ranked_lists.py
exclusion_csr_host, pure numpy) against brute-force set constructions, in both
call shapes: the two-tower model's (queried users x a candidate frame that is
a permutation of its itemIds: frame row != sorted position) and the ALS
model's (sorted known ids, side "user" and, with the arguments swapped, side
"item")."""
import numpy as np
import pytest

from src.ranked_lists import exclusion_csr_host


def _brute(row_keys, col_keys, excl_rows, excl_cols):
    """The exclusion CSR by sets: per row key the sorted distinct positions in
    col_keys of the ids paired with it."""
    row_of = {int(r): q for q, r in enumerate(np.asarray(row_keys).tolist())}
    col_of = {int(c): p for p, c in enumerate(np.asarray(col_keys).tolist())}
    sets = [set() for _ in row_of]
    for r, c in zip(np.asarray(excl_rows).tolist(), np.asarray(excl_cols).tolist()):
        if r in row_of and c in col_of:
            sets[row_of[r]].add(col_of[c])
    indptr = np.cumsum([0] + [len(s) for s in sets]).astype(np.int64)
    return indptr, np.array([c for s in sets for c in sorted(s)], np.int32)


# ------------------------------------------------- the two-tower call shape
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
    indptr, cols = exclusion_csr_host(users, item_ids, eu, ei)
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
        indptr, cols = exclusion_csr_host(*args)
        assert indptr.tolist() == [0] * (len(args[0]) + 1) and cols.size == 0
    # only unknown users / items
    indptr, cols = exclusion_csr_host(users, item_ids, np.array([3, 2]), np.array([int(item_ids[0]), 1]))
    assert indptr.tolist() == [0] * (len(users) + 1) and cols.size == 0


# --------------------------------------------------------- the ALS call shape
def _als_pairs():
    known_users = -50 + 3 * np.arange(37, dtype=np.int64)
    known_items = -40 + 7 * np.arange(29, dtype=np.int64)
    rng = np.random.default_rng(11)
    users = np.r_[rng.choice(known_users, 400), [-49, 10 ** 6, int(known_users[3])]]  # two unknown users
    items = np.r_[rng.choice(known_items, 400), [int(known_items[0]), -39, 5]]         # two unknown items
    again = rng.integers(0, len(users), 60)                                             # duplicates
    users, items = np.r_[users, users[again]], np.r_[items, items[again]]
    perm = rng.permutation(len(users))                                                  # unsorted
    return known_users, known_items, users[perm], items[perm]


def _als_args(side, known_users, known_items, users, items):
    """DeviceALSFactors.exclusion's call: side "item" is side "user" with the arguments swapped."""
    return (known_users, known_items, users, items) if side == "user" else (known_items, known_users, items, users)


@pytest.mark.parametrize("side", ["user", "item"])
def test_host_exclusion_builder(side):
    known_users, known_items, users, items = _als_pairs()
    args = _als_args(side, known_users, known_items, users, items)
    e_indptr, e_cols = _brute(*args)
    for cols_sorted in (True, False):  # the sorted-columns shortcut the ALS model takes, and the general route
        indptr, cols = exclusion_csr_host(*args, cols_sorted=cols_sorted)
        assert indptr.dtype == np.int64 and cols.dtype == np.int32
        assert np.array_equal(indptr, e_indptr) and np.array_equal(cols, e_cols)
        assert 0 < len(cols) < 400  # duplicates went, something stayed
        for r in range(len(indptr) - 1):
            assert np.all(np.diff(cols[indptr[r]: indptr[r + 1]]) > 0)  # ascending and distinct
    # nothing known, and nothing at all: an empty CSR over every row
    for u, i in ((np.array([10 ** 6]), np.array([5])), (np.zeros(0, np.int64), np.zeros(0, np.int64))):
        indptr, cols = exclusion_csr_host(*_als_args(side, known_users, known_items, u, i), cols_sorted=True)
        assert indptr.dtype == np.int64 and cols.dtype == np.int32
        assert len(indptr) == (37 if side == "user" else 29) + 1 and not indptr.any() and len(cols) == 0
    with pytest.raises(ValueError, match="user_ids and item_ids must have the same length"):
        exclusion_csr_host(*_als_args(side, known_users, known_items, users, items[:-1]), cols_sorted=True,
                           what="user_ids and item_ids")
    with pytest.raises(ValueError, match="exclude: userId and itemId must have the same length"):
        exclusion_csr_host(*_als_args(side, known_users, known_items, users[:-1], items),
                           what="exclude: userId and itemId")


@pytest.mark.parametrize("side", ["user", "item"])
def test_unsorted_col_keys_from_the_als_call_shape(side):
    """Column keys in any order: the columns are positions in col_keys as given."""
    known_users, known_items, users, items = _als_pairs()
    row_keys, col_keys, er, ec = _als_args(side, known_users, known_items, users, items)
    col_keys = np.random.default_rng(5).permutation(col_keys)
    assert not np.array_equal(col_keys, np.sort(col_keys))
    indptr, cols = exclusion_csr_host(row_keys, col_keys, er, ec)
    e_indptr, e_cols = _brute(row_keys, col_keys, er, ec)
    assert indptr.dtype == np.int64 and cols.dtype == np.int32
    assert np.array_equal(indptr, e_indptr) and np.array_equal(cols, e_cols) and len(cols) > 0
    # the same sets as over the sorted keys, under the permutation
    s_indptr, s_cols = exclusion_csr_host(row_keys, np.sort(col_keys), er, ec, cols_sorted=True)
    assert np.array_equal(indptr, s_indptr)
    assert not np.array_equal(cols, s_cols)
    for r in range(len(indptr) - 1):
        sl = slice(indptr[r], indptr[r + 1])
        assert sorted(col_keys[cols[sl]].tolist()) == np.sort(col_keys)[s_cols[sl]].tolist()


def test_random_cases_match_brute_force():
    """200 random cases, empty sides, unknown ids and duplicates among them, in
    both ALS call shapes and with sorted and permuted column keys."""
    rng = np.random.default_rng(2024)
    seen_empty = seen_pairs = 0
    for case in range(200):
        n_u, n_i = (int(rng.integers(0, 4)) if case % 5 == 0 else int(rng.integers(1, 40)) for _ in range(2))
        known_users = np.sort(rng.choice(np.arange(-25, 25), n_u, replace=False)).astype(np.int64)
        known_items = np.sort(rng.choice(np.arange(-40, 40), n_i, replace=False)).astype(np.int64)
        n_pairs = 0 if case % 7 == 0 else int(rng.integers(1, 300))
        users = rng.integers(-30, 30, n_pairs)    # some unknown, many repeated
        items = rng.integers(-45, 45, n_pairs)
        for side in ("user", "item"):
            row_keys, col_keys, er, ec = _als_args(side, known_users, known_items, users, items)
            want = _brute(row_keys, col_keys, er, ec)
            for cols_sorted in (True, False):
                got = exclusion_csr_host(row_keys, col_keys, er, ec, cols_sorted=cols_sorted)
                assert got[0].dtype == np.int64 and got[1].dtype == np.int32
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (case, side)
            shuffled = rng.permutation(col_keys)
            got = exclusion_csr_host(row_keys, shuffled, er, ec)
            want = _brute(row_keys, shuffled, er, ec)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (case, side)
            seen_empty += len(want[1]) == 0
            seen_pairs += len(want[1]) > 0
    assert seen_empty > 20 and seen_pairs > 100  # both kinds of case were drawn
