"""CPU, world_size 2 (gloo): the non-negative fit through DeviceALS's sharding.
Explicit: every row's NNLS solve sees the same operands as in the one-rank
fit, so the sharded fit is bit-equal to the unsharded oracle fit. Implicit:
YtY is computed once per half-sweep from the whole replicated source buffer,
whose row layout permutes its summation order, so it equals the unsharded fit
within the fit tolerance. The per-row arithmetic and the Gramian are the numpy
oracle (tests/nnls_oracle.py), injected."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import nnls_oracle as no

N_USERS, N_ITEMS, NNZ, K, REG, ALPHA, ITERS = 90, 60, 700, 8, 0.1, 40.0, 2


def _ratings():
    """Skewed degrees, duplicates kept, negative and zero ratings."""
    rng = np.random.default_rng(5)
    pu = 1 / (np.arange(N_USERS) + 1.0) ** 0.6
    u = rng.choice(N_USERS, NNZ, p=pu / pu.sum())
    i = rng.integers(0, N_ITEMS, NNZ)
    r = rng.choice(np.array([-2, -0.5, 0, 0.5, 1, 2, 3, 4, 5], np.float32), NNZ)
    return u, i, r


def _csr(transposed):
    u, i, r = _ratings()
    return no.coo_to_csr(i, u, r, N_ITEMS) if transposed else no.coo_to_csr(u, i, r, N_USERS)


def _np_sweep(indptr, indices, values, src, k, reg, dst, implicit=False, alpha=0.0, yty=None):
    assert (yty is not None) == implicit
    out = no.half_sweep(indptr.numpy(), indices.numpy(), values.numpy(), src.numpy(), k, reg, implicit, alpha,
                        None if yty is None else yty.numpy())
    dst.zero_()
    dst[: out.shape[0], :k] = torch.from_numpy(out)


CALLS = []


def _np_gramian(src, k):
    CALLS.append(tuple(src.shape))
    return torch.from_numpy(no.gramian(src.numpy()))


def _cpu_remap(x, table):
    x.copy_(table[x.long()])


def _worker(rank, world, port, U0, q, chunks, balanced, implicit):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from src.als_engine import DeviceALS, RowLayout, shard_for_layout
    from src.synthetic import DeviceCSR

    sides = []
    for transposed, n, n_cols, ch in ((False, N_USERS, N_ITEMS, chunks), (True, N_ITEMS, N_USERS, 1)):
        ip, ix, v = _csr(transposed)
        lay = RowLayout.balanced(np.diff(ip), world, ch, row_cost=4) if balanced else RowLayout.equal(n, world, ch)
        full = DeviceCSR(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(v), 0, n, n_cols)
        sides.append((shard_for_layout(full, lay, rank), lay))
    (csr, ulay), (csc, ilay) = sides
    eng = DeviceALS(N_USERS, N_ITEMS, K, REG, csr, csc, world=world, rank=rank, group=dist.group.WORLD,
                    sweep=_np_sweep, gramian=_np_gramian, chunks=chunks, item_chunks=1, user_layout=ulay,
                    item_layout=ilay, remap=_cpu_remap, implicit=implicit, alpha=ALPHA, nonnegative=True)
    eng.set_user_factors(U0)
    eng.fit(ITERS)
    q.put((rank, eng.user_factors.numpy().copy(), eng.item_factors.numpy().copy(), list(CALLS),
           (ulay.slots, ilay.slots, eng.kp)))
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("chunks,balanced", [(1, False), (2, True)])
def test_sharded_nonneg_fit_matches_unsharded_oracle(chunks, balanced, implicit):
    world = 2
    rng = np.random.default_rng(0)
    U0 = (rng.normal(size=(N_USERS, K)) / np.sqrt(K)).astype(np.float32)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, U0, q, chunks, balanced, implicit))
             for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    U, V = no.fit(_csr(False), _csr(True), U0, K, REG, ITERS, implicit, ALPHA)
    assert (U == 0).any() and (V == 0).any() and (U >= 0).all() and (V >= 0).all()
    for _, Ur, Vr, calls, (uslots, islots, kp) in res:
        if implicit:
            np.testing.assert_allclose(Vr, V, rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(Ur, U, rtol=1e-4, atol=1e-5)
            # one Gramian per half-sweep (not per chunk), of the whole replicated source buffer
            assert calls == [(uslots, kp), (islots, kp)] * ITERS
        else:
            assert np.array_equal(Vr, V) and np.array_equal(Ur, U), "explicit: bit-equal to the one-rank fit"
            assert calls == [], "explicit: no Gramian"
