"""MatrixTable.pool_rows on the CPU against a plain fp64 loop: the local
table, both planes under run_dist, the table variants and the refusals. The
kernel is in test_gpu_pool_rows.py."""

import functools
from unittest import mock

import pytest
import torch

import multiverso_amd as mv
from conftest import run_dist
from multiverso_amd.log import FatalError

U = 2.0 ** -24   # one fp32 rounding, relative
LENS = [0, 1, 12, 3, 0, 2]   # 12 ids over 7 rows: duplicates inside the bag


def pool_ref(table, ids, offsets, weights=None, bf16_parts=None):
    """(out, S), fp64 ``[B, C]``: out[b] adds ``w_i * x_i`` over bag b in list
    order, S[b] adds ``|w_i||x_i|``. With ``bf16_parts``, the owners' row
    ranges ``[(lo, hi)]``, every owner's partial is rounded to bf16 once
    (through fp32) before the owners are added."""
    ids, offsets = torch.as_tensor(ids), torch.as_tensor(offsets)
    x = table.double()[ids]
    p = x if weights is None else weights.double().unsqueeze(1) * x
    B = len(offsets) - 1
    out = torch.zeros(B, table.shape[1], dtype=torch.float64)
    for lo, hi in bf16_parts or [(0, table.shape[0])]:
        mine = ((ids >= lo) & (ids < hi)).tolist()
        part = torch.zeros_like(out)
        for b in range(B):
            for i in range(int(offsets[b]), int(offsets[b + 1])):
                if mine[i]:
                    part[b] += p[i]
        out += part.float().bfloat16().double() if bf16_parts else part
    bag_of = torch.repeat_interleave(torch.arange(B), offsets.diff())
    return out, torch.zeros_like(out).index_add_(0, bag_of, p.abs())


def assert_pooled(got, ref, offsets, owners=1, mean=False, exact=False):
    """``got`` against ``pool_ref``'s (out, S): equal when ``exact``, else
    within (L + owners + 1) * 2^-24 * S; a mean divides both by the bag's
    length and adds the division's one rounding."""
    want, S = ref
    L = torch.as_tensor(offsets).diff().double().unsqueeze(1)
    tol = (L + owners + 1) * U * S
    if mean:
        want, tol = want / L.clamp(min=1), tol / L.clamp(min=1)
        tol = tol + U * want.abs()
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = (got.cpu().double() - want).abs()
    assert bool((err <= (0 if exact else tol)).all()), float(err.max())


def make_case(R, C, lens, seed, ints):
    """(table, ids, offsets, weights), integer-valued or normal."""
    g = torch.Generator().manual_seed(seed)
    n = sum(lens)
    if ints:
        table = torch.randint(-4, 5, (R, C), generator=g).float()
        weights = torch.randint(-2, 3, (n,), generator=g).float()
    else:
        table, weights = torch.randn(R, C, generator=g), torch.randn(
            n, generator=g)
    offsets = torch.tensor([0] + list(lens)).cumsum(0)
    return table, torch.randint(0, R, (n,), generator=g), offsets, weights


@pytest.fixture()
def env():
    mv.init()
    yield
    mv.shutdown()


def _table(data, cls=None, **kw):
    t = (cls or mv.MatrixTable)(data.shape[0], data.shape[1], **kw)
    t.shard.copy_(data)
    return t


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [1, 3, 64])
def test_local_against_the_loop(env, C, weighted, mode):
    for ints in (True, False):
        table, ids, offs, w = make_case(7, C, LENS, 10 + C, ints)
        w = w if weighted else None
        got = _table(table).pool_rows(ids, offs, w, mode)
        assert_pooled(got, pool_ref(table, ids, offs, w), offs,
                      mean=mode == "mean", exact=ints and mode == "sum")


def test_no_bags_and_no_ids(env):
    t = _table(torch.ones(5, 3))
    none = torch.empty(0, dtype=torch.int64)
    got = t.pool_rows(none, [0], torch.empty(0), "mean")
    assert got.shape == (0, 3) and got.dtype == torch.float32
    got = t.pool_rows(none, [0, 0, 0], mode="mean")
    assert got.shape == (2, 3) and not got.any() and not got.signbit().any()


def test_table_variants_and_monitors(env):
    table, ids, offs, w = make_case(7, 3, LENS, 3, True)
    table = table * 37          # sums past 256: the bf16 rounding is visible
    want = pool_ref(table, ids, offs, w)
    for kw in (dict(add_filter="onebit"), dict(add_filter="topk:8"),
               dict(dtype=torch.float64)):
        assert_pooled(_table(table, **kw).pool_rows(ids, offs, w), want, offs,
                      exact=True)
    got = _table(table, wire_dtype=torch.bfloat16).pool_rows(ids, offs, w)
    rounded = pool_ref(table, ids, offs, w, bf16_parts=[(0, 7)])
    assert not torch.equal(rounded[0], want[0])
    assert_pooled(got, rounded, offs, exact=True)
    # the sparse table's bitmap stays as it is
    sp = mv.SparseMatrixTable(7, 3)
    sp.add(table)
    sp.get_into(torch.zeros_like(table))
    sp.add_rows([3], torch.ones(1, 3))
    bits = sp.up_to_date.clone()
    table[3] += 1
    want = pool_ref(table, ids, offs, w)
    assert_pooled(sp.pool_rows(ids, offs, w), want, offs, exact=True)
    assert torch.equal(sp.up_to_date, bits) and int(bits.sum()) == 6
    # a deferred Add is visible
    t = mv.MatrixTable(7, 3)
    t.add(table, async_op=True)
    assert t._pending or t._deferred is not None
    assert_pooled(t.pool_rows(ids, offs, w), want, offs, exact=True)
    from multiverso_amd.dashboard import Dashboard
    assert Dashboard.get("worker.pool_rows").count >= 6
    assert Dashboard.get("server.pool_rows").count >= 6


def test_refusals(env):
    t = _table(torch.ones(7, 3))
    ids = torch.tensor([0, 6, 2])
    bad_calls = [("offsets", (ids, o)) for o in
                 ([1, 3], [0, 2], [0, 2, 1, 3], [], [[0, 3]])]
    bad_calls += [("row_ids", (i, [0, 3])) for i in ([0, 7, 2], [-1, 1, 2])]
    bad_calls += [("weights", (ids, [0, 3], w)) for w in
                  (torch.ones(2), torch.ones(3, dtype=torch.int64))]
    bad_calls += [("mode", (ids, [0, 3], None, "max"))]
    for word, args in bad_calls:
        with pytest.raises(FatalError, match=word):
            t.pool_rows(*args)
    with pytest.raises(FatalError, match="float table"):
        mv.MatrixTable(7, 3, dtype=torch.int32).pool_rows(ids, [0, 3])


# ---- the two planes under run_dist --------------------------------------
def _plane_body(rank, world, sync, roles=None):
    import multiverso_amd as mv
    if sync:
        mv.init(sync=True)
    else:
        mv.init([f"-ps_role={roles[rank]}"] if roles else None)
    zoo = mv.Zoo.get()
    assert (zoo.async_engine is None) == sync
    R = 7                                           # uneven shards: 3+4, 2+2+3
    table = make_case(R, 5, LENS, 20, True)[0] * 37
    _, ids, offs, w = make_case(R, 5, LENS, 21 + rank, True)   # my own bags
    # bags that touch one, some and all owners, ahead of the random ones
    head = [0, 0, 0, R - 1] + list(range(R))
    ids = torch.cat([torch.tensor(head), ids])
    offs = torch.cat([torch.tensor([0, 2, 4]), offs + len(head)])
    w = torch.cat([torch.ones(len(head)), w])
    if rank == 1 and sync:                          # one rank with B == 0
        ids, offs, w = ids[:0], offs[:1], w[:0]
    for kw in ({}, dict(wire_dtype=torch.bfloat16)):
        t = mv.MatrixTable(R, 5, **kw)
        t.shard.copy_(table[t.row_offset:t.row_offset + t.local_rows])
        mv.barrier()
        if zoo.is_worker:
            ranges = [t.spec.range_of(s) for s in range(t.spec.n)]
            parts = [(lo, lo + cnt) for lo, cnt in ranges] if kw else None
            for wts in (None, w):
                assert_pooled(t.pool_rows(ids, offs, wts),
                              pool_ref(table, ids, offs, wts, parts), offs,
                              exact=True)
        else:   # a CHECK tears the process group down; this job goes on
            with mock.patch("torch.distributed.destroy_process_group"), \
                    pytest.raises(FatalError, match="ps_role=server"):
                t.pool_rows(ids, offs)
        mv.barrier()
    mv.shutdown()


@pytest.mark.parametrize("world,sync,roles", [
    (2, True, None), (3, True, None), (2, False, None),
    (3, False, ("default", "server", "worker"))])
def test_planes(world, sync, roles):
    run_dist(functools.partial(_plane_body, sync=sync, roles=roles), world)
