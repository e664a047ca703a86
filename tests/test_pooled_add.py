"""MatrixTable.add_pooled on the CPU: equal to add_rows of the expanded values
on a twin table (local and on both planes under run_dist), the table variants
and the refusals. The kernel is in test_gpu_pooled_add.py."""

import functools
from unittest import mock

import pytest
import torch

import multiverso_amd as mv
from conftest import run_dist
from multiverso_amd.log import FatalError
from multiverso_amd.updaters import AddOption

LENS = [0, 1, 12, 3, 0, 2]   # 18 ids over 7 rows: duplicates inside the bag
UPDATERS = ["default", "sgd", "momentum", "adagrad", "dcasgd", "dcasgda",
            "adam"]
OPTION = AddOption(worker_id=1, momentum=0.5, learning_rate=0.5, rho=0.25,
                   lambda_=0.125)


def pooled_ref(R, ids, offsets, g, weights=None, mode="sum"):
    """The plain reference, a loop over the ids: ``(vals, sums, S, L)`` in
    fp64. ``vals[i] = w'_i * g[bag(i)]`` are the rows add_rows would take,
    with ``w'`` in fp32 as add_pooled defines it; ``sums[r]`` adds them over
    the ids that name row r in list order, ``S[r]`` their magnitudes, and
    ``L[r]`` counts them."""
    C = g.shape[1]
    vals = torch.zeros(len(ids), C, dtype=torch.float64)
    sums, S = torch.zeros(R, C, dtype=torch.float64), torch.zeros(
        R, C, dtype=torch.float64)
    L = torch.zeros(R, 1, dtype=torch.float64)
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        for i in range(lo, hi):
            w = torch.tensor(1.0) if weights is None else weights[i].float()
            if mode == "mean":
                w = w / torch.tensor(float(hi - lo))
            vals[i] = w.double() * g[b].double()
            sums[int(ids[i])] += vals[i]
            S[int(ids[i])] += vals[i].abs()
            L[int(ids[i])] += 1
    return vals, sums, S, L


def make_case(R, C, lens, seed, ints):
    """(table, ids, offsets, bag_values, weights), integer-valued or normal;
    the weights are fp32 from the start."""
    g = torch.Generator().manual_seed(seed)
    n, B = sum(lens), len(lens)
    if ints:
        table, vals = (torch.randint(-4, 5, s, generator=g).float()
                       for s in ((R, C), (B, C)))
        weights = torch.randint(-2, 3, (n,), generator=g).float()
    else:
        table, vals, weights = (torch.randn(s, generator=g)
                                for s in ((R, C), (B, C), (n,)))
    offsets = torch.tensor([0] + list(lens)).cumsum(0)
    return table, torch.randint(0, R, (n,), generator=g), offsets, vals, weights


def state_of(t):
    """The shard and every state tensor of its updater, in a fixed order."""
    u = vars(t.updater)
    return ([t.shard] + [u[k] for k in sorted(u)
                         if torch.is_tensor(u[k]) and k != "shard"]
            + [u["_bak"][k] for k in sorted(u.get("_bak", {}))])


def assert_twins(t, twin, exact):
    for a, b in zip(state_of(t), state_of(twin), strict=True):
        assert torch.equal(a, b) if exact else torch.allclose(
            a, b, rtol=1e-6, atol=1e-6), (a - b).abs().max()


def _table(data, cls=None, **kw):
    t = (cls or mv.MatrixTable)(data.shape[0], data.shape[1], **kw)
    t.shard.copy_(data[t.row_offset:t.row_offset + t.local_rows])
    return t


def both(updater, table, ids, offs, g, w, mode, exact, steps=2, **kw):
    """``steps`` add_pooled calls on one table, add_rows of the expanded rows
    on its twin (every rank of a sync plane calls this together)."""
    t, twin = (_table(table, updater_type=updater, **kw) for _ in range(2))
    option = None if updater == "adam" else OPTION
    rows = pooled_ref(table.shape[0], ids, offs, g, w, mode)[0].float()
    for _ in range(steps):
        t.add_pooled(ids, offs, g, w, mode, option)
        twin.add_rows(ids, rows, option)
    mv.barrier()
    assert_twins(t, twin, exact)
    return t


@pytest.fixture()
def env():
    mv.init()
    yield
    mv.shutdown()


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("updater", UPDATERS)
def test_local_equals_add_rows(env, updater, weighted, mode):
    for ints in (True, False):
        table, ids, offs, g, w = make_case(12, 5, LENS, 11, ints)
        t = both(updater, table, ids, offs, g, w if weighted else None, mode,
                 exact=ints and mode == "sum")
        untouched = [r for r in range(12) if r not in ids.tolist()]
        assert untouched and torch.equal(t.shard[untouched], table[untouched])


def test_table_variants(env):
    table, ids, offs, g, w = make_case(7, 3, LENS, 3, True)
    g = g * 259                # 9 bits and more: the bf16 rounding is visible
    sums = pooled_ref(7, ids, offs, g, w)[1]
    none = torch.empty(0, dtype=torch.int64)
    for kw in (dict(add_filter="onebit"), dict(add_filter="topk:8"),
               dict(dtype=torch.float64), {}):
        t = _table(table, **kw)
        t.add_pooled(none, [0], torch.empty(0, 3))            # B == 0
        t.add_pooled(none, [0, 0], torch.ones(1, 3), mode="mean")
        assert torch.equal(t.shard.double(), table.double())
        t.add_pooled(ids, offs, g, w)
        assert torch.equal(t.shard.double(), table + sums)
    # bf16 wire: bag_values is rounded once, the sums stay fp32
    t = _table(table, wire_dtype=torch.bfloat16)
    t.add_pooled(ids, offs, g, w)
    rounded = pooled_ref(7, ids, offs, g.bfloat16().float(), w)[1]
    assert not torch.equal(rounded, sums)
    assert torch.equal(t.shard.double(), table + rounded)
    # the sparse table's bitmap behaves as after add_rows
    sp, twin = (_table(table, mv.SparseMatrixTable) for _ in range(2))
    for s in (sp, twin):
        s.get_into(torch.zeros_like(table))
        assert bool(s.up_to_date.all())
    few = (ids[:3], [0, 3], g[:1], w[:3])
    sp.add_pooled(*few)
    twin.add_rows(ids[:3], pooled_ref(7, *few)[0].float())
    assert torch.equal(sp.up_to_date, twin.up_to_date)
    assert not bool(sp.up_to_date.all()) and bool(sp.up_to_date.any())
    assert torch.equal(sp.shard, twin.shard)
    # a deferred Add lands first
    t = mv.MatrixTable(7, 3, updater_type="momentum")
    t.add(table, OPTION, async_op=True)
    assert t._pending or t._deferred is not None
    twin = mv.MatrixTable(7, 3, updater_type="momentum")
    twin.add(table, OPTION)
    t.add_pooled(ids, offs, g, w, option=OPTION)
    twin.add_rows(ids, pooled_ref(7, ids, offs, g, w)[0].float(), OPTION)
    assert_twins(t, twin, exact=True)


def test_refusals(env):
    t = _table(torch.ones(7, 3))
    ids, g = torch.tensor([0, 6, 2]), torch.ones(1, 3)
    bad_calls = [("offsets", (ids, o, g)) for o in
                 ([1, 3], [0, 2], [0, 2, 1, 3], [], [[0, 3]])]
    bad_calls += [("row_ids", (i, [0, 3], g)) for i in ([0, 7, 2], [-1, 1, 2])]
    bad_calls += [("weights", (ids, [0, 3], g, w)) for w in
                  (torch.ones(2), torch.ones(3, dtype=torch.int64))]
    bad_calls += [("mode", (ids, [0, 3], g, None, "max"))]
    bad_calls += [("bag_values", (ids, [0, 3], v)) for v in
                  (torch.ones(2, 3), torch.ones(1, 4),
                   torch.ones(1, 3, dtype=torch.int64))]
    for word, args in bad_calls:
        with pytest.raises(FatalError, match="add_pooled " + word):
            t.add_pooled(*args)
    with pytest.raises(FatalError, match="float table"):
        mv.MatrixTable(7, 3, dtype=torch.int32).add_pooled(ids, [0, 3], g)
    assert torch.equal(t.shard, torch.ones(7, 3))


# ---- the two planes under run_dist --------------------------------------
def _plane_body(rank, world, sync, roles=None):
    import multiverso_amd as mv
    if sync:
        mv.init(sync=True)
    else:
        mv.init([f"-ps_role={roles[rank]}"] if roles else None)
    zoo = mv.Zoo.get()
    R = 7                                           # uneven shards: 3+4, 2+2+3
    table = make_case(R, 5, LENS, 20, True)[0]
    _, ids, offs, g, w = make_case(R, 5, LENS, 21 + rank, True)  # my own bags
    # bags that touch one, some and all owners, ahead of the random ones
    head = [0, 0, 0, R - 1] + list(range(R))
    ids = torch.cat([torch.tensor(head), ids])
    offs = torch.cat([torch.tensor([0, 2, 4]), offs + len(head)])
    w = torch.cat([torch.ones(len(head)), w])
    g = torch.cat([torch.ones(3, 5), g])
    if rank == 1 and sync:                          # one rank with B == 0
        ids, offs, w, g = ids[:0], offs[:1], w[:0], g[:0]
    t = mv.MatrixTable(R, 5)
    if not zoo.is_worker:   # a CHECK tears the process group down: patched
        with mock.patch("torch.distributed.destroy_process_group"), \
                pytest.raises(FatalError, match="ps_role=server"):
            t.add_pooled(ids, offs, g)
    for updater in UPDATERS:
        for wts, mode, kw in ((None, "sum", {}), (w, "mean", {}), (w, "sum",
                              dict(wire_dtype=torch.bfloat16))):
            if sync:
                both(updater, table, ids, offs, g, wts, mode, mode == "sum",
                     steps=1, **kw)
                continue
            # servers apply on arrival: the workers take turns, so that the
            # twin sees the same order
            t, twin = (_table(table, updater_type=updater, **kw)
                       for _ in range(2))
            opt = None if updater == "adam" else OPTION
            for turn in zoo.worker_ranks:
                if rank == turn:
                    t.add_pooled(ids, offs, g, wts, mode, opt)
                    twin.add_rows(ids, pooled_ref(R, ids, offs, g, wts,
                                                  mode)[0].float(), opt)
                mv.barrier()
            assert_twins(t, twin, mode == "sum")
    # Adam counts no update on a shard that receives no ids
    t = mv.MatrixTable(R, 5, updater_type="adam")
    if zoo.is_worker:
        t.add_pooled([0, 1, 0], [0, 3], torch.ones(1, 5))
    mv.barrier()
    if zoo.is_server:   # one collective update, or one for every worker
        calls = 1 if sync else len(zoo.worker_ranks)
        assert t.updater.step == (calls if t.row_offset == 0 else 0)
    mv.shutdown()


@pytest.mark.parametrize("world,sync,roles", [
    (2, True, None), (3, True, None), (2, False, None),
    (3, False, ("default", "server", "worker"))])
def test_planes(world, sync, roles):
    run_dist(functools.partial(_plane_body, sync=sync, roles=roles), world)
