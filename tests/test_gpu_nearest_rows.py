"""k_row_topk + k_topk_merge on the MI355X against the fp64 oracle
(nearest_oracle.py), through MatrixTable.nearest_rows and, for what the
table layer hides (padding, refusal), through the row_topk binding."""

import pytest
import torch

import multiverso_amd as mv
from conftest import run_dist
from multiverso_amd.tables.matrix_table import EMPTY_ID, merge_topk
from nearest_cases import (EXACT, LOOSE, RANDOM, exact_case, loose_case,
                           random_case, sweep_case)
from nearest_oracle import check, oracle_topk

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def env():
    mv.init()
    assert mv.Zoo.get().device.type == "cuda"
    yield
    mv.shutdown()


@pytest.fixture(scope="module")
def hip(env):
    from multiverso_amd import ops
    return ops.module(required=True)


def _table(data, **kw):
    t = mv.MatrixTable(data.shape[0], data.shape[1], **kw)
    assert t.shard.is_cuda
    t.shard.copy_(data)
    return t


def _ints(R, C, Q, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-3, 4, (R, C), generator=g).float(),
            torch.randint(-3, 4, (Q, C), generator=g).float())


def _same_as_oracle(got, table, queries, k):
    want_s, want_i = oracle_topk(table, queries, k, "dot")
    assert torch.equal(got[1].cpu(), want_i)
    assert torch.equal(got[0].cpu(), want_s)


# ---- against the oracle -------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("Q", range(1, 17))
def test_every_query_count(env, Q, metric):
    table, queries, k = sweep_case(Q)
    got = _table(table).nearest_rows(queries, k, metric)
    assert got[0].is_cuda and got[1].is_cuda
    assert check(got, (table, queries, k, metric)) == 0


@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("shape", RANDOM)
def test_random_cases(env, shape, metric):
    """(5000, 8) has more rows than the grid has waves; (130, 65, 17, 1)
    takes two passes."""
    table, queries, k = random_case(shape)
    got = _table(table).nearest_rows(queries, k, metric)
    assert check(got, (table, queries, k, metric)) == 0


@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("shape", LOOSE)
def test_loose_cases(env, shape, metric):
    table, queries, k = loose_case(shape)
    got = _table(table).nearest_rows(queries, k, metric)
    check(got, (table, queries, k, metric))    # either branch


@pytest.mark.parametrize("shape", EXACT)
def test_exact_cases(env, shape):
    table, queries, k = exact_case(shape)
    _same_as_oracle(_table(table).nearest_rows(queries, k, "dot"), table,
                    queries, k)


def test_no_queries(env):
    t = _table(torch.ones(9, 4))
    s, i = t.nearest_rows(torch.empty(0, 4), 3)
    assert s.shape == (0, 3) and i.shape == (0, 3)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and s.is_cuda


# ---- edges --------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 63, 64])
@pytest.mark.parametrize("cols", [1, 3, 64, 65, 200, 257])
def test_lane_tails_and_list_edges(env, cols, k):
    table, queries = _ints(150, cols, 3, 1000 + cols)
    t = _table(table)
    _same_as_oracle(t.nearest_rows(queries, k, "dot"), table, queries, k)
    g = torch.Generator().manual_seed(cols * 100 + k)
    table = torch.randn(150, cols, generator=g)
    queries = torch.randn(3, cols, generator=g)
    t.shard.copy_(table)
    for metric in ("dot", "cosine"):
        check(t.nearest_rows(queries, k, metric),
              (table, queries, k, metric))


def test_fewer_rows_than_waves_and_than_k(hip):
    """Three rows: one wave of the block's four has none, and k = 5 leaves
    two empty slots, which the merge across shards then drops."""
    shard = torch.tensor([[1., 0.], [3., 0.], [2., 0.]], device="cuda")
    q = torch.tensor([[1., 0.], [-1., 0.]], device="cuda")
    s, i = hip.row_topk(shard, q, 5, False, 100)
    assert i.cpu().tolist() == [[101, 102, 100, EMPTY_ID, EMPTY_ID],
                                [100, 102, 101, EMPTY_ID, EMPTY_ID]]
    assert s.cpu().tolist() == [[3., 2., 1., -INF, -INF],
                                [-1., -2., -3., -INF, -INF]]
    other = (torch.tensor([[2.5, 0.5, -INF]] * 2, device="cuda"),
             torch.tensor([[7, 8, EMPTY_ID]] * 2, device="cuda"))
    ms, mi = merge_topk(torch.cat([s, other[0]], 1),
                        torch.cat([i, other[1]], 1), 5)
    assert mi.cpu().tolist() == [[101, 7, 102, 100, 8],
                                 [7, 8, 100, 102, 101]]
    # no rows at all: every slot empty, nothing launched
    s, i = hip.row_topk(shard[:0], q, 2, True, 0)
    assert i.cpu().tolist() == [[EMPTY_ID] * 2] * 2
    assert s.cpu().tolist() == [[-INF] * 2] * 2


def test_cosine_zero_row_and_zero_query(env):
    table = torch.tensor([[0., 0.], [1., 1.], [-1., 0.], [0., 0.]])
    s, i = _table(table).nearest_rows(
        torch.tensor([[1., 0.], [0., 0.]]), 4, "cosine")
    assert i.cpu().tolist() == [[1, 0, 3, 2], [0, 1, 2, 3]]
    s = s.cpu()
    assert s[0, 1:3].tolist() == [0.0, 0.0] and s[1].tolist() == [0.0] * 4
    assert float(s[0, 3]) == -1.0
    assert abs(float(s[0, 0]) - 0.5 ** 0.5) <= 4 * 2.0 ** -24


def test_inf_row_ranks_first_nan_row_last(env):
    table, _ = _ints(200, 5, 1, 7)
    table[130, 2] = INF
    table[40, 1] = float("nan")
    t = _table(table)
    q = torch.tensor([[1., 1., 2., 1., 1.]])
    s, i = t.nearest_rows(q, 64, "dot")
    assert int(i[0, 0]) == 130 and float(s[0, 0]) == INF
    assert 40 not in i.cpu().tolist()[0]
    small = _table(table[36:46].clone())       # the NaN row is local row 4
    s, i = small.nearest_rows(q, 10, "dot")
    assert int(i[0, 9]) == 4 and float(s[0, 9]) == -INF
    assert bool(s[0, :9].isfinite().all())
    assert 4 not in small.nearest_rows(q, 9, "dot")[1].cpu().tolist()[0]


def test_identical_rows_lowest_ids_win(env):
    table, queries = _ints(5000, 8, 2, 9)
    queries[0] = torch.tensor([3., 3., 3., 3., 3., 3., 3., 3.])
    g = torch.Generator().manual_seed(10)
    where = torch.randperm(5000, generator=g)[:64].sort().values
    table[where] = 3.0                          # the best score, 64 times
    t = _table(table)
    s, i = t.nearest_rows(queries, 64, "dot")
    assert torch.equal(i[0].cpu(), where) and s[0].cpu().tolist() == [72.] * 64
    s, i = t.nearest_rows(queries, 10, "dot")
    assert torch.equal(i[0].cpu(), where[:10])
    _same_as_oracle((s, i), table, queries, 10)


def test_repeatable_and_query_forms(env):
    table, queries, k = random_case(RANDOM[1])
    t = _table(table)
    dev = queries.cuda()
    for metric in ("dot", "cosine"):
        s, i = t.nearest_rows(dev, k, metric)
        wide = torch.zeros(queries.shape[0], 2 * queries.shape[1],
                           device="cuda")
        wide[:, ::2] = dev
        forms = {"again": dev, "strided": wide[:, ::2], "cpu": queries,
                 "double": queries.double()}
        for name, q in forms.items():
            s2, i2 = t.nearest_rows(q, k, metric)
            assert torch.equal(i2, i), (metric, name)
            assert torch.equal(s2, s), (metric, name, (s2 - s).abs().max())


def test_lds_budget_chunks_and_refusal(env, hip):
    # 16 queries of 2000 columns exceed one pass: finer chunks
    table, queries = _ints(50, 2000, 16, 3)
    _same_as_oracle(_table(table).nearest_rows(queries, 5, "dot"), table,
                    queries, 5)
    # one query of 16385 columns exceeds the budget: the launcher refuses
    # and the table layer answers with torch ops
    table, queries = _ints(20, 16385, 1, 4)
    t = _table(table)
    assert hip.row_topk(t.shard, queries.cuda(), 3, False, 0) is None
    _same_as_oracle(t.nearest_rows(queries, 3, "dot"), table, queries, 3)


# ---- table level --------------------------------------------------------
def test_sees_fused_add_get_and_deferred_add(env):
    table, queries, k = exact_case(EXACT[0])
    t = mv.MatrixTable(*table.shape)
    t.add(table.cuda())
    got = t.get()                               # the fused Add+Get
    assert torch.equal(got.cpu(), table)
    _same_as_oracle(t.nearest_rows(queries, k, "dot"), table, queries, k)
    bump = torch.zeros_like(table)
    bump[77] = queries[0]
    t.add(bump.cuda())                          # deferred on one rank
    assert t._deferred is not None
    now = table + bump
    _same_as_oracle(t.nearest_rows(queries, k, "dot"), now, queries, k)


def _async_gpu(rank, world):
    import multiverso_amd as mv
    mv.init()
    zoo = mv.Zoo.get()
    assert zoo.device.type == "cuda" and zoo.async_engine is not None
    for shape in EXACT[:2]:
        table, queries, k = exact_case(shape)
        t = mv.MatrixTable(*table.shape)
        assert t.shard.is_cuda
        t.add(table if rank == 0 else torch.zeros_like(table))
        mv.barrier()
        nq = queries.shape[0] - rank
        s, i = t.nearest_rows(queries[:nq], k, "dot")
        assert s.is_cuda and i.is_cuda
        want_s, want_i = oracle_topk(table, queries[:nq], k, "dot")
        assert torch.equal(i.cpu(), want_i), (rank, shape)
        assert torch.equal(s.cpu(), want_s), (rank, shape)
        mv.barrier()
    mv.shutdown()


def test_async_engine_gpu_shards():
    run_dist(_async_gpu, 2, gpu_share=True)
