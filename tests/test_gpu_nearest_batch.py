"""k_row_topk_mm (the MFMA scan nearest_rows takes from 17 queries) on the
MI355X against the fp64 oracle of nearest_oracle.py, through the row_topk_mm
binding and, for the dispatch, through MatrixTable.nearest_rows."""

import pytest
import torch

import multiverso_amd as mv
from multiverso_amd.tables.matrix_table import EMPTY_ID
from nearest_oracle import check, margin, oracle_topk

pytestmark = pytest.mark.gpu
INF, METRICS = float("inf"), ["dot", "cosine"]
# (R, cols, Q, k): tile, wave, panel and query-block edges, see the issue
GAP = [(1, 1, 17, 1), (31, 3, 17, 5), (129, 2, 32, 1), (33, 65, 33, 5),
       (700, 33, 40, 10), (130, 200, 64, 10), (5000, 8, 100, 64)]
NO_GAP = (300, 257, 65, 64)     # no seed gives it a gap: either branch of check


@pytest.fixture(scope="module")
def hip():
    mv.init()
    assert mv.Zoo.get().device.type == "cuda"
    from multiverso_amd import ops
    yield ops.module(required=True)
    mv.shutdown()


def _randn(shape):
    g = torch.Generator().manual_seed(200)
    return (torch.randn(shape[:2], generator=g),
            torch.randn(shape[2], shape[1], generator=g), shape[3])


def _ints(R, C, Q, seed):            # [-3, 3], rows from R//12 distinct ones
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(-3, 4, (max(R // 12, 2), C), generator=g)
    table = pool[torch.randint(0, pool.shape[0], (R,), generator=g)].float()
    return table, torch.randint(-3, 4, (Q, C), generator=g).float()


def _scan(hip, table, queries, k, metric, row_offset=0, fn="row_topk_mm"):
    q = queries.cuda()                # what a server is handed: normalised
    if metric == "cosine":
        n = torch.linalg.vector_norm(q, dim=1, keepdim=True)
        q = torch.where(n > 0, q / n, q)
    return getattr(hip, fn)(table.cuda(), q, k, metric == "cosine",
                            row_offset)


def _table(data):
    t = mv.MatrixTable(*data.shape)
    t.shard.copy_(data)
    return t


def _same(a, b):
    return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", GAP + [NO_GAP])
def test_against_oracle(hip, shape, metric):
    table, queries, k = _randn(shape)
    if shape != NO_GAP:
        assert margin(table, queries, k, metric) > 1.0
    weaker = check(_scan(hip, table, queries, k, metric),
                   (table, queries, k, metric))
    assert weaker == 0 or shape == NO_GAP


@pytest.mark.parametrize("shape", [(500, 24, 40, 64), (100, 7, 33, 64)])
def test_integer_data_and_ties(hip, shape):
    R, C, Q, k = shape
    table, queries = _ints(R, C, Q, 31 + R)
    assert _same(_scan(hip, table, queries, k, "dot"),
                 oracle_topk(table, queries, k, "dot"))


def test_planted_ties_lowest_ids_win(hip):
    g = torch.Generator().manual_seed(9)
    table = torch.randint(-3, 4, (5000, 8), generator=g).float()
    queries = torch.randint(-3, 4, (20, 8), generator=g).float()
    queries[0] = 3.0
    where = torch.randperm(5000, generator=g)[:64].sort().values
    table[where] = 3.0                          # the best score, 64 times
    s, i = _scan(hip, table, queries, 64, "dot")
    assert torch.equal(i[0].cpu(), where) and s[0].cpu().tolist() == [72.] * 64
    assert _same((s, i), oracle_topk(table, queries, 64, "dot"))


def test_special_values(hip):
    g = torch.Generator().manual_seed(7)
    table = torch.randint(1, 4, (10, 5), generator=g).float()
    queries = torch.randint(1, 4, (17, 5), generator=g).float()
    table[2] = 0.0
    queries[5] = 0.0
    s, i = (x.cpu() for x in _scan(hip, table, queries, 10, "cosine"))
    check((s, i), (table, queries, 10, "cosine"))
    assert s[:, 9].tolist() == [0.0] * 17       # every other score is > 0
    assert i[:, 9].tolist() == [2] * 5 + [9] + [2] * 11
    assert s[5].tolist() == [0.0] * 10 and i[5].tolist() == list(range(10))
    table[2] = 1.0
    table[6, 3] = INF
    table[4, 1] = float("nan")
    clean = table.clone()
    clean[6] = clean[4] = 0.0                   # what the other rows must see
    for k in (10, 9):
        s, i = (x.cpu() for x in _scan(hip, table, queries[:5].repeat(4, 1),
                                       k, "dot"))
        assert bool((i[:, 0] == 6).all()) and bool((s[:, 0] == INF).all())
        if k == 10:
            assert bool((i[:, 9] == 4).all()) and bool((s[:, 9] == -INF).all())
        want_s, want_i = oracle_topk(clean, queries[:5].repeat(4, 1), 10, "dot")
        keep = (want_i != 6) & (want_i != 4)    # the 8 finite rows, in order
        assert torch.equal(i[:, 1:9], want_i[keep].view(20, 8))
        assert torch.equal(s[:, 1:9], want_s[keep].view(20, 8))


def test_padding_and_refusal(hip):
    shard = torch.tensor([[1., 0.], [3., 0.], [2., 0.]])
    q = torch.tensor([[1., 0.], [-1., 0.]]).repeat(9, 1)
    s, i = _scan(hip, shard, q, 5, "dot", row_offset=100)
    assert i.cpu().tolist() == [[101, 102, 100, EMPTY_ID, EMPTY_ID],
                                [100, 102, 101, EMPTY_ID, EMPTY_ID]] * 9
    assert s.cpu().tolist() == [[3., 2., 1., -INF, -INF],
                                [-1., -2., -3., -INF, -INF]] * 9
    s, i = _scan(hip, shard[:0], q, 2, "cosine")
    assert i.cpu().tolist() == [[EMPTY_ID] * 2] * 18
    assert s.cpu().tolist() == [[-INF] * 2] * 18
    # 2049 columns: the plan refuses, the table layer takes k_row_topk
    table, queries = _ints(20, 2049, 17, 4)
    assert _scan(hip, table, queries, 3, "dot") is None
    assert _same(_table(table).nearest_rows(queries, 3, "dot"),
                 oracle_topk(table, queries, 3, "dot"))


@pytest.mark.parametrize("metric", METRICS)
def test_dispatch_by_query_count(hip, metric):
    table, queries, k = _randn((700, 33, 40, 10))
    t = _table(table)
    got = t.nearest_rows(queries, k, metric)
    assert _same(got, _scan(hip, table, queries, k, metric))
    assert _same(got, t.nearest_rows(queries, k, metric))
    assert check(got, (table, queries, k, metric)) == 0
    assert _same(t.nearest_rows(queries[:16], k, metric),
                 _scan(hip, table, queries[:16], k, metric, fn="row_topk"))


def test_sees_deferred_add(hip):
    table, queries = _ints(500, 24, 40, 531)
    t = mv.MatrixTable(*table.shape)
    t.add(table.cuda())
    t.get()
    bump = torch.zeros_like(table)
    bump[77] = queries[0]
    t.add(bump.cuda())                          # deferred on one rank
    assert t._deferred is not None
    assert _same(t.nearest_rows(queries, 64, "dot"),
                 oracle_topk(table + bump, queries, 64, "dot"))
