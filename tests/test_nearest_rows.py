"""MatrixTable.nearest_rows on the CPU: the oracle itself, merge_topk, the
local table, both planes under run_dist, the table variants, the refusals
and the serving example. The GPU kernels are in test_gpu_nearest_rows.py."""

import os

import pytest
import torch

import multiverso_amd as mv
from conftest import run_dist
from multiverso_amd.log import FatalError
from multiverso_amd.tables.matrix_table import EMPTY_ID, merge_topk
from nearest_cases import (EXACT, LOOSE, RANDOM, exact_case, loose_case,
                           random_case, sweep_case)
from nearest_oracle import check, oracle, oracle_topk, rank_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture()
def env():
    mv.init()
    yield
    mv.shutdown()


def _table(data, **kw):
    t = mv.MatrixTable(data.shape[0], data.shape[1], **kw)
    t.add(data)
    t.flush()
    return t


# ---- the oracle and the cases -------------------------------------------
def test_oracle_against_python_loop():
    table = torch.tensor([[1., 2., 2.], [0., 0., 0.], [3., 0., -4.],
                          [-1., -2., -2.], [.5, .5, .5], [2., 4., 4.]])
    queries = torch.tensor([[1., 0., 0.], [0., 0., 0.], [1., 2., 2.]])
    for metric in ("dot", "cosine"):
        S, A = oracle(table, queries, metric)
        for q in range(3):
            qv = [float(x) for x in queries[q]]
            qn = sum(x * x for x in qv) ** 0.5
            if metric == "cosine" and qn > 0:
                qv = [x / qn for x in qv]
            for r in range(6):
                rv = [float(x) for x in table[r]]
                s = sum(a * b for a, b in zip(rv, qv))
                a = sum(abs(a * b) for a, b in zip(rv, qv))
                if metric == "cosine":
                    rn = sum(x * x for x in rv) ** 0.5
                    s, a = (s / rn, a / rn) if rn > 0 else (0.0, 0.0)
                assert abs(float(S[q, r]) - s) < 1e-12
                assert abs(float(A[q, r]) - a) < 1e-12
    # the zero-norm row scores exactly 0 under cosine; ties rank by id
    S, _ = oracle(table, queries, "cosine")
    assert float(S[0, 1]) == 0.0 and float(S[2, 1]) == 0.0
    assert rank_rows(S)[2].tolist()[:2] == [0, 5]   # both cosine 1.0


def test_cases_have_their_gap():
    """A bad seed fails here, on the oracle alone."""
    for shape in RANDOM:
        random_case(shape)
    for Q in range(1, 17):
        sweep_case(Q)


# ---- merge_topk ---------------------------------------------------------
def test_merge_topk_ties_nan_and_empty_slots():
    nan = float("nan")
    s = torch.tensor([[1., 3., 3., nan, -INF, 3., -INF],
                      [-INF, -INF, 2., 2., -INF, nan, 0.]])
    i = torch.tensor([[9, 7, 2, 1, EMPTY_ID, 5, 4],
                      [EMPTY_ID, 8, 6, 3, EMPTY_ID, 0, 11]])
    ms, mi = merge_topk(s, i, 6)
    assert mi.tolist() == [[2, 5, 7, 9, 1, 4], [3, 6, 11, 0, 8, EMPTY_ID]]
    assert ms.tolist() == [[3., 3., 3., 1., -INF, -INF],
                           [2., 2., 0., -INF, -INF, -INF]]
    # fewer candidates than k: the tail is empty slots
    ms, mi = merge_topk(s[:, :2], i[:, :2], 3)
    assert mi.tolist() == [[7, 9, EMPTY_ID], [8, EMPTY_ID, EMPTY_ID]]
    assert ms[0].tolist() == [3., 1., -INF]
    # no queries
    ms, mi = merge_topk(torch.empty(0, 0), torch.empty(0, 0,
                                                       dtype=torch.int64), 4)
    assert ms.shape == (0, 4) and mi.shape == (0, 4)
    assert ms.dtype == torch.float32 and mi.dtype == torch.int64


# ---- local table --------------------------------------------------------
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("shape", RANDOM)
def test_local_random(env, shape, metric):
    table, queries, k = random_case(shape)
    t = _table(table)
    got = t.nearest_rows(queries, k, metric)
    assert check(got, (table, queries, k, metric)) == 0


@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("shape", LOOSE)
def test_local_loose(env, shape, metric):
    table, queries, k = loose_case(shape)
    got = _table(table).nearest_rows(queries, k, metric)
    check(got, (table, queries, k, metric))   # either branch


@pytest.mark.parametrize("shape", EXACT)
def test_local_exact(env, shape):
    table, queries, k = exact_case(shape)
    s, i = _table(table).nearest_rows(queries, k, "dot")
    want_s, want_i = oracle_topk(table, queries, k, "dot")
    assert torch.equal(i, want_i) and torch.equal(s, want_s)
    assert check((s, i), (table, queries, k, "dot")) >= 0


def test_query_forms(env):
    table, queries, k = exact_case(EXACT[0])
    t = _table(table)
    s, i = t.nearest_rows(queries, k, "dot")
    one_s, one_i = t.nearest_rows(queries[2], k, "dot")        # [num_col]
    assert one_s.shape == (1, k) and torch.equal(one_i[0], i[2])
    wide = torch.zeros(queries.shape[0], 2 * queries.shape[1])
    wide[:, ::2] = queries
    for q in (queries.double(), queries.half(), wide[:, ::2]):
        s2, i2 = t.nearest_rows(q, k, "dot")
        assert torch.equal(s2, s) and torch.equal(i2, i)
    s0, i0 = t.nearest_rows(torch.empty(0, table.shape[1]), 3)
    assert s0.shape == (0, 3) and i0.shape == (0, 3)
    assert s0.dtype == torch.float32 and i0.dtype == torch.int64


def test_cosine_zero_row_and_zero_query(env):
    table = torch.tensor([[0., 0.], [1., 1.], [-1., 0.], [0., 0.]])
    t = _table(table)
    s, i = t.nearest_rows(torch.tensor([[1., 0.], [0., 0.]]), 4, "cosine")
    assert i.tolist() == [[1, 0, 3, 2], [0, 1, 2, 3]]
    assert s[0, 1:3].tolist() == [0.0, 0.0] and s[1].tolist() == [0.0] * 4
    assert float(s[0, 3]) == -1.0


def test_refusals(env):
    t = _table(torch.ones(70, 4))
    q = torch.ones(2, 4)
    for bad_k in (0, 65, -1):
        with pytest.raises(FatalError):
            t.nearest_rows(q, bad_k)
    small = _table(torch.ones(5, 4))
    with pytest.raises(FatalError):
        small.nearest_rows(q, 6)                  # k > num_row
    assert small.nearest_rows(q, 5)[1].tolist() == [[0, 1, 2, 3, 4]] * 2
    with pytest.raises(FatalError):
        t.nearest_rows(torch.ones(2, 5), 3)       # wrong width
    with pytest.raises(FatalError):
        t.nearest_rows(q, 3, metric="l2")
    ti = mv.MatrixTable(8, 4, dtype=torch.int32)
    with pytest.raises(FatalError):
        ti.nearest_rows(q, 3)
    td = mv.MatrixTable(8, 4, dtype=torch.float64)
    with pytest.raises(FatalError):
        td.nearest_rows(q, 3)


def test_table_variants_and_monitors(env):
    table, queries, k = exact_case(EXACT[0])
    want_s, want_i = oracle_topk(table, queries, k, "dot")
    # small integers survive the bf16 wire of the loading Add
    for kw in (dict(wire_dtype=torch.bfloat16), dict(updater_type="adam")):
        t = mv.MatrixTable(*table.shape, **kw)
        t.shard.copy_(table)
        s, i = t.nearest_rows(queries, k, "dot")
        assert torch.equal(i, want_i) and torch.equal(s, want_s)
    t = mv.MatrixTable(*table.shape, add_filter="onebit")
    t.shard.copy_(table)
    before = t.shard.clone()
    s, i = t.nearest_rows(queries, k, "dot")
    assert torch.equal(i, want_i) and torch.equal(s, want_s)
    assert torch.equal(t.shard, before) and t.residual is None
    from multiverso_amd.dashboard import Dashboard
    assert Dashboard.get("worker.nearest_rows").count >= 3
    assert Dashboard.get("server.nearest_rows").count >= 3


def test_sparse_table_bitmap_untouched(env):
    table, queries, k = exact_case(EXACT[1])
    sp = mv.SparseMatrixTable(*table.shape)
    sp.add(table)
    cache = torch.zeros_like(table)
    sp.get_into(cache)
    sp.add_rows([3, 50], torch.ones(2, table.shape[1]))
    bits = sp.up_to_date.clone()
    assert int(bits.sum()) == table.shape[0] - 2
    s, i = sp.nearest_rows(queries, k, "dot")
    now = table.clone()
    now[3] += 1
    now[50] += 1
    want_s, want_i = oracle_topk(now, queries, k, "dot")
    assert torch.equal(i, want_i) and torch.equal(s, want_s)
    assert torch.equal(sp.up_to_date, bits)
    assert sp.get_into(cache) == 2    # still exactly the two stale rows


def test_deferred_add_is_visible(env):
    """An Add that has not been applied yet (async handle pending, or the
    single-rank deferral on a GPU shard) lands before the search."""
    t = mv.MatrixTable(6, 2)
    delta = torch.zeros(6, 2)
    delta[4] = torch.tensor([5., 0.])
    t.add(delta, async_op=True)
    assert t._pending or t._deferred is not None
    assert float(t.shard.abs().sum()) == 0.0      # not applied yet
    s, i = t.nearest_rows(torch.tensor([1., 0.]), 1, "dot")
    assert i.tolist() == [[4]] and s.tolist() == [[5.0]]
    assert t._deferred is None and not t._pending


# ---- the two planes under run_dist --------------------------------------
def _load(t, table, rank):
    """Rank 0 carries the content; the default updater adds."""
    import multiverso_amd as mv
    if mv.Zoo.get().is_worker:
        t.add(table if rank == 0 else torch.zeros_like(table))
    mv.barrier()


def _plane_body(rank, world, sync, roles=None):
    import multiverso_amd as mv
    args = [f"-ps_role={roles[rank]}"] if roles else None
    if sync:
        mv.init(sync=True)
    else:
        mv.init(args)
    zoo = mv.Zoo.get()
    assert (zoo.async_engine is None) == sync
    for shape in EXACT:
        table, queries, k = exact_case(shape)
        t = mv.MatrixTable(*table.shape)
        _load(t, table, rank)
        if zoo.is_server:
            assert t.local_rows in t.spec.counts
            if shape == EXACT[1]:
                assert t.local_rows < k          # padding reaches the merge
        if zoo.is_worker:
            # a different Q on every rank, 0 on rank 1
            nq = {0: queries.shape[0], 1: 0}.get(rank, 2)
            s, i = t.nearest_rows(queries[:nq], k, "dot")
            want_s, want_i = oracle_topk(table, queries[:nq], k, "dot")
            assert s.shape == (nq, k) and i.shape == (nq, k)
            assert torch.equal(i, want_i), (rank, shape)
            assert torch.equal(s, want_s), (rank, shape)
        mv.barrier()
    table, queries, k = random_case(RANDOM[1])
    t = mv.MatrixTable(*table.shape)
    _load(t, table, rank)
    if zoo.is_worker:
        for metric in ("dot", "cosine"):
            got = t.nearest_rows(queries, k, metric)
            assert check(got, (table, queries, k, metric)) == 0
    mv.barrier()
    mv.shutdown()


def _sync_plane(rank, world):
    _plane_body(rank, world, True)


def _async_plane(rank, world):
    _plane_body(rank, world, False)


def _async_plane_roles(rank, world):
    _plane_body(rank, world, False, ["default", "server", "worker"])


@pytest.mark.parametrize("world", [2, 3])
def test_sync_plane(world):
    run_dist(_sync_plane, world)


def test_async_plane():
    run_dist(_async_plane, 2)


def test_async_plane_with_roles():
    run_dist(_async_plane_roles, 3)


# ---- the serving example ------------------------------------------------
def test_embedding_server_never_gathers_the_table(env, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "serve_embeddings", os.path.join(ROOT, "examples",
                                         "serve_embeddings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    words = ["king", "queen", "apple", "pear"]
    vecs = torch.tensor([[1.0, 0.0, 0.0], [0.9, 0.1, 0.0],
                         [0.0, 1.0, 0.0], [0.0, 0.9, 0.1]])
    table = _table(vecs)

    def no_get(*a, **kw):
        raise AssertionError("/nn must not gather the whole table")
    table.get = no_get
    from fastapi.testclient import TestClient
    client = TestClient(mod.build_app(table, words, 3))
    nn = client.get("/nn/king?k=1").json()
    assert nn["neighbors"][0]["word"] == "queen"
    nn = client.get("/nn/apple?k=3").json()
    assert [n["word"] for n in nn["neighbors"]] == ["pear", "queen", "king"]
