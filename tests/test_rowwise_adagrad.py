"""The "rowwise_adagrad" updater, CPU tier, against the rule in fp64.

One step: B = (C/2 + 10) u |step| + u |w|, u = 2^-24 (the sum of C squares
carries at most C + 1 roundings, the root halves them, every other operation
adds one); G: (C + 3) u G. After k steps: k ((C/2 + 10) u sum|step_i| + u |w_k|),
since the error of w_1 enters w_2 = w_1 - step_2 with gain 1: "2 B of the second
step" cannot hold what step 1's rounding left on a weight that it cancelled to
near zero (derivation and the measured 14.9 x: profiles/rowwise_adagrad.md)."""

import functools

import pytest
import torch

import multiverso_amd as mv
from multiverso_amd.updaters import RowwiseAdaGradUpdater

from conftest import run_dist

U, LR, RHO = 2.0 ** -24, 0.5, 0.25
EPS = float(torch.tensor(RowwiseAdaGradUpdater.EPS, dtype=torch.float32))
IDS = [5, 8, 5, 0, 7, 5, 7]
KW = dict(updater_type="rowwise_adagrad")
OPT = mv.AddOption(learning_rate=LR, rho=RHO)


@pytest.fixture()
def env():
    mv.init()
    yield
    mv.shutdown()


def rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def ints(shape, seed):   # small integers: fp32 sums are exact in any order
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).float()


def ref_step(w, G, delta, rows=slice(None)):
    """The rule in fp64, in place on w [R, C] and G [R], for the rows listed
    (all by default) of the dense delta; returns |step|."""
    g = delta[rows].double() / LR
    G[rows] += (g * g).sum(1) / w.size(1)
    step = torch.zeros_like(w)
    step[rows] = (RHO / (G[rows] + EPS).sqrt()).unsqueeze(1) * g
    w -= step
    return step.abs()


def within(got, G_got, w, G, step, k=1):
    """got, G_got against the fp64 w, G after k steps of summed |step|."""
    C = w.size(1)
    err = (got.cpu().double().view_as(w) - w).abs()
    tol = (C / 2 + 10) * U * step + U * w.abs()
    err_G, tol_G = (G_got.cpu().double() - G).abs(), (C + 3) * U * G
    print("err / bound: w", float((err / tol).max()),
          "G", float((err_G / tol_G.clamp_min(1e-300)).max()))
    return bool((err <= k * tol).all() and (err_G <= k * tol_G).all())


def dense(R, ids, vals):
    d = torch.zeros(R, vals.size(1), dtype=torch.float64)
    return d.index_add_(0, torch.as_tensor(ids), vals.double())


def start(t, seed):
    w0 = rand((t.num_row, t.num_col), seed)
    t.shard.copy_(w0[t.row_offset:t.row_offset + t.local_rows])
    return w0.double(), torch.zeros(t.num_row, dtype=torch.float64)


@pytest.mark.parametrize("table", [mv.MatrixTable, mv.SparseMatrixTable])
@pytest.mark.parametrize("shape,wire", [((9, 5), None), ((4, 1), None),
                                        ((3, 8), torch.bfloat16)])
def test_whole_table(env, table, shape, wire):
    t = (table(*shape, **KW) if wire is None else
         mv.MatrixTable(*shape, wire_dtype=wire, **KW))
    state = t.updater.g_sqr_row
    assert state.shape == (shape[0],) and state.dtype == torch.float32
    assert not state.any()
    w, G = start(t, 1)
    steps = 0
    for k in (1, 2):
        d = rand(shape, 10 + k)
        t.add(d, option=OPT)
        t.flush()
        steps += ref_step(w, G, d if wire is None else d.to(wire))
        assert within(t.shard, state, w, G, steps, k)


def test_add_rows_duplicates_and_unlisted(env):
    R, C = 10, 6
    t = mv.MatrixTable(R, C, **KW)
    start(t, 2)
    t.add(rand((R, C), 3), option=OPT)       # G off zero everywhere
    t.flush()
    before, G_before = t.shard.clone(), t.updater.g_sqr_row.clone()
    w, G = before.cpu().double(), G_before.cpu().double()
    vals = ints((len(IDS), C), 4)
    vals[3] = 0                                    # row 0: an all-zero sum
    t.add_rows(IDS, vals, option=OPT)
    touched = sorted(set(IDS))
    step = ref_step(w, G, dense(R, IDS, vals), touched)
    assert within(t.shard, t.updater.g_sqr_row, w, G, step)
    rest = [r for r in range(R) if r not in touched] + [0]
    assert torch.equal(t.shard[rest], before[rest])
    assert torch.equal(t.updater.g_sqr_row[rest], G_before[rest])
    assert not (t.shard[touched[1:]] == before[touched[1:]]).all(1).any()


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("weighted", [False, True])
def test_add_pooled_is_add_rows_of_expanded(env, mode, weighted):
    R, C = 10, 4
    lens = torch.tensor([1, 2, 4, 0, 8, 1])        # exact means
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    n = int(offs[-1])
    ids = torch.randint(0, R, (n,), generator=torch.Generator().manual_seed(5))
    bags, wts = ints((len(lens), C), 6), ints((n,), 7) / 2
    rows = bags[torch.repeat_interleave(torch.arange(len(lens)), lens)]
    if weighted:
        rows = rows * wts.unsqueeze(1)
    if mode == "mean":
        rows = rows / torch.repeat_interleave(lens, lens).unsqueeze(1)
    t, twin = (mv.MatrixTable(R, C, **KW) for _ in range(2))
    start(t, 8), start(twin, 8)
    t.add_pooled(ids, offs, bags, wts if weighted else None, mode, option=OPT)
    twin.add_rows(ids, rows, option=OPT)
    assert torch.equal(t.shard, twin.shard)
    assert torch.equal(t.updater.g_sqr_row, twin.updater.g_sqr_row)
    assert t.updater.g_sqr_row.any()


@pytest.mark.parametrize("make", [
    lambda: mv.ArrayTable(8, **KW),
    lambda: mv.ArrayTable(8, dtype=torch.int32, **KW),
    lambda: mv.MatrixTable(8, 2, dtype=torch.int64, **KW)])
def test_refusals(env, make):
    with pytest.raises(TypeError, match="no rows|int64"):
        make()


def _two_ranks(rank, world, sync):   # top-level: spawn pickles it
    import multiverso_amd as mv
    mv.init(sync=sync)
    assert sync or mv.Zoo.get().async_engine is not None
    R, C = 7, 3                                     # shards of 3 and 4 rows
    t = mv.MatrixTable(R, C, **KW)
    w, G = start(t, 20)
    mine = slice(t.row_offset, t.row_offset + t.local_rows)
    mv.barrier()
    d = ints((R, C), 21)                            # from both ranks
    t.add(d, option=OPT)
    mv.barrier()
    if sync:                                        # one step on the sum
        steps = ref_step(w, G, 2 * d)
    else:                                           # one step per arrival
        steps = ref_step(w, G, d) + ref_step(w, G, d)
    assert within(t.get(), t.updater.g_sqr_row, w, G[mine], steps, 2)
    # keyed, rows of shard 0 only: shard 1 keeps weights and state
    kept = t.shard.clone(), t.updater.g_sqr_row.clone()
    mv.barrier()
    ids, vals = ([1, 2, 1], [0]), (ints((3, C), 23), ints((1, C), 24))
    t.add_rows(ids[rank], vals[rank], option=OPT)
    mv.barrier()
    steps += ref_step(w, G, dense(R, ids[0] + ids[1], torch.cat(vals)),
                      [0, 1, 2])
    assert within(t.get(), t.updater.g_sqr_row, w, G[mine], steps, 3)
    if rank:
        assert torch.equal(t.shard, kept[0])
        assert torch.equal(t.updater.g_sqr_row, kept[1])
    mv.shutdown()


@pytest.mark.parametrize("sync", [True, False])
def test_two_ranks(sync):
    run_dist(functools.partial(_two_ranks, sync=sync), 2)
