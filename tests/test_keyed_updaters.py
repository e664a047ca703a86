"""Row-keyed Add (add_rows) on momentum / dcasgd / dcasgda tables, CPU tier:
duplicates of one batch are summed, the updater steps once per distinct row,
and rows that are not in the batch keep their weights and their state."""

import numpy as np
import pytest
import torch

import multiverso_amd as mv

from conftest import run_dist

STATEFUL = ["momentum", "dcasgd", "dcasgda"]


@pytest.fixture()
def env():
    mv.init()
    yield
    mv.shutdown()


def option_for(name, worker_id=0):
    if name == "momentum":
        return mv.AddOption(momentum=0.5)
    return mv.AddOption(worker_id=worker_id, learning_rate=0.1, lambda_=0.5,
                        rho=0.9)


def state_of(t, name, worker_id=0):
    """Weights and every state tensor of the table's updater, as rows."""
    shape = (t.local_rows, t.num_col)
    u = t.updater
    out = [t.shard.clone()]
    if name == "momentum":
        out.append(u.smooth_gradient.view(shape).clone())
    elif name == "adagrad":
        out.append(u.g_sqr.view(shape).clone())
    elif name in ("dcasgd", "dcasgda"):
        out.append(u._backup(worker_id).view(shape).clone())
    if name == "dcasgda":
        out.append(u.mean_sqr.view(shape).clone())
    return out


def test_momentum_hand_computed(env):
    t = mv.MatrixTable(6, 2, updater_type="momentum")
    opt = mv.AddOption(momentum=0.5)
    t.add_rows([1, 4], torch.ones(2, 2), option=opt)  # m = .5,  w = -.5
    t.add_rows([1, 4], torch.ones(2, 2), option=opt)  # m = .75, w = -1.25
    want = torch.zeros(6, 2)
    want[[1, 4]] = -1.25
    assert torch.equal(t.get(), want)
    want_m = torch.zeros(6, 2)
    want_m[[1, 4]] = 0.75
    assert torch.equal(t.updater.smooth_gradient.view(6, 2), want_m)


@pytest.mark.parametrize("name", STATEFUL)
def test_duplicates_are_summed(env, name):
    # multiples of 1/8: a + b is exact in fp32 in any order, so both tables
    # hand their updater bit-identical per-row sums
    a = torch.tensor([0.5, 1.25, -2.0])
    b = torch.tensor([1.5, -0.25, 4.0])
    c = torch.tensor([3.0, 0.125, -1.0])
    opt = option_for(name)
    t1 = mv.MatrixTable(7, 3, updater_type=name)
    t2 = mv.MatrixTable(7, 3, updater_type=name)
    for _ in range(2):   # the second round runs on non-zero state
        t1.add_rows([2, 2, 5], torch.stack([a, b, c]), option=opt)
        t2.add_rows([2, 5], torch.stack([a + b, c]), option=opt)
    s1, s2 = state_of(t1, name), state_of(t2, name)
    assert s1[0][2].abs().sum() > 0
    for x, y in zip(s1, s2):
        assert torch.equal(x, y)


def test_dcasgd_hand_computed(env):
    """The numbers of test_local.py::test_dcasgd_updater, on rows 2 and 7
    of a 9x4 table."""
    t = mv.MatrixTable(9, 4, updater_type="dcasgd")
    rows = [2, 7]
    g = torch.full((2, 4), 2.0)
    opt0 = mv.AddOption(worker_id=0, learning_rate=0.1, lambda_=0.5)
    opt1 = mv.AddOption(worker_id=1, learning_rate=0.1, lambda_=0.5)
    for opt, want in [(opt0, -0.2), (opt1, -0.4), (opt0, -0.56)]:
        t.add_rows(rows, g, option=opt)
        got = t.get()
        assert torch.allclose(got[rows], torch.full((2, 4), want))
        rest = torch.ones(9, dtype=torch.bool)
        rest[rows] = False
        assert torch.equal(got[rest], torch.zeros(7, 4))


def test_dcasgda_hand_computed(env):
    """test_local.py::test_dcasgda_updater through add_rows, then a third
    step from another worker slot against the formula."""
    t = mv.MatrixTable(9, 4, updater_type="dcasgda")
    rows = [2, 7]
    g = torch.full((2, 4), 2.0)
    opt = mv.AddOption(learning_rate=0.1, lambda_=0.5, rho=0.9)
    t.add_rows(rows, g, option=opt)
    assert torch.allclose(t.get()[rows], torch.full((2, 4), -0.2))
    t.add_rows(rows, g, option=opt)
    assert torch.allclose(t.get()[rows], torch.full((2, 4), -0.4))
    # worker 1's backup starts at the current weights; worker 0 then steps
    # with bak = -0.4 at w = -0.6
    opt1 = mv.AddOption(worker_id=1, learning_rate=0.1, lambda_=0.5, rho=0.9)
    t.add_rows(rows, g, option=opt1)
    assert torch.allclose(t.get()[rows], torch.full((2, 4), -0.6))
    t.add_rows(rows, g, option=opt)
    m = 0.4
    for _ in range(3):
        m = 0.9 * m + 0.1 * 4.0
    lam_t = 0.5 / np.sqrt(m + 1e-7)
    want = -0.6 - 0.1 * (2.0 + lam_t * 4.0 * (-0.6 - -0.4))
    got = t.get()
    assert torch.allclose(got[rows], torch.full((2, 4), float(want)))
    assert torch.allclose(t.updater.mean_sqr.view(9, 4)[rows],
                          torch.full((2, 4), float(m)))
    rest = torch.ones(9, dtype=torch.bool)
    rest[rows] = False
    assert torch.equal(got[rest], torch.zeros(7, 4))
    assert torch.equal(t.updater.mean_sqr.view(9, 4)[rest], torch.zeros(7, 4))


@pytest.mark.parametrize("name", STATEFUL)
def test_option_none_and_empty_batch(env, name):
    t = mv.MatrixTable(5, 3, updater_type=name)
    twin = mv.MatrixTable(5, 3, updater_type=name)
    delta = torch.zeros(5, 3)
    delta[[0, 3]] = torch.tensor([[1.0, 2.0, -1.0], [0.5, 0.0, 4.0]])
    t.add_rows([0, 3], delta[[0, 3]])          # option=None
    # option=None means what it means for the whole-table update(): on a
    # fresh table (all state zero) a zero delta row is a no-op for each of
    # the three updaters, so the twin's whole-table Add is the oracle
    twin.add(delta)
    assert torch.allclose(t.get(), twin.get(), rtol=1e-6, atol=1e-6)
    assert t.get()[0].abs().sum() > 0
    before = state_of(t, name)
    t.add_rows([], torch.zeros(0, 3))
    t.add_rows([], torch.zeros(0, 3), option=option_for(name))
    for x, y in zip(before, state_of(t, name)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", STATEFUL + ["default", "sgd", "adagrad"])
def test_all_rows_equals_whole_table(env, name):
    R, C = 9, 3
    g = torch.Generator().manual_seed(11)
    opt = option_for(name)
    keyed = mv.MatrixTable(R, C, updater_type=name)
    whole = mv.MatrixTable(R, C, updater_type=name)
    for _ in range(3):
        delta = torch.randn(R, C, generator=g)
        keyed.add_rows(torch.arange(R), delta, option=opt)
        whole.add(delta, option=opt)
    for x, y in zip(state_of(keyed, name), state_of(whole, name)):
        assert torch.allclose(x, y, rtol=1e-6, atol=1e-6)
    assert keyed.get().abs().sum() > 0


def test_float64_momentum(env):
    t = mv.MatrixTable(6, 3, dtype=torch.float64, updater_type="momentum")
    opt = mv.AddOption(momentum=0.25)
    g = torch.Generator().manual_seed(3)
    m = torch.zeros(6, 3, dtype=torch.float64)
    w = torch.zeros(6, 3, dtype=torch.float64)
    for ids in ([0, 4, 4], [4, 5]):
        vals = torch.randn(len(ids), 3, generator=g, dtype=torch.float64)
        t.add_rows(ids, vals, option=opt)
        for r in sorted(set(ids)):
            s = sum(vals[k] for k, i in enumerate(ids) if i == r)
            m[r] = 0.25 * m[r] + 0.75 * s
            w[r] -= m[r]
    got = t.get()
    assert got.dtype == torch.float64
    assert torch.allclose(got, w, rtol=1e-12, atol=1e-12)
    assert torch.allclose(t.updater.smooth_gradient.view(6, 3), m,
                          rtol=1e-12, atol=1e-12)
    assert torch.equal(got[[1, 2, 3]], torch.zeros(3, 3, dtype=torch.float64))


def test_deterministic_flag(env):
    """The flag's pre-sum of duplicate rows feeds the same one step."""
    mv.set_flag("deterministic", True)
    try:
        t = mv.MatrixTable(6, 2, updater_type="momentum")
        t.add_rows([4, 1, 4], torch.ones(3, 2),
                   option=mv.AddOption(momentum=0.5))
    finally:
        mv.set_flag("deterministic", False)
    want = torch.zeros(6, 2)
    want[1] = -0.5
    want[4] = -1.0
    assert torch.equal(t.get(), want)


# ---- two ranks (worker functions are top-level for spawn pickling) ----

def _sync_momentum(rank, world):
    import multiverso_amd as mv
    mv.init(sync=True)
    t = mv.MatrixTable(12, 4, updater_type="momentum")
    opt = mv.AddOption(momentum=0.5)
    ids = [3, 9] + ([7] if rank == 1 else [])
    t.add_rows(ids, torch.ones(len(ids), 4), option=opt)
    got = t.get()
    want = torch.zeros(12, 4)
    want[[3, 9]] = -1.0   # one step on the sum 2: m = 1
    want[7] = -0.5
    assert torch.equal(got, want), (rank, got)
    mv.shutdown()


def test_two_ranks_sync_plane():
    run_dist(_sync_momentum, 2)


def _async_momentum(rank, world):
    import multiverso_amd as mv
    mv.init()
    assert mv.Zoo.get().async_engine is not None
    t = mv.MatrixTable(12, 4, updater_type="momentum")
    t.add_rows([3], torch.ones(1, 4), option=mv.AddOption(momentum=0.5))
    mv.barrier()
    got = t.get()
    want = torch.zeros(12, 4)
    want[3] = -1.25       # two steps: m = .5, then .75
    assert torch.equal(got, want), (rank, got)
    mv.shutdown()


def test_two_ranks_async_plane():
    run_dist(_async_momentum, 2)


def test_sparse_matrix_table_momentum(env):
    t = mv.SparseMatrixTable(8, 3, updater_type="momentum")
    opt = mv.AddOption(momentum=0.5)
    t.add_rows([6, 1, 6], torch.ones(3, 3), option=opt)   # row 6: sum 2
    want = torch.zeros(8, 3)
    want[1] = -0.5
    want[6] = -1.0
    assert torch.equal(t.get(), want)
    assert torch.equal(t.get_rows([6, 1, 0]), want[[6, 1, 0]])
