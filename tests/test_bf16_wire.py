"""bf16 wire format (``wire_dtype=torch.bfloat16``), CPU tier: fp32 master
shard and updater state, bfloat16 Add deltas and Get results. The oracle is
a table without the keyword that is fed the deltas rounded to bf16 and
widened again: the wire table must leave the same fp32 shard, bit for bit,
and return that shard rounded to bf16."""

import os

import pytest
import torch

import multiverso_amd as mv

from conftest import run_dist

BF16 = torch.bfloat16
UPDATERS = ["default", "sgd", "momentum", "adagrad", "dcasgd", "dcasgda",
            "adam"]


@pytest.fixture()
def env():
    mv.init()
    yield
    mv.shutdown()


def option_for(name):
    if name in ("default", "sgd"):
        return None
    if name == "momentum":
        return mv.AddOption(momentum=0.5)
    if name == "adagrad":
        return mv.AddOption(learning_rate=0.1, rho=0.1)
    if name == "adam":
        return mv.AddOption.adam(lr=0.01, weight_decay=0.1)
    return mv.AddOption(learning_rate=0.1, lambda_=0.5, rho=0.9)


def rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def rounded(x):
    """What the wire carries, widened again."""
    return x.to(BF16).float()


# ---- construction ----

@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float64])
def test_bf16_needs_a_float32_table(env, dtype):
    with pytest.raises(TypeError, match="wire_dtype"):
        mv.ArrayTable(8, dtype=dtype, wire_dtype=BF16)
    with pytest.raises(TypeError, match="wire_dtype"):
        mv.MatrixTable(4, 2, dtype=dtype, wire_dtype=BF16)


def test_other_wire_dtypes_are_rejected(env):
    with pytest.raises(TypeError, match="wire_dtype"):
        mv.ArrayTable(8, wire_dtype=torch.float16)
    with pytest.raises(TypeError, match="wire_dtype"):
        mv.MatrixTable(4, 2, dtype=torch.float64, wire_dtype=torch.float32)


def test_sparse_table_takes_no_wire_dtype(env):
    with pytest.raises(TypeError):
        mv.SparseMatrixTable(8, 2, wire_dtype=BF16)
    with pytest.raises(TypeError):
        mv.SparseMatrixTable(8, 2, wire_dtype=None)


@pytest.mark.parametrize("wire", [None, torch.float32])
def test_fp32_wire_is_todays_table(env, wire):
    plain = mv.MatrixTable(5, 3, updater_type="sgd")
    t = mv.MatrixTable(5, 3, updater_type="sgd", wire_dtype=wire)
    a = mv.ArrayTable(9, wire_dtype=wire)
    assert t.wire == torch.float32 and a.wire == torch.float32
    d = rand((5, 3), 1)          # not representable in bf16: must not round
    plain.add(d)
    t.add(d)
    got = t.get()
    assert got.dtype == torch.float32
    assert torch.equal(got, plain.get())
    assert torch.equal(got, -d)
    # a bf16 delta handed to such a table is still widened
    a.add(rand(9, 2).to(BF16))
    got = a.get()
    assert got.dtype == torch.float32
    assert torch.equal(got, rounded(rand(9, 2)))
    rows = t.get_rows([4, 0])
    assert rows.dtype == torch.float32
    assert torch.equal(rows, -d[[4, 0]])


# ---- single-rank equivalence ----

def check_equivalence(wire_t, oracle_t, shape, name):
    opt = option_for(name)
    for k in range(3):
        d = rand(shape, 10 + k)
        # a bf16 input is taken as it is, an fp32 one is rounded once
        wire_t.add(d.to(BF16) if k == 1 else d, option=opt)
        oracle_t.add(rounded(d), option=opt)
    got = wire_t.get()
    want = oracle_t.get()
    assert wire_t.shard.dtype == torch.float32
    assert torch.equal(wire_t.shard, oracle_t.shard)
    assert wire_t.shard.abs().sum() > 0
    assert got.dtype == BF16 and got.shape == want.shape
    assert torch.equal(got, want.to(BF16))
    out32 = torch.full(shape, 7.0)
    assert wire_t.get(out=out32) is out32
    assert torch.equal(out32, want.to(BF16).float())
    out16 = torch.zeros(shape, dtype=BF16)
    assert wire_t.get(out=out16) is out16
    assert torch.equal(out16, want.to(BF16))


@pytest.mark.parametrize("name", UPDATERS)
@pytest.mark.parametrize("size", [5, 1029])
def test_array_matches_rounded_delta_oracle(env, name, size):
    check_equivalence(mv.ArrayTable(size, updater_type=name, wire_dtype=BF16),
                      mv.ArrayTable(size, updater_type=name), (size,), name)


@pytest.mark.parametrize("name", UPDATERS)
def test_matrix_matches_rounded_delta_oracle(env, name):
    check_equivalence(
        mv.MatrixTable(33, 7, updater_type=name, wire_dtype=BF16),
        mv.MatrixTable(33, 7, updater_type=name), (33, 7), name)


def test_strided_out(env):
    t = mv.MatrixTable(6, 4, wire_dtype=BF16)
    d = rand((6, 4), 3)
    t.add(d)
    big = torch.zeros(6, 8, dtype=BF16)
    view = big[:, ::2]
    assert t.get(out=view) is view
    assert torch.equal(view, d.to(BF16))


# ---- keyed ----

IDS = [2, 30, 2, 7, 2, 30, 0]


@pytest.mark.parametrize("name", ["default", "momentum", "adagrad", "adam"])
def test_add_rows_with_duplicates(env, name):
    t = mv.MatrixTable(33, 7, updater_type=name, wire_dtype=BF16)
    o = mv.MatrixTable(33, 7, updater_type=name)
    opt = option_for(name)
    for k in range(2):
        v = rand((len(IDS), 7), 20 + k)
        t.add_rows(IDS, v, option=opt)
        o.add_rows(IDS, rounded(v), option=opt)
    assert torch.equal(t.shard, o.shard)
    assert t.shard[2].abs().sum() > 0
    got = t.get_rows([30, 2, 5, 2])
    assert got.dtype == BF16 and got.shape == (4, 7)
    assert torch.equal(got, o.get_rows([30, 2, 5, 2]).to(BF16))


def test_get_rows_rounds_the_master(env):
    t = mv.MatrixTable(8, 3, wire_dtype=BF16)
    w = rand((8, 3), 4)
    t.shard.copy_(w)               # a master that bf16 cannot hold
    got = t.get_rows([7, 1, 1])
    assert got.dtype == BF16
    assert torch.equal(got, w[[7, 1, 1]].to(BF16))
    assert torch.equal(t.shard, w)  # reading never rounds the shard


@pytest.mark.parametrize("deterministic", [False, True])
def test_duplicate_sum_is_not_rerounded(env, deterministic):
    # 1 + 2^-9 + 2^-9 = 1 + 2^-8: every addend is a bf16 value, the sum is a
    # tie that bf16 would round back to 1
    v = torch.tensor([[1.0], [2.0 ** -9], [2.0 ** -9], [3.0]])
    assert torch.equal(rounded(v), v)
    mv.set_flag("deterministic", deterministic)
    try:
        t = mv.MatrixTable(6, 1, wire_dtype=BF16)
        t.add_rows([3, 3, 3, 5], v)
    finally:
        mv.set_flag("deterministic", False)
    want = torch.zeros(6, 1)
    want[3] = 1.0 + 2.0 ** -8
    want[5] = 3.0
    assert want[3].to(BF16).float() != want[3]
    assert torch.equal(t.shard, want)


# ---- store / load ----

def test_store_load_keep_the_fp32_master(env, tmp_path):
    path = os.path.join(tmp_path, "m.bin")
    t = mv.MatrixTable(9, 5, updater_type="momentum", wire_dtype=BF16)
    t.add(rand((9, 5), 5), option=mv.AddOption(momentum=0.3))
    t.add(rand((9, 5), 6), option=mv.AddOption(momentum=0.3))
    master = t.shard.clone()
    assert not torch.equal(master, rounded(master))
    t.store(path)
    assert os.path.getsize(path) == 9 * 5 * 4
    t2 = mv.MatrixTable(9, 5, wire_dtype=BF16)
    t2.load(path)
    assert torch.equal(t2.shard, master)
    a = mv.ArrayTable(11, wire_dtype=BF16)
    a.shard.copy_(rand(11, 7))
    apath = os.path.join(tmp_path, "a.bin")
    a.store(apath)
    a2 = mv.ArrayTable(11)
    a2.load(apath)
    assert torch.equal(a2.shard, a.shard)


# ---- two ranks: integer-valued deltas, every partial sum exact in bf16 ----

def _exercise_two_ranks(rank, world, uneven_rows):
    """Whole and keyed ops on wire tables; the same checks hold on the
    collective plane and on the async plane (a barrier fences the Adds)."""
    # whole-table Add/Get, uneven shards: 7 elements over 2 ranks
    a = mv.ArrayTable(7, wire_dtype=BF16)
    assert a.shard.dtype == torch.float32
    base = torch.arange(7, dtype=torch.float32)
    a.add(base * (rank + 1))
    mv.barrier()
    got = a.get()
    assert got.dtype == BF16
    tri = world * (world + 1) // 2
    assert torch.equal(got, (base * tri).to(BF16)), (rank, got)
    out32 = torch.empty(7)
    a.get(out=out32)
    assert torch.equal(out32, base * tri)
    off, cnt = a.spec.range_of(rank)
    assert torch.equal(a.shard, base[off:off + cnt] * tri)

    # stateful updater behind the wire: momentum mu = 0 is w -= sum of deltas
    m = mv.MatrixTable(uneven_rows, 3, updater_type="momentum",
                       wire_dtype=BF16)
    d = torch.arange(uneven_rows * 3, dtype=torch.float32).view(-1, 3)
    m.add(d.to(BF16), option=mv.AddOption(momentum=0.0))
    mv.barrier()
    got = m.get()
    assert got.dtype == BF16
    assert torch.equal(got, (-d * world).to(BF16)), (rank, got)

    # keyed: both ranks hit row 0 and the last row, plus one row of their own
    k = mv.MatrixTable(uneven_rows, 4, wire_dtype=BF16)
    last = uneven_rows - 1
    k.add_rows([0, last, 1 + rank, 0],
               torch.full((4, 4), float(rank + 1)))
    mv.barrier()
    rows = k.get_rows([last, 0, 1, 2])
    assert rows.dtype == BF16 and rows.shape == (4, 4)
    want = torch.tensor([tri, 2 * tri, 1, 2], dtype=torch.float32)
    assert torch.equal(rows.float(), want.view(4, 1).expand(4, 4)), (rank,
                                                                     rows)
    mv.barrier()


def _sync_plane(rank, world):
    mv.init(sync=True)
    _exercise_two_ranks(rank, world, uneven_rows=5)
    mv.shutdown()


def _async_plane(rank, world):
    mv.init()
    assert mv.Zoo.get().async_engine is not None
    _exercise_two_ranks(rank, world, uneven_rows=5)
    base = torch.arange(40, dtype=torch.float32).view(10, 4)
    # tables without the bf16 wire still cast into a Get buffer of another
    # dtype, whichever side owns the chunk
    p = mv.MatrixTable(10, 4)
    p.add(base * (rank + 1))
    q = mv.ArrayTable(7, dtype=torch.float64)
    q.add(torch.arange(7, dtype=torch.float64) * (rank + 1))
    mv.barrier()
    for dt in (torch.float64, torch.float16, BF16):
        out = torch.zeros(10, 4, dtype=dt, device="cpu")
        assert p.get(out=out) is out
        assert torch.equal(out.cpu(), (3 * base).to(dt)), (rank, dt, out)
    out = torch.zeros(7, device="cpu")
    assert q.get(out=out) is out
    assert torch.equal(out.cpu(), 3 * torch.arange(7.0)), (rank, out)
    assert p.get().dtype == torch.float32 and q.get().dtype == torch.float64
    # unequal op counts: nobody waits for anybody
    t = mv.ArrayTable(7, wire_dtype=BF16)
    for _ in range(2 if rank == 0 else 5):
        t.add(torch.ones(7))
        assert t.get().dtype == BF16
    mv.barrier()
    assert torch.equal(t.get(), torch.full((7,), 7.0, dtype=BF16))
    mv.barrier()
    mv.shutdown()


def test_two_ranks_sync_plane():
    run_dist(_sync_plane, 2)


def test_two_ranks_async_plane():
    run_dist(_async_plane, 2)
