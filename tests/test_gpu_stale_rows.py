"""GPU tests of SparseMatrixTable's stale-row Get in HIP: the stale_count /
stale_emit bindings (k_stale_count, k_stale_scan, k_stale_emit) against
torch's nonzero, row_gather_at, and the table on one GPU. Integers and copied
floats are compared exactly."""

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -5.0
GUARD = 5          # odd: the bitmap starts 1 byte past a 4-byte boundary
FRESH = 7          # any non-zero byte is fresh, and stays what it is


@pytest.fixture(scope="module")
def hip():
    from multiverso_amd import ops
    return ops.module(required=True)


def ref_take(bitmap, w0, w1):
    """torch reference on a CPU copy: (counts, ids, bitmap afterwards)."""
    after = bitmap.clone()
    lists = [(bitmap[w] == 0).nonzero().reshape(-1) for w in range(w0, w1)]
    for w, stale in zip(range(w0, w1), lists):
        after[w, stale] = 1
    ids = torch.cat(lists) if lists else torch.empty(0, dtype=torch.int64)
    return [int(s.numel()) for s in lists], ids, after


def pattern(kind, nw, R):
    g = torch.Generator().manual_seed(1000 * nw + R)
    if kind == "all":
        return torch.zeros(nw, R, dtype=torch.uint8)
    if kind.startswith("p"):
        return (torch.rand(nw, R, generator=g) >= float(kind[1:])).to(
            torch.uint8) * FRESH
    fresh = torch.full((nw, R), FRESH, dtype=torch.uint8)
    if kind == "last":
        fresh[:, R - 1] = 0
    return fresh


@pytest.mark.parametrize("kind", ["all", "none", "p0.5", "p0.01", "last"])
@pytest.mark.parametrize("nw", [1, 3])
@pytest.mark.parametrize("R", [1, 3, 4, 5, 1023, 1024, 1025, 2051, 5000])
def test_bindings_against_nonzero(hip, R, nw, kind):
    start = pattern(kind, nw, R)
    ranges = [(0, nw), (1, 1)] if nw == 1 else [(0, nw), (1, 2), (1, 1)]
    for w0, w1 in ranges:
        buf = torch.zeros(nw * R + 2 * GUARD, dtype=torch.uint8, device="cuda")
        bitmap = buf[GUARD:GUARD + nw * R].view(nw, R)
        bitmap.copy_(start)
        assert bitmap.data_ptr() % 4 == 1
        counts, ids, after = ref_take(start, w0, w1)
        plan, totals = hip.stale_count(bitmap, w0, w1)
        assert totals.device.type == "cpu" and totals.dtype == torch.int64
        assert totals.tolist() == counts
        got = hip.stale_emit(bitmap, plan, w0, w1, sum(counts))
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), ids)
        # the range is fresh; the other workers and the guards are untouched
        assert torch.equal(bitmap.cpu(), after)
        assert bool((after[w0:w1] != 0).all())
        assert not buf[:GUARD].any() and not buf[GUARD + nw * R:].any()
        assert hip.stale_count(bitmap, w0, w1)[1].tolist() == [0] * (w1 - w0)


def test_no_rows(hip):
    bitmap = torch.zeros(3, 0, dtype=torch.bool, device="cuda")
    plan, totals = hip.stale_count(bitmap, 0, 3)
    assert totals.tolist() == [0, 0, 0]
    assert hip.stale_emit(bitmap, plan, 0, 3, 0).numel() == 0


@pytest.mark.parametrize("shift", [0, 1])   # out 16-byte aligned, or 4 off
@pytest.mark.parametrize("cols", [1, 3, 4, 50])
def test_row_gather_at(hip, cols, shift):
    R = 1000
    g = torch.Generator().manual_seed(cols)
    shard = torch.randn(R, cols, generator=g).cuda()
    rows = torch.cat([torch.tensor([R - 1, 0]),
                      torch.randperm(R - 2, generator=g)[:600] + 1]).cuda()
    buf = torch.full((R * cols + 2,), SENTINEL, device="cuda")
    out = buf[shift:shift + R * cols].view(R, cols)
    hip.row_gather_at(out, shard, rows[:0])
    assert bool((buf == SENTINEL).all())
    hip.row_gather_at(out, shard, rows)
    want = torch.full((R, cols), SENTINEL, device="cuda")
    want[rows] = shard[rows]
    assert torch.equal(out, want)
    assert float(buf[shift - 1]) == SENTINEL and float(buf[-1]) == SENTINEL


@pytest.mark.parametrize("cols", [3, 50])
def test_table_one_rank(cols):
    import multiverso_amd as mv
    R = 2051
    mv.init()
    t = mv.SparseMatrixTable(R, cols)
    g = torch.Generator().manual_seed(cols)
    ids = torch.randint(0, R, (300,), generator=g)
    vals = torch.randn(300, cols, generator=g).cuda()
    distinct = ids.unique().cuda()
    untouched = torch.ones(R, dtype=torch.bool, device="cuda")
    untouched[distinct] = False
    cache = torch.empty(R, cols, device="cuda")
    assert t.get_into(cache) == R    # a new table is stale everywhere

    def check_touched(view):
        table = t.get()
        assert torch.equal(view[distinct], table[distinct])
        assert bool((view[untouched] == SENTINEL).all())

    t.add_rows(ids, vals)
    cache.fill_(SENTINEL)
    assert t.get_into(cache) == distinct.numel()
    check_touched(cache)
    before = cache.clone()
    assert t.get_into(cache) == 0 and torch.equal(cache, before)
    # a strided cache takes the gather + index_put fallback
    t.add_rows(ids, vals)
    wide = torch.full((R, cols + 3), SENTINEL, device="cuda")
    assert t.get_into(wide[:, 1:1 + cols]) == distinct.numel()
    check_touched(wide[:, 1:1 + cols])
    assert bool((wide[:, 0] == SENTINEL).all())
    assert bool((wide[:, 1 + cols:] == SENTINEL).all())
    # a whole-table add makes every row stale
    t.add(torch.ones(R, cols, device="cuda"))
    cache.fill_(SENTINEL)
    assert t.get_into(cache) == R and torch.equal(cache, t.get())
    mv.shutdown()


def test_several_workers_one_gpu():
    import multiverso_amd as mv
    R, cols = 2051, 3
    mv.init()
    t = mv.SparseMatrixTable(R, cols)
    t.shard.copy_(torch.randn(R, cols, generator=torch.Generator()
                              .manual_seed(4)))
    start = pattern("p0.3", 3, R).bool()
    counts, ids, after = ref_take(start, 0, 3)
    t.up_to_date = start.cuda()
    got_counts, got_ids = t._take_stale(0, 3)
    assert got_counts == counts and torch.equal(got_ids.cpu(), ids)
    assert torch.equal(t.up_to_date.cpu(), after)
    _, ids1, after1 = ref_take(start, 1, 2)
    t.up_to_date = start.cuda()
    gids, served = t._server_stale_for(1)
    assert torch.equal(gids.cpu(), ids1 + t.row_offset)
    assert torch.equal(served, t.shard[ids1.cuda()])
    assert torch.equal(t.up_to_date.cpu(), after1)
    mv.shutdown()


@pytest.mark.parametrize("bad", ["cpu", "dtype", "strided", "range",
                                 "gather_cpu", "gather_dtype", "gather_cols"])
def test_refusals(hip, bad):
    bitmap = torch.zeros(3, 8, dtype=torch.bool, device="cuda")
    shard = torch.zeros(8, 4, device="cuda")
    rows = torch.arange(2, device="cuda")
    with pytest.raises(RuntimeError):
        if bad == "cpu":
            hip.stale_count(bitmap.cpu(), 0, 3)
        elif bad == "dtype":
            hip.stale_count(bitmap.to(torch.int32), 0, 3)
        elif bad == "strided":
            hip.stale_count(bitmap[:, ::2], 0, 3)
        elif bad == "range":
            hip.stale_count(bitmap, 2, 1)
        elif bad == "gather_cpu":
            hip.row_gather_at(shard.cpu(), shard, rows)
        elif bad == "gather_dtype":
            hip.row_gather_at(shard.double(), shard, rows)
        else:
            hip.row_gather_at(torch.zeros(8, 5, device="cuda"), shard, rows)
