"""k_row_pool on the MI355X against the fp64 loop of test_pool_rows.py,
through the row_pool binding and through MatrixTable.pool_rows on one GPU."""

import functools

import pytest
import torch

import multiverso_amd as mv
from conftest import run_dist
from test_pool_rows import assert_pooled, make_case, pool_ref

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
# v4f form: the last width of each group size (16 .. 256), the first of each
# VPL bucket (260, 516), one past a panel (1028). Scalar form: 1, 3, the last
# width of each group (7 .. 63), the first of each bucket (65, 129), 257.
WIDTHS = [1, 3, 4, 7, 15, 16, 31, 32, 63, 64, 65, 128, 129, 256, 257, 260,
          516, 1028]
# around U (4, and 2 at VPL 4) and every group size, 130 and 5000, shuffled
LENS = (16, 0, 5000, 1, 65, 3, 33, 4, 130, 2, 5, 63, 7, 17, 8, 31, 9, 64, 15,
        32, 0)
ROWS = 300


@pytest.fixture(scope="module")
def hip():
    mv.init()
    assert mv.Zoo.get().device.type == "cuda"
    from multiverso_amd import ops
    yield ops.module(required=True)
    mv.shutdown()


@functools.lru_cache(maxsize=None)
def _case(C, ints, lens=LENS):
    return make_case(ROWS, C, lens, 100 + C, ints)


def _pool(hip, table, ids, offs, w, dtype=None):
    return hip.row_pool(table.cuda(), ids.cuda(), offs.cuda(),
                        None if w is None else w.cuda(), dtype)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", WIDTHS)
def test_against_the_loop(hip, C, weighted):
    for ints in (True, False):
        table, ids, offs, w = _case(C, ints)
        w = w if weighted else None
        got = _pool(hip, table, ids, offs, w)
        assert_pooled(got, pool_ref(table, ids, offs, w), offs, exact=ints)
        assert torch.equal(_pool(hip, table, ids, offs, w), got)   # repeatable
        for b in (2, 3, 6, 8):     # alone: another grid, no wave neighbours
            lo, hi = int(offs[b]), int(offs[b + 1])
            alone = _pool(hip, table, ids[lo:hi], torch.tensor([0, hi - lo]),
                          None if w is None else w[lo:hi])
            assert torch.equal(alone[0], got[b]), (b, hi - lo)


@pytest.mark.parametrize("weighted", [False, True])
def test_more_bags_than_groups(hip, weighted):
    """5000 bags of a 64-lane group each: the 1024-block grid holds 4096."""
    for ints in (True, False):
        table, ids, offs, w = _case(200, ints,
                                    tuple(1 + i % 3 for i in range(5000)))
        w = w if weighted else None
        assert_pooled(_pool(hip, table, ids, offs, w),
                      pool_ref(table, ids, offs, w), offs, exact=ints)


@pytest.mark.parametrize("C", [5, 64])
def test_inf_and_nan_stay_in_their_bags(hip, C):
    table, ids, offs, w = (t.clone() for t in _case(C, True))
    table[0, 0], table[-1, C - 1], table[17, 1] = INF, -INF, NAN
    w[ids == 0] = 0.0                     # 0 * inf = NaN, as in the formula
    clean = torch.tensor([not bool(torch.isin(
        ids[offs[b]:offs[b + 1]], torch.tensor([0, 17, ROWS - 1])).any())
        for b in range(len(LENS))])
    assert clean[1] and clean[3] and not clean[2]   # empty, short, long
    for wts in (None, w):
        got = _pool(hip, table, ids, offs, wts).cpu()
        want = pool_ref(table, ids, offs, wts)[0]
        assert torch.equal(got.double().nan_to_num(1e30, 2e30, -2e30),
                           want.nan_to_num(1e30, 2e30, -2e30))
        assert bool(got[clean].isfinite().all())
        assert not bool(got[~clean].isfinite().all(1).any())


@pytest.mark.parametrize("C", [7, 64, 260])
def test_bf16_output_is_the_rounded_fp32(hip, C):
    table, ids, offs, w = _case(C, False)
    for wts in (None, w):
        narrow = _pool(hip, table, ids, offs, wts, torch.bfloat16)
        assert narrow.dtype == torch.bfloat16
        assert torch.equal(narrow,
                           _pool(hip, table, ids, offs, wts).bfloat16())


def test_binding_refusals_and_empty_requests(hip):
    table, ids, offs, w = (t.cuda() for t in _case(4, True))
    for bad in ((table.cpu(), ids, offs, w), (table, ids.cpu(), offs, w),
                (table, ids, offs.cpu(), w), (table, ids, offs, w.cpu()),
                (table[:, ::2], ids, offs, w), (table, ids[::2], offs, None),
                (table, ids, offs[::2], None), (table, ids, offs, w[:-1]),
                (table, ids.int(), offs, w), (table, ids, offs[:0], w),
                (table.double(), ids, offs, None)):
        with pytest.raises(RuntimeError):
            hip.row_pool(*bad)
    none = hip.row_pool(table, ids[:0], offs[:1], None)
    assert none.shape == (0, 4) and none.dtype == torch.float32
    zeros = hip.row_pool(table, ids[:0], offs[:3] * 0, w[:0])
    assert zeros.shape == (2, 4) and not zeros.any()


# ---- table level --------------------------------------------------------
def test_table_sum_mean_and_deferred_add(hip):
    table, ids, offs, w = _case(64, False)
    t = mv.MatrixTable(ROWS, 64)
    t.add(table.cuda())                         # deferred on one rank
    assert t._deferred is not None
    for mode in ("sum", "mean"):
        for args in ((ids, offs, w), (ids.cuda(), offs.cuda(), None)):
            got = t.pool_rows(*args, mode=mode)
            assert got.is_cuda and t._deferred is None
            assert_pooled(got, pool_ref(table, ids, offs, args[2]), offs,
                          mean=mode == "mean")
    ints = _case(64, True)
    tb = mv.MatrixTable(ROWS, 64, wire_dtype=torch.bfloat16)
    tb.shard.copy_(ints[0])
    assert_pooled(tb.pool_rows(*ints[1:]),
                  pool_ref(*ints, bf16_parts=[(0, ROWS)]), ints[2], exact=True)


def _async_gpu(rank, world):
    import multiverso_amd as mv
    mv.init()
    zoo = mv.Zoo.get()
    assert zoo.device.type == "cuda" and zoo.async_engine is not None
    table = make_case(ROWS + 1, 12, LENS, 5, True)[0]
    _, ids, offs, w = make_case(ROWS + 1, 12, LENS, 6 + rank, True)
    t = mv.MatrixTable(ROWS + 1, 12)
    t.shard.copy_(table[t.row_offset:t.row_offset + t.local_rows])
    mv.barrier()
    for wts in (None, w):
        got = t.pool_rows(ids, offs, wts)
        assert got.is_cuda and t.shard.is_cuda
        assert_pooled(got, pool_ref(table, ids, offs, wts), offs, exact=True)
    mv.barrier()
    mv.shutdown()


def test_async_engine_gpu_shards():
    run_dist(_async_gpu, 2, gpu_share=True)
