"""k_rowwise_elem and k_row_unpool_rowwise on the MI355X, through the bindings
and through a table on one GPU, against the fp64 rule and the bound of
test_rowwise_adagrad.py; the four forms against each other bit for bit."""

import pytest
import torch

import multiverso_amd as mv
from conftest import run_dist
from test_rowwise_adagrad import (EPS, KW, LR, OPT, RHO, dense, ints, rand,
                                  ref_step, start, within)

pytestmark = pytest.mark.gpu
K = (LR, RHO, EPS)
# the edges of every group size and VPL bucket: v4f form, then scalar form
WIDTHS = [4, 20, 64, 256, 260, 512, 1024, 1, 3, 5, 63, 65, 130, 255]
COUNTS = (1, 2, 3, 5, 16, 17, 63, 64, 65, 130)   # run lengths of the ids
IDS = [5, 49, 5, 0, 17, 5, 17, 30]


def per_wave(C):   # rows a wave: 64 / G, G the smallest group over the row
    v = C // 4 if C % 4 == 0 else C
    return 64 // min(64, max(4, 1 << (v - 1).bit_length()))


# 1 row, one fewer than a wave holds, a ragged last wave; more rows than the
# grid (1024 blocks x 4 waves) has groups, at G = 4 and at G = 64
SHAPES = sorted({(r, c) for c in WIDTHS for r in
                 (1, max(per_wave(c) - 1, 1), 2 * per_wave(c) + 1)})
SHAPES += [(70000, 4), (5000, 1024)]


@pytest.fixture(scope="module")
def hip():
    mv.init()
    assert mv.Zoo.get().device.type == "cuda"
    from multiverso_amd import ops
    yield ops.module(required=True)
    mv.shutdown()


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("R,C", SHAPES)
def test_whole_shard(hip, R, C):
    w, G = rand((R, C), C).double(), torch.zeros(R, dtype=torch.float64)
    plain, again, rev, copy, copy16, wire16 = (
        (w.float().cuda(), torch.zeros(R, device="cuda")) for _ in range(6))
    steps = 0
    for k in (1, 2):
        d = rand((R, C), C + k).bfloat16().float().cuda()
        hip.rowwise_adagrad_update(*plain, d, C, *K)
        hip.rowwise_adagrad_update(*again, d, C, *K)
        hip.rowwise_adagrad_update(*rev, d, C, *K, reverse=True)
        hip.rowwise_adagrad_update(*wire16, d.bfloat16(), C, *K)
        out, out16 = torch.empty_like(d), torch.empty_like(d).bfloat16()
        hip.rowwise_adagrad_copy_update(*copy, d, out, C, *K)
        hip.rowwise_adagrad_copy_update(*copy16, d, out16, C, *K, reverse=True)
        steps += ref_step(w, G, d.cpu())
        assert within(*plain, w, G, steps, k)
        assert all(same(x, plain) for x in (again, rev, copy, copy16, wire16))
        assert torch.equal(out, copy[0])
        assert torch.equal(out16, copy16[0].bfloat16())
    hip.rowwise_adagrad_update(*again, torch.zeros_like(d), C, *K)
    assert same(again, plain)                       # no gradient, no bits


@pytest.mark.parametrize("C", WIDTHS)
def test_keyed_and_pooled_equal_whole_shard(hip, C):
    """Small integers and weights of -1, 1/2, 1, 2: every sum is exact, so the
    summed gradient is the same bits in all forms."""
    R, gen = 300, torch.Generator().manual_seed(C)
    ids = torch.repeat_interleave(torch.randperm(R, generator=gen)[:len(COUNTS)],
                                  torch.tensor(COUNTS))
    ids = ids[torch.randperm(len(ids), generator=gen)]
    src = torch.arange(len(ids)) // 3                # bags of 3 ids
    bags = ints((int(src[-1]) + 1, C), C)
    wts = torch.tensor([-1, .5, 1, 2])[torch.randint(0, 4, ids.shape,
                                                     generator=gen)]
    vals = bags[src] * wts.unsqueeze(1)
    w, G = rand((R, C), 1), rand((R,), 2).abs()
    rows, perm = torch.sort(ids.cuda(), stable=True)
    whole, keyed, keyed16, pooled, uniq = (
        (w.cuda(), G.cuda()) for _ in range(5))
    hip.rowwise_adagrad_update(*whole, dense(R, ids, vals).float().cuda(), C,
                               *K)
    hip.row_rowwise_adagrad_update(*keyed, rows, vals.cuda(), *K, perm)
    hip.row_rowwise_adagrad_update(*keyed16, rows, vals.cuda().bfloat16(), *K,
                                   perm)
    hip.unpool_rowwise_adagrad_update(*pooled, rows, perm, src.cuda(),
                                      bags.cuda(), wts.cuda(), *K)
    assert same(keyed, whole) and same(keyed16, whole) and same(pooled, whole)
    wd, Gd = w.double(), G.double()
    assert within(*keyed, wd, Gd, ref_step(wd, Gd, dense(R, ids, vals)))
    unlisted = torch.ones(R, dtype=torch.bool)
    unlisted[ids] = False
    assert same((keyed[0].cpu()[unlisted], keyed[1].cpu()[unlisted]),
                (w[unlisted], G[unlisted]))
    # the identity list (unique ids, no perm) of add_rows
    whole = w.cuda(), G.cuda()
    some = torch.randperm(R, generator=gen)[:70]
    hip.row_rowwise_adagrad_update(*uniq, some.cuda(), vals[:70].cuda(), *K)
    hip.rowwise_adagrad_update(*whole, dense(R, some, vals[:70]).float().cuda(),
                               C, *K)
    assert same(uniq, whole)


@pytest.mark.parametrize("C", [16, 64, 3])           # G = 4, 16, scalar 4
def test_inf_stays_in_its_row(hip, C):
    R, bad = 40, 17
    w, G, d = rand((R, C), 3), rand((R,), 4).abs(), rand((R, C), 5)
    d[bad, C // 2] = float("inf")
    a, b = (w.cuda(), G.cuda()), (w.cuda(), G.cuda())
    hip.rowwise_adagrad_update(*a, d.cuda(), C, *K)
    hip.row_rowwise_adagrad_update(*b, torch.arange(R).cuda(), d.cuda(), *K)
    rest = [r for r in range(R) if r != bad]
    wd, Gd = w.double(), G.double()
    step = ref_step(wd, Gd, d, rest)
    for x, g in (a, b):
        assert within(x[rest], g[rest], wd[rest], Gd[rest], step[rest])
        assert g[bad] == float("inf") and not x[bad].isfinite().all()


def test_binding_refusals(hip):
    w, G, d = (torch.zeros(s, device="cuda") for s in ((6, 8), (6,), (6, 8)))
    ids, wide = torch.arange(6).cuda(), torch.zeros(2, 1028, device="cuda")
    for bad in ((w.cpu(), G, d, 8), (w, G.cpu(), d, 8), (w, G, d.cpu(), 8),
                (w.t(), G, d, 8), (w, G[:5], d, 8), (w, G, d[:5], 8),
                (w, G, d, 7), (wide, G[:2], wide.clone(), 1028)):
        with pytest.raises(RuntimeError):
            hip.rowwise_adagrad_update(*bad, *K)
    for bad in ((w, G, ids.cpu(), d), (w, G, ids, d[:5]), (w, G[:5], ids, d),
                (w, G, ids, d.t().contiguous().t())):
        with pytest.raises(RuntimeError):
            hip.row_rowwise_adagrad_update(*bad, *K)


# table level: 64 columns in HIP; 257 and 1028 are past the widest row
@pytest.mark.parametrize("C", [64, 257, 1028])
@pytest.mark.parametrize("wire", [None, torch.bfloat16])
def test_table_on_one_gpu(hip, C, wire):
    R, ids = 50, torch.tensor(IDS)
    t = mv.MatrixTable(R, C, wire_dtype=wire, **KW)
    w, G = start(t, 6)
    d, vals = ints((R, C), 7), ints((len(IDS), C), 8)   # exact in bf16 too
    t.add(d.cuda(), option=OPT)                 # deferred on one rank
    assert t._deferred is not None
    got = t.get()                                    # the fused Add+Get
    assert t._deferred is None
    assert torch.equal(got, t.shard.to(got.dtype))
    steps = ref_step(w, G, d)
    assert within(t.shard, t.updater.g_sqr_row, w, G, steps)
    t.add_rows(ids, vals.cuda(), option=OPT)
    steps += ref_step(w, G, dense(R, ids, vals), sorted(set(IDS)))
    offs = torch.arange(0, len(IDS) + 1, 2)          # bags of 2 ids
    t.add_pooled(ids.cuda(), offs.cuda(), vals[:4].cuda(), option=OPT)
    expanded = vals[torch.arange(len(IDS)) // 2]
    steps += ref_step(w, G, dense(R, ids, expanded), sorted(set(IDS)))
    assert within(t.shard, t.updater.g_sqr_row, w, G, steps, 3)   # 3 steps


def _async_gpu(rank, world):
    import multiverso_amd as mv
    mv.init()
    zoo = mv.Zoo.get()
    assert zoo.device.type == "cuda" and zoo.async_engine is not None
    R, C = 41, 12
    t = mv.MatrixTable(R, C, **KW)
    w, G = start(t, 9)
    mv.barrier()
    # rank r names rows r, r + 2, ...: no row gets steps from both ranks
    ids = [torch.tensor([r, r + 2, r + 38, r + 2, r + 20, r]) for r in (0, 1)]
    bags = [ints((3, C), 10 + r) for r in (0, 1)]
    t.add_pooled(ids[rank], torch.tensor([0, 2, 4, 6]), bags[rank], option=OPT)
    mv.barrier()
    d = sum(dense(R, i, b[torch.arange(6) // 2]) for i, b in zip(ids, bags))
    step = ref_step(w, G, d, sorted(set(torch.cat(ids).tolist())))
    mine = slice(t.row_offset, t.row_offset + t.local_rows)
    assert t.shard.is_cuda
    assert within(t.shard, t.updater.g_sqr_row, w[mine], G[mine], step[mine])
    mv.shutdown()


def test_async_engine_gpu_shards():
    run_dist(_async_gpu, 2, gpu_share=True)
