"""k_row_unpool on the MI355X against the fp64 loop of test_pooled_add.py,
through the unpool_X_update bindings and MatrixTable.add_pooled on one GPU."""

import functools

import pytest
import torch

import multiverso_amd as mv
from conftest import run_dist
from test_pooled_add import make_case, pooled_ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
INF, NAN = float("inf"), float("nan")
ROWS = 300
# the edges of every group size, VPL bucket, panel and the scalar form
WIDTHS = [1, 3, 4, 16, 63, 64, 65, 128, 257, 260, 516, 1028]
# how often a listed row occurs; shuffled over the list, so that the runs of
# the sorted ids straddle the 64-position windows and share waves
COUNTS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130, 3000)
STATES = {"default": 0, "sgd": 0, "adagrad": 1, "momentum": 1, "dcasgd": 1,
          "dcasgda": 2, "adam": 2}
SCALARS = {"default": (), "sgd": (), "adagrad": (0.5, 0.25, 1e-6),
           "momentum": (0.9,), "dcasgd": (0.1, 0.04),
           "dcasgda": (0.1, 0.04, 0.9, 1e-7),
           "adam": (0.9, 0.999, 1e-2, 31.6, 1.0 - 1e-5, 1e-8)}
# max |x - ref| / (1 + |ref|) over weights and G of the whole-table
# adagrad_update (k_elem) against the fp64 formula on a dense delta that holds
# the sums of _case(64, True): measured on the MI355X, profiles/pooled_add.md
ADAGRAD_WHOLE_ERR = 5.735e-8


@pytest.fixture(scope="module")
def hip():
    mv.init()
    assert mv.Zoo.get().device.type == "cuda"
    from multiverso_amd import ops
    yield ops.module(required=True)
    mv.shutdown()


@functools.lru_cache(maxsize=None)
def _case(C, ints, counts=COUNTS, R=ROWS):
    """(table, ids, offsets, vals, weights, exact weights, (sums, S, L) with
    and without the weights): ``counts`` rows listed that often, bags of 1..7
    ids, so one gradient row serves several runs."""
    g = torch.Generator().manual_seed(C)
    n, lens = sum(counts), []
    while sum(lens) < n:
        lens.append(min(1 + len(lens) % 7, n - sum(lens)))
    table, _, offs, vals, w = make_case(R, C, lens, 100 + C, ints)
    ids = torch.repeat_interleave(torch.randperm(R, generator=g)[:len(counts)],
                                  torch.tensor(counts))
    ids = ids[torch.randperm(n, generator=g)]
    wx = torch.tensor([-1.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (n,),
                                                           generator=g)]
    return (table, ids, offs, vals, w, wx,
            {k: pooled_ref(R, ids, offs, vals, x)[1:]
             for k, x in ((False, None), (True, w))})


def _src(offs):
    return torch.repeat_interleave(torch.arange(len(offs) - 1), offs.diff())


def _unpool(hip, name, tensors, ids, offs, vals, w):
    """One unpool_X_update on clones of ``tensors`` (the shard, then the
    state); returns the clones."""
    out = [t.cuda().clone() for t in tensors]
    rows, perm = torch.sort(ids.cuda(), stable=True)
    getattr(hip, f"unpool_{name}_update")(
        *out, rows, perm, _src(offs).cuda(), vals.cuda(),
        None if w is None else w.cuda(), *SCALARS[name])
    return out


def _check_sum(hip, case, weighted, ints):
    table, ids, offs, vals, w = case[:5]
    sums, S, L = case[6][weighted]
    w = w if weighted else None
    got, = _unpool(hip, "default", [table], ids, offs, vals, w)
    err = (got.cpu().double() - (table + sums)).abs()
    tol = (L + 2) * U * (table.abs() + S)
    assert bool((err <= (0 if ints else tol)).all()), float(err.max())
    listed = L.squeeze(1) > 0
    assert torch.equal(got.cpu()[~listed], table[~listed])
    assert torch.equal(_unpool(hip, "default", [table], ids, offs, vals,
                               w)[0], got)                       # repeatable


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", WIDTHS)
def test_sum_against_the_loop(hip, C, weighted):
    for ints in (True, False):
        _check_sum(hip, _case(C, ints), weighted, ints)


@pytest.mark.parametrize("counts,R", [((1,) * 5000, 5000), ((3000,), ROWS)])
def test_more_heads_than_groups_and_one_long_run(hip, counts, R):
    for ints in (True, False):
        _check_sum(hip, _case(8, ints, counts, R), True, ints)


@pytest.mark.parametrize("C", [3, 64, 260])
@pytest.mark.parametrize("name", ["sgd", "momentum", "dcasgd", "dcasgda",
                                  "adam"])
def test_bit_exact_against_the_keyed_kernels(hip, name, C):
    """Equal to row_X_update (sgd: the non-atomic row_scatter_add of rows
    pre-summed in list order in fp32) fed the expanded rows; the weights are
    exact powers of two, so fmaf(w, x, acc) is acc + w*x."""
    table, ids, offs, vals, _, wx = _case(C, False)[:6]
    state = [torch.rand(ROWS, C, generator=torch.Generator().manual_seed(s))
             for s in range(STATES[name])]
    for w in (None, wx):
        rows = vals[_src(offs)] * (1 if w is None else w.unsqueeze(1))
        want = [t.cuda().clone() for t in [table] + state]
        if name == "sgd":
            pre = torch.zeros(ROWS, C)
            for i, r in enumerate(ids.tolist()):
                pre[r] += rows[i]
            u = ids.unique()
            hip.row_scatter_add(want[0], u.cuda(), pre[u].cuda(), -1.0, True)
        else:
            srt, perm = torch.sort(ids.cuda(), stable=True)
            getattr(hip, f"row_{name}_update")(*want, srt, rows.cuda(),
                                               *SCALARS[name], perm)
        got = _unpool(hip, name, [table] + state, ids, offs, vals, w)
        for a, b in zip(got, want, strict=True):
            assert torch.equal(a, b), float((a - b).abs().max())


def test_adagrad_against_the_formula(hip):
    """Integer data, so the sums are the same exact numbers on every path:
    twice the error of the whole-table kernel on a dense delta of them."""
    table, ids, offs, vals, w = _case(64, True)[:5]
    sums = _case(64, True)[6][True][0]
    lr, rho, eps = SCALARS["adagrad"]
    gsq = torch.rand(ROWS, 64, generator=torch.Generator().manual_seed(1))
    G = gsq.double() + (sums / lr) ** 2
    ref = [table.double() - rho * (sums / lr) / (G + eps).sqrt(), G]
    whole = [table.cuda().clone(), gsq.cuda().clone()]
    hip.adagrad_update(whole[0].view(-1), whole[1].view(-1),
                       sums.float().cuda().view(-1), lr, rho, eps)
    got = _unpool(hip, "adagrad", [table, gsq], ids, offs, vals, w)
    errs = [max(float(((x.cpu().double() - r).abs() / (1 + r.abs())).max())
                for x, r in zip(xs, ref)) for xs in (whole, got)]
    print(f"adagrad error: whole-table {errs[0]:.3e}, unpool {errs[1]:.3e}")
    assert errs[1] <= 2 * ADAGRAD_WHOLE_ERR


@pytest.mark.parametrize("C", [7, 64, 260])
def test_bf16_vals_are_the_widened_fp32(hip, C):
    table, ids, offs, vals, w = _case(C, False)[:5]
    state = [torch.zeros(ROWS, C)] * 2
    for name, tensors in (("default", [table]), ("adam", [table] + state)):
        for wts in (None, w):
            narrow = _unpool(hip, name, tensors, ids, offs, vals.bfloat16(),
                             wts)
            wide = _unpool(hip, name, tensors, ids, offs,
                           vals.bfloat16().float(), wts)
            assert all(torch.equal(a, b) for a, b in zip(narrow, wide))


@pytest.mark.parametrize("C", [5, 64])
def test_inf_and_nan_stay_in_their_rows(hip, C):
    table, ids, offs, vals, w = (t.clone() for t in _case(C, True)[:5])
    vals[0, 0], vals[-1, C - 1], vals[17, 1] = INF, -INF, NAN
    src = _src(offs)
    w[src == 0] = 0.0                     # 0 * inf = NaN, as in the formula
    dirty = torch.zeros(ROWS, dtype=torch.bool)
    dirty[ids[torch.isin(src, torch.tensor([0, 17, len(offs) - 2]))]] = True
    assert dirty.any() and not dirty[ids].all()
    for wts in (None, w):
        got = _unpool(hip, "default", [table], ids, offs, vals, wts)[0].cpu()
        want = table + pooled_ref(ROWS, ids, offs, vals, wts)[1]
        assert torch.equal(got.double().nan_to_num(1e30, 2e30, -2e30),
                           want.nan_to_num(1e30, 2e30, -2e30))
        assert bool(got[~dirty].isfinite().all())
        assert not bool(got[dirty].isfinite().all(1).any())


def test_binding_refusals(hip):
    table, ids, offs, vals, w = (t.cuda() for t in _case(4, True)[:5])
    rows, perm = torch.sort(ids, stable=True)
    src = _src(offs.cpu()).cuda()
    good = [table, rows, perm, src, vals, w]
    for at, bad in ((0, table.cpu()), (1, rows.cpu()), (4, vals.cpu()),
                    (0, table[:, ::2]), (1, rows.int()), (2, perm.int()),
                    (3, src.int()), (4, vals.double()), (5, w.double()),
                    (2, perm[:-1]), (3, src[:-1]), (5, w[:-1]),
                    (4, vals.view(-1)),            # declares no P
                    (4, vals[:, :2].contiguous()), (0, table.double())):
        bad = good[:at] + [bad] + good[at + 1:]
        with pytest.raises(RuntimeError):
            hip.unpool_default_update(*bad)
    with pytest.raises(RuntimeError):
        hip.unpool_adam_update(table, table.clone(), table[:5].clone(), rows,
                               perm, src, vals, w, *SCALARS["adam"])


# ---- table level --------------------------------------------------------
def test_table_on_one_gpu(hip):
    from multiverso_amd.dashboard import Dashboard
    table, ids, _, vals, _, wx = _case(64, False)[:6]
    lens = [(1, 2, 4, 8, 0, 16)[i % 6] for i in range(600)]   # exact means
    offs = torch.tensor([0] + lens).cumsum(0)
    ids, wx, vals = ids[:offs[-1]], wx[:offs[-1]], vals[:600]
    for mode, w in (("sum", None), ("mean", wx)):
        rows, sums, S, L = pooled_ref(ROWS, ids, offs, vals, w, mode)
        t = mv.MatrixTable(ROWS, 64, updater_type="sgd")
        t.add(-table.cuda())                        # deferred on one rank
        assert t._deferred is not None
        d2h = Dashboard.get("comm.keyed_d2h").count
        t.add_pooled(ids.cuda(), offs.cuda(), vals.cuda(), w, mode)
        assert Dashboard.get("comm.keyed_d2h").count == d2h + 1
        err = (t.shard.cpu().double() - (table - sums)).abs()
        assert t._deferred is None
        assert bool((err <= (L + 2) * U * (table.abs() + S)).all())
        t, twin = (mv.SparseMatrixTable(ROWS, 64, updater_type="adam")
                   for _ in range(2))
        for s in (t, twin):
            s.get_into(torch.zeros(ROWS, 64, device="cuda"))
        t.add_pooled(ids, offs, vals, w, mode)
        twin.add_rows(ids, rows.float())
        assert torch.equal(t.up_to_date, twin.up_to_date)
        for a in ("shard", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(t.updater, a), getattr(twin.updater, a))
    table, ids, offs, vals, w = _case(64, True)[:5]
    t = mv.MatrixTable(ROWS, 64, wire_dtype=torch.bfloat16)
    t.add_pooled(ids, offs, vals * 259, w)          # 9 bits and more: rounded
    want = pooled_ref(ROWS, ids, offs, (vals * 259).bfloat16().float(), w)[1]
    assert torch.equal(t.shard.cpu().double(), want)


def _async_gpu(rank, world):
    import multiverso_amd as mv
    mv.init()
    zoo = mv.Zoo.get()
    assert zoo.device.type == "cuda" and zoo.async_engine is not None
    table = make_case(ROWS + 1, 12, [1], 5, True)[0]
    lens = [1 + i % 7 for i in range(40)]
    cases = [make_case(ROWS + 1, 12, lens, 6 + r, True)[1:] for r in (0, 1)]
    t = mv.MatrixTable(ROWS + 1, 12)
    t.shard.copy_(table[t.row_offset:t.row_offset + t.local_rows])
    mv.barrier()
    t.add_pooled(*cases[rank])
    mv.barrier()
    want = table + sum(pooled_ref(ROWS + 1, *c)[1] for c in cases)
    assert t.shard.is_cuda and torch.equal(
        t.shard.cpu().double(), want[t.row_offset:t.row_offset + t.local_rows])
    mv.shutdown()


def test_async_engine_gpu_shards():
    run_dist(_async_gpu, 2, gpu_share=True)
