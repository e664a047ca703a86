"""GPU tests of the "adam" updater: the AdamOp bodies behind adam_update /
adam_copy_update (k_elem) and row_adam_update (k_row_update), and an adam
MatrixTable that lives on the GPU.

The oracle is the formula in float64 on the same fp32 inputs. State starts at
m = randn, v = |randn| + 0.1, so the denominator stays conditioned and the
error measured is the kernel's, not a cancellation's; one case starts from
zero state at t = 1, where the bias corrections are largest (1 - b2 = 1e-3).
Tolerance for w, m and v: rtol 1e-5, atol 1e-6, the project's dcasgd pair;
every op of the body is correctly rounded fp32 (eps 6e-8) on operands of
magnitude ~1. Each case prints its max abs error."""

import functools

import pytest
import torch

from conftest import run_dist

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-6
EPS = 1e-8
LR, B1, B2 = 0.01, 0.9, 0.999
R, N = 300, 257
# scalar with one lane per row, scalar odd, v4f with two vectors per row,
# v4f with a row spanning half a wave
COLS = [1, 7, 8, 128]
# tail only, one vector, body plus tail, many blocks
SIZES = [1, 3, 4, 1029, 262147]


@pytest.fixture(scope="module")
def hip():
    from multiverso_amd import ops
    return ops.module(required=True)


def rand(shape, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=dtype)


def scalars(t, wd=0.0, lr=LR, b1=B1, b2=B2):
    """What AdamUpdater.next_scalars hands the kernel for update count t."""
    return (b1, b2, lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** -0.5,
            1.0 - lr * wd, EPS)


def formula(w, m, v, g, t, wd=0.0, lr=LR, b1=B1, b2=B2):
    """New (w, m, v) in float64 from tensors of any float dtype."""
    w, m, v, g = (x.double().cpu() for x in (w, m, v, g))
    w = w * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    w = w - (lr / (1 - b1 ** t)) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + EPS)
    return [w, m, v]


def check(label, got, want, rtol=RTOL, atol=ATOL):
    for name, a, b in zip("wmv", got, want):
        a = a.double().cpu()
        print(label, name, "max abs err", float((a - b).abs().max()))
        assert torch.allclose(a, b, rtol=rtol, atol=atol), (label, name)


def fresh(shape, seed=40, dtype=torch.float32, zero_state=False):
    """[w, m, v] on the GPU."""
    w = rand(shape, seed, dtype)
    if zero_state:
        return [w.cuda(), torch.zeros_like(w).cuda(),
                torch.zeros_like(w).cuda()]
    return [w.cuda(), rand(shape, seed + 1, dtype).cuda(),
            (rand(shape, seed + 2, dtype).abs() + 0.1).cuda()]


# ---- whole-shard kernels ----

@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", SIZES)
def test_adam_update(hip, n, wd):
    before = fresh(n)
    after = [x.clone() for x in before]
    g = rand(n, 43).cuda()
    hip.adam_update(*after, g, *scalars(3, wd))
    torch.cuda.synchronize()
    check(f"n={n} wd={wd}", after, formula(*before, g, 3, wd))
    assert not torch.equal(after[0], before[0])


@pytest.mark.parametrize("n", [3, 1029])
def test_adam_update_zero_state_first_step(hip, n):
    before = fresh(n, zero_state=True)
    after = [x.clone() for x in before]
    g = rand(n, 43).cuda()
    hip.adam_update(*after, g, *scalars(1, 0.01))
    torch.cuda.synchronize()
    check(f"zero state n={n}", after, formula(*before, g, 1, 0.01))
    # m/sqrt(v) is the sign of g on the first step
    want = before[0] * (1 - LR * 0.01) - LR * torch.sign(g)
    assert torch.allclose(after[0], want, rtol=1e-5, atol=1e-5)


def test_adam_update_zero_gradient_zero_state(hip):
    before = fresh(1029, zero_state=True)
    after = [x.clone() for x in before]
    hip.adam_update(*after, torch.zeros(1029, device="cuda"), *scalars(1))
    torch.cuda.synchronize()
    assert torch.isfinite(after[0]).all()
    for a, b in zip(after, before):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", SIZES)
def test_adam_copy_update(hip, n):
    plain, fused = fresh(n), fresh(n)
    g = rand(n, 43).cuda()
    out = torch.full((n,), float("nan"), device="cuda")
    hip.adam_update(*plain, g, *scalars(3, 0.01))
    hip.adam_copy_update(*fused, g, out, *scalars(3, 0.01))
    torch.cuda.synchronize()
    assert torch.equal(out, fused[0])
    for a, b, c in zip(fused, plain, fresh(n)):
        assert torch.equal(a, b)
        assert not torch.equal(a, c)


@pytest.mark.parametrize("n", [1, 1029])
def test_adam_update_float64(hip, n):
    before = fresh(n, dtype=torch.float64)
    after = [x.clone() for x in before]
    g = rand(n, 43, torch.float64).cuda()
    hip.adam_update(*after, g, *scalars(3, 0.01))
    torch.cuda.synchronize()
    # atol: a few fp64 roundings (1e-16) at |w| ~ 1, for results near zero
    check(f"f64 n={n}", after, formula(*before, g, 3, 0.01), rtol=1e-12,
          atol=1e-14)
    assert not torch.equal(after[0], before[0])


def test_argument_checks(hip):
    w, m, v = fresh(8)
    g = rand(8, 43).cuda()
    with pytest.raises(RuntimeError, match="size mismatch"):
        hip.adam_update(w, m, v[:4].contiguous(), g, *scalars(1))
    with pytest.raises(RuntimeError, match="must be on GPU"):
        hip.adam_update(w, m, v, g.cpu(), *scalars(1))
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        i = torch.zeros(8, dtype=torch.int32, device="cuda")
        hip.adam_update(i, i, i, i, *scalars(1))
    with pytest.raises(RuntimeError, match="must be fp32"):
        hip.adam_copy_update(w, m, v, g, g.double(), *scalars(1))
    rows = torch.arange(2, device="cuda")
    with pytest.raises(RuntimeError, match="v shape mismatch"):
        hip.row_adam_update(w.view(2, 4), m.view(2, 4), v.view(4, 2), rows,
                            g.view(2, 4), *scalars(1))


# ---- keyed kernel ----

@functools.lru_cache(maxsize=None)
def occurrences():
    """N row ids in [0, R), on the host: row 0, row R-1, one row 40 times,
    20 pairs and 175 singletons, shuffled."""
    g = torch.Generator(device="cpu").manual_seed(1234)
    hot = 137
    pool = [r for r in range(1, R - 1) if r != hot]
    pick = torch.randperm(len(pool), generator=g)[:195].tolist()
    pairs = [pool[p] for p in pick[:20]]
    singles = [pool[p] for p in pick[20:]]
    ids = torch.tensor([0, R - 1] + [hot] * 40 + pairs * 2 + singles)
    assert ids.numel() == N and int(ids.min()) == 0 and int(ids.max()) == R - 1
    return ids[torch.randperm(N, generator=g)]


def row_sums(ids, vals):
    """{row: fp32 sum of its value rows in occurrence order}, an explicit
    loop on the host."""
    sums = {}
    for k, r in enumerate(ids.tolist()):
        sums[r] = sums[r] + vals[k] if r in sums else vals[k].clone()
    return sums


def call(hip, tensors, rows, vals, perm=None, t=3, wd=0.01):
    hip.row_adam_update(*tensors, rows, vals, *scalars(t, wd), perm)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def keyed_case(cols):
    """One sorted+perm call of the binding on the shared occurrence list;
    returns (before, after, touched rows, per-row sums [touched, cols])."""
    from multiverso_amd import ops
    hip = ops.module(required=True)
    ids = occurrences()
    vals = rand((N, cols), 50)
    sums = row_sums(ids, vals)
    touched = torch.tensor(sorted(sums))
    g = torch.stack([sums[r] for r in touched.tolist()])
    before = fresh((R, cols))
    after = [t.clone() for t in before]
    sids, perm = torch.sort(ids.cuda(), stable=True)
    call(hip, after, sids, vals.cuda(), perm)
    return before, after, touched.cuda(), g


@pytest.mark.parametrize("cols", COLS)
def test_row_binding_vs_formula(cols):
    before, after, touched, g = keyed_case(cols)
    want = formula(*[x[touched] for x in before], g, 3, 0.01)
    check(f"keyed cols={cols}", [x[touched] for x in after], want)


@pytest.mark.parametrize("cols", COLS)
def test_row_untouched_rows(cols):
    before, after, touched, _ = keyed_case(cols)
    rest = torch.ones(R, dtype=torch.bool, device="cuda")
    rest[touched] = False
    assert int(rest.sum()) == R - touched.numel() > 0
    for b, a in zip(before, after):
        assert torch.equal(a[rest], b[rest])     # not decayed either
        assert not torch.equal(a[touched], b[touched])


@pytest.mark.parametrize("cols", COLS)
def test_row_perm_none_on_unique_unsorted_ids(hip, cols):
    g = torch.Generator(device="cpu").manual_seed(77)
    ids = torch.randperm(R, generator=g)[:101].cuda()
    vals = rand((101, cols), 51).cuda()
    plain, sorted_ = fresh((R, cols)), fresh((R, cols))
    call(hip, plain, ids, vals)
    sids, perm = torch.sort(ids, stable=True)
    call(hip, sorted_, sids, vals, perm)
    for a, b, c in zip(plain, sorted_, fresh((R, cols))):
        assert torch.equal(a, b)
        assert not torch.equal(a, c)


@pytest.mark.parametrize("cols", COLS)
def test_row_reproducible(hip, cols):
    _, first, _, _ = keyed_case(cols)
    again = fresh((R, cols))
    sids, perm = torch.sort(occurrences().cuda(), stable=True)
    call(hip, again, sids, rand((N, cols), 50).cuda(), perm)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_row_empty_batch(hip):
    tensors = fresh((R, 8))
    rows = torch.empty(0, dtype=torch.int64, device="cuda")
    vals = torch.empty(0, 8, device="cuda")
    call(hip, tensors, rows, vals)
    call(hip, tensors, rows, vals, rows.clone())
    for a, b in zip(tensors, fresh((R, 8))):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cols", COLS)
def test_row_all_rows_equals_whole_table_kernel(hip, cols):
    delta = rand((R, cols), 52).cuda()
    keyed, whole = fresh((R, cols)), fresh((R, cols))
    call(hip, keyed, torch.arange(R, device="cuda"), delta)
    hip.adam_update(*[t.view(-1) for t in whole], delta.view(-1),
                    *scalars(3, 0.01))
    torch.cuda.synchronize()
    # every multiply-add of AdamOp is an explicit fma, so the v4f body, the
    # scalar tail and the row kernel round alike
    for a, b, c in zip(keyed, whole, fresh((R, cols))):
        assert torch.equal(a, b)
        assert not torch.equal(a, c)


# ---- table level ----

def test_table_single_process():
    import multiverso_amd as mv
    mv.init(sync=True)
    try:
        wd = 0.01
        opt = mv.AddOption.adam(lr=LR, beta1=B1, beta2=B2, weight_decay=wd)
        t = mv.MatrixTable(64, 16, updater_type="adam")
        assert t.shard.is_cuda
        state = [torch.zeros(64, 16, dtype=torch.float64) for _ in range(3)]
        count = [0]

        def step(ids, vals):
            """One update of the shard: a shared t for every row named."""
            count[0] += 1
            for r, s in row_sums(torch.tensor(ids), vals).items():
                new = formula(*[x[r] for x in state], s, count[0], wd)
                for x, y in zip(state, new):
                    x[r] = y

        def check_table(label, got_w=None):
            if got_w is None:
                got_w = t.get_rows(list(range(64)))
            u = t.updater
            assert u.step == count[0]
            check(label, [got_w, u.exp_avg.view(64, 16),
                          u.exp_avg_sq.view(64, 16)], state)

        ids = [5, 63, 5, 0, 17, 5, 17]
        vals = rand((len(ids), 16), 60)
        t.add_rows(ids, vals.cuda(), option=opt)
        step(ids, vals)
        check_table("keyed")
        # a deferred whole-table Add lands (and counts) before the keyed one
        delta = rand((64, 16), 61)
        t.add(delta.cuda(), option=opt)
        assert t.updater.step == 1
        step(list(range(64)), delta)
        vals = rand((len(ids), 16), 62)
        t.add_rows(ids, vals.cuda(), option=opt)
        step(ids, vals)
        check_table("deferred whole + keyed")
        uniq = [40, 3, 22, 63, 0]
        vals = rand((len(uniq), 16), 63)
        t.add_rows(uniq, vals.cuda(), option=opt, assume_unique=True)
        step(uniq, vals)
        check_table("assume_unique")
        # the deterministic flag pre-sums duplicates; same one step
        mv.set_flag("deterministic", True)
        try:
            vals = rand((len(ids), 16), 64)
            t.add_rows(ids, vals.cuda(), option=opt)
        finally:
            mv.set_flag("deterministic", False)
        step(ids, vals)
        check_table("deterministic")
        # Add immediately followed by get(): the fused update+copy kernel
        delta = rand((64, 16), 65)
        t.add(delta.cuda(), option=opt)
        got = t.get()
        step(list(range(64)), delta)
        assert count[0] == 6
        check_table("fused add+get", got)
        assert torch.equal(got, t.shard)
        # an empty keyed Add is no update
        t.add_rows([], torch.zeros(0, 16, device="cuda"), option=opt)
        assert t.updater.step == 6
    finally:
        mv.set_flag("sync", False)
        mv.shutdown()


def _async_adam_gpu(rank, world):
    import multiverso_amd as mv
    mv.init()   # async mode; both ranks map cuda:0
    assert mv.Zoo.get().async_engine is not None
    t = mv.MatrixTable(12, 4, updater_type="adam")
    assert t.shard.is_cuda
    t.add_rows([3], torch.ones(1, 4), option=mv.AddOption.adam(lr=0.1))
    mv.barrier()
    got = t.get().cpu()
    state = [torch.zeros(4, dtype=torch.float64) for _ in range(3)]
    for step in (1, 2):   # two sequential steps with g = 1
        state = formula(*state, torch.ones(4), step, lr=0.1)
    want = torch.zeros(12, 4, dtype=torch.float64)
    want[3] = state[0]
    assert torch.allclose(got.double(), want, rtol=RTOL, atol=ATOL), (rank,
                                                                      got)
    assert abs(float(got[3, 0]) + 0.2) < 1e-6
    mv.shutdown()


def test_async_engine_shared_gpu():
    run_dist(_async_adam_gpu, 2, gpu_share=True)
