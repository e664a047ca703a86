"""GPU tests of the keyed stateful updaters: the k_row_update kernel behind
row_momentum_update / row_dcasgd_update / row_dcasgda_update, and add_rows
on momentum / dcasgd / dcasgda tables that live on the GPU.

Tolerances are those of test_gpu_kernels.py::test_momentum / test_dcasgd /
test_dcasgda: the same op bodies against the same torch formulas."""

import functools

import pytest
import torch

from conftest import run_dist

pytestmark = pytest.mark.gpu

R, N = 300, 257
# scalar with one lane per row, scalar odd, v4f with two vectors per row,
# v4f with a row spanning half a wave
COLS = [1, 7, 8, 128]
NAMES = ["momentum", "dcasgd", "dcasgda"]
STATE = {"momentum": ("m",), "dcasgd": ("bak",), "dcasgda": ("bak", "msq")}
ARGS = {"momentum": (0.9,), "dcasgd": (0.1, 0.04),
        "dcasgda": (0.1, 0.04, 0.95, 1e-7)}
# (rtol, atol) for data and then each state tensor
TOL = {"momentum": [(1e-6, 1e-5), (1e-6, 1e-6)],
       "dcasgd": [(1e-5, 1e-6), (1e-5, 1e-6)],
       "dcasgda": [(1e-4, 1e-5), (1e-4, 1e-5), (1e-5, 1e-7)]}


@pytest.fixture(scope="module")
def hip():
    from multiverso_amd import ops
    return ops.module(required=True)


def rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g)


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


def fresh(name, cols, seed=40):
    """[data, state...] on the GPU, [R, cols] each."""
    ts = [rand((R, cols), seed)]
    for k, s in enumerate(STATE[name]):
        t = rand((R, cols), seed + 1 + k)
        ts.append(t if s == "bak" else t.abs())
    return [t.cuda() for t in ts]


def formula(name, data, state, g):
    """New [data, state...] by the torch formulas of test_gpu_kernels.py."""
    if name == "momentum":
        mu, = ARGS[name]
        m = mu * state[0] + (1 - mu) * g
        return [data - m, m]
    if name == "dcasgd":
        lr, lam = ARGS[name]
        w = data - lr * (g + lam * g * g * (data - state[0]))
        return [w, w]
    lr, lam, rho, eps = ARGS[name]
    bak, msq = state
    m = rho * msq + (1 - rho) * g * g
    lam_t = lam / torch.sqrt(m + eps)
    w = data - lr * (g + lam_t * g * g * (data - bak))
    return [w, w, m]


def call(hip, name, tensors, rows, vals, perm=None):
    getattr(hip, f"row_{name}_update")(*tensors, rows, vals, *ARGS[name],
                                       perm)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def keyed_case(name, cols):
    """One sorted+perm call of the binding on the shared occurrence list;
    returns (before, after, touched rows, per-row sums [touched, cols])."""
    from multiverso_amd import ops
    hip = ops.module(required=True)
    ids = occurrences()
    vals = rand((N, cols), 50)
    sums = row_sums(ids, vals)
    touched = torch.tensor(sorted(sums))
    g = torch.stack([sums[r] for r in touched.tolist()]).cuda()
    before = fresh(name, cols)
    after = [t.clone() for t in before]
    sids, perm = torch.sort(ids.cuda(), stable=True)
    call(hip, name, after, sids, vals.cuda(), perm)
    return before, after, touched.cuda(), g


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("name", NAMES)
def test_binding_vs_formula(name, cols):
    before, after, touched, g = keyed_case(name, cols)
    want = formula(name, before[0][touched], [s[touched] for s in before[1:]],
                   g)
    for got, ref, (rtol, atol) in zip(after, want, TOL[name]):
        err = (got[touched] - ref).abs()
        print(name, cols, "max abs err", float(err.max()))
        assert torch.allclose(got[touched], ref, rtol=rtol, atol=atol)
    if name != "momentum":
        assert torch.equal(after[1][touched], after[0][touched])


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("name", NAMES)
def test_untouched_rows(name, cols):
    before, after, touched, _ = keyed_case(name, cols)
    rest = torch.ones(R, dtype=torch.bool, device="cuda")
    rest[touched] = False
    assert int(rest.sum()) == R - touched.numel() > 0
    for b, a in zip(before, after):
        assert torch.equal(a[rest], b[rest])
        assert not torch.equal(a[touched], b[touched])


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("name", NAMES)
def test_perm_none_on_unique_unsorted_ids(hip, name, cols):
    g = torch.Generator(device="cpu").manual_seed(77)
    ids = torch.randperm(R, generator=g)[:101].cuda()
    vals = rand((101, cols), 51).cuda()
    plain, sorted_ = fresh(name, cols), fresh(name, cols)
    call(hip, name, plain, ids, vals)
    sids, perm = torch.sort(ids, stable=True)
    call(hip, name, sorted_, sids, vals, perm)
    for a, b, c in zip(plain, sorted_, fresh(name, cols)):
        assert torch.equal(a, b)
        assert not torch.equal(a, c)


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("name", NAMES)
def test_reproducible(hip, name, cols):
    _, first, _, _ = keyed_case(name, cols)
    again = fresh(name, cols)
    sids, perm = torch.sort(occurrences().cuda(), stable=True)
    call(hip, name, again, sids, rand((N, cols), 50).cuda(), perm)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch(hip, name):
    tensors = fresh(name, 8)
    rows = torch.empty(0, dtype=torch.int64, device="cuda")
    vals = torch.empty(0, 8, device="cuda")
    call(hip, name, tensors, rows, vals)
    call(hip, name, tensors, rows, vals, rows.clone())
    for a, b in zip(tensors, fresh(name, 8)):
        assert torch.equal(a, b)


# the updaters whose keyed entry points are not row_X_update
STATE.update({"default": (), "sgd": (), "adagrad": ("gsq",)})
ARGS.update({"default": (), "sgd": (), "adagrad": (0.1, 0.04, 1e-6)})


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("name", NAMES + ["default", "sgd", "adagrad"])
def test_all_rows_equals_whole_table_kernel(hip, name, cols):
    delta = rand((R, cols), 52).cuda()
    keyed, whole = fresh(name, cols), fresh(name, cols)
    rows = torch.arange(R, device="cuda")
    whole_fn = getattr(hip, "add_inplace" if name == "default"
                       else name + "_update")
    if name in ("default", "sgd"):
        hip.row_scatter_add(keyed[0], rows, delta,
                            1.0 if name == "default" else -1.0)
    elif name == "adagrad":
        # assume_unique, as perm=None is for the others. The atomic form
        # (assume_unique=False) was measured NOT to round like the
        # whole-table kernel even on distinct rows: max abs difference
        # 2.4e-7 on the weights and 1.2e-4 on G at these shapes
        hip.row_scatter_adagrad(*keyed, rows, delta, *ARGS[name], True)
    else:
        call(hip, name, keyed, rows, delta)
    whole_fn(*[t.view(-1) for t in whole], delta.view(-1), *ARGS[name])
    torch.cuda.synchronize()
    # MomentumOp's fma is explicit; the DC-ASGD bodies were measured to
    # round alike in both kernels too, at every width here
    for a, b in zip(keyed, whole):
        assert torch.equal(a, b)


def test_table_single_process():
    import multiverso_amd as mv
    mv.init(sync=True)
    try:
        mu = 0.5
        opt = mv.AddOption(momentum=mu)
        t = mv.MatrixTable(64, 16, updater_type="momentum")
        assert t.shard.is_cuda
        w, m = torch.zeros(64, 16), torch.zeros(64, 16)

        def step(ids, vals):
            for r, s in row_sums(torch.tensor(ids), vals).items():
                m[r] = mu * m[r] + (1 - mu) * s
                w[r] = w[r] - m[r]

        def check():
            got = t.get_rows(list(range(64))).cpu()
            assert torch.allclose(got, w, rtol=1e-6, atol=1e-5)
            sg = t.updater.smooth_gradient.view(64, 16).cpu()
            assert torch.allclose(sg, m, rtol=1e-6, atol=1e-6)

        ids = [5, 63, 5, 0, 17, 5, 17]
        vals = rand((len(ids), 16), 60)
        t.add_rows(ids, vals.cuda(), option=opt)
        step(ids, vals)
        check()
        # a deferred whole-table Add lands before the keyed one
        delta = rand((64, 16), 61)
        t.add(delta.cuda(), option=opt)
        step(list(range(64)), delta)
        vals = rand((len(ids), 16), 62)
        t.add_rows(ids, vals.cuda(), option=opt)
        step(ids, vals)
        check()
        uniq = [40, 3, 22, 63, 0]
        vals = rand((len(uniq), 16), 63)
        t.add_rows(uniq, vals.cuda(), option=opt, assume_unique=True)
        step(uniq, vals)
        check()
        # rows no keyed Add named took the whole-table step only
        assert torch.equal(t.updater.smooth_gradient.view(64, 16)[1].cpu(),
                           (1 - mu) * delta[1])
        # the deterministic flag pre-sums duplicates; same one step
        mv.set_flag("deterministic", True)
        try:
            vals = rand((len(ids), 16), 64)
            t.add_rows(ids, vals.cuda(), option=opt)
        finally:
            mv.set_flag("deterministic", False)
        step(ids, vals)
        check()
    finally:
        mv.set_flag("sync", False)
        mv.shutdown()


def _async_momentum_gpu(rank, world):
    import multiverso_amd as mv
    mv.init()   # async mode; both ranks map cuda:0
    assert mv.Zoo.get().async_engine is not None
    t = mv.MatrixTable(12, 4, updater_type="momentum")
    assert t.shard.is_cuda
    t.add_rows([3], torch.ones(1, 4), option=mv.AddOption(momentum=0.5))
    mv.barrier()
    got = t.get().cpu()
    want = torch.zeros(12, 4)
    want[3] = -1.25       # two steps: m = .5, then .75
    assert torch.equal(got, want), (rank, got)
    mv.shutdown()


def test_async_engine_shared_gpu():
    run_dist(_async_momentum_gpu, 2, gpu_share=True)
