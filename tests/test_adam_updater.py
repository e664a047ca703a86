"""The "adam" updater, CPU tier: whole-table and row-keyed Add against torch's
own optimizers (Adam, AdamW, SparseAdam) on a CPU parameter, the shard-wide
step counter, the AddOption envelope and both two-rank planes.

Tolerance on w: rtol 1e-5, atol 1e-6, the project's dcasgd pair. The table
multiplies sqrt(v) by a host-computed 1/sqrt(1-b2^t) where torch divides by
sqrt(1-b2^t); at |w| ~ 1 over 5 steps that differs by a few fp32 ulps
(3e-7 absolute at most in a probe of this formula against the three
optimizers)."""

import pytest
import torch

import multiverso_amd as mv
from multiverso_amd.updaters import AdamUpdater

from conftest import run_dist

RTOL, ATOL = 1e-5, 1e-6
IDS = [5, 63, 5, 0, 17, 5, 17]


@pytest.fixture()
def env():
    mv.init()
    yield
    mv.shutdown()


def rand(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=dtype)


def adam_ref(w, m, v, g, t, lr=1e-3, b1=0.9, b2=0.999, wd=0.0, eps=1e-8):
    """One step of the issue's formula, out of place, in the dtype given
    (the oracles below pass float64)."""
    w = w * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    w = w - (lr / (1 - b1 ** t)) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    return w, m, v


def close(got, want):
    err = (got.double() - want.double()).abs().max()
    print("max abs err", float(err))
    return torch.allclose(got.double(), want.double(), rtol=RTOL, atol=ATOL)


def make_table(kind):
    if kind == "array":
        return mv.ArrayTable(37, updater_type="adam"), (37,)
    return mv.MatrixTable(9, 4, updater_type="adam"), (9, 4)


# (table option, torch optimizer class, its keyword arguments)
WHOLE = {
    "adam_defaults_option_none": (None, torch.optim.Adam, {}),
    "adam_defaults_explicit": (mv.AddOption.adam(), torch.optim.Adam, {}),
    "adam_custom": (mv.AddOption.adam(lr=0.01, beta1=0.8, beta2=0.99),
                    torch.optim.Adam, dict(lr=0.01, betas=(0.8, 0.99))),
    "adamw": (mv.AddOption.adam(lr=0.01, weight_decay=0.01),
              torch.optim.AdamW, dict(lr=0.01, weight_decay=0.01)),
    "adamw_defaults_lr": (mv.AddOption.adam(weight_decay=0.01),
                          torch.optim.AdamW, dict(weight_decay=0.01)),
}


@pytest.mark.parametrize("case", sorted(WHOLE))
@pytest.mark.parametrize("kind", ["array", "matrix"])
def test_whole_table_vs_torch_optim(env, kind, case):
    option, opt_cls, kw = WHOLE[case]
    t, shape = make_table(kind)
    w0 = rand(shape, 1)
    t.shard.copy_(w0)
    p = torch.nn.Parameter(w0.clone())
    opt = opt_cls([p], eps=AdamUpdater.EPS, amsgrad=False, **kw)
    for k in range(5):
        g = rand(shape, 10 + k)
        t.add(g, option=option)
        p.grad = g.clone()
        opt.step()
    got = t.get()
    assert not torch.allclose(got, w0, rtol=0, atol=1e-4)
    assert close(got.view(shape), p.detach())
    assert t.updater.step == 5


def test_option_none_is_adam_defaults(env):
    a, shape = make_table("matrix")
    b, _ = make_table("matrix")
    for k in range(3):
        g = rand(shape, 20 + k)
        a.add(g)
        b.add(g, option=mv.AddOption.adam())
    assert torch.equal(a.get(), b.get())
    assert torch.equal(a.updater.exp_avg_sq, b.updater.exp_avg_sq)
    a.add_rows([2, 2, 7], rand((3, 4), 24))
    b.add_rows([2, 2, 7], rand((3, 4), 24), option=mv.AddOption.adam())
    assert torch.equal(a.get(), b.get())
    # not the AddOption() field defaults (lr .01, b1 0, b2 .1, wd .1)
    c, _ = make_table("matrix")
    c.add(rand(shape, 20), option=mv.AddOption())
    d, _ = make_table("matrix")
    d.add(rand(shape, 20))
    assert not torch.allclose(c.get(), d.get(), rtol=0, atol=1e-3)


def test_keyed_vs_sparse_adam(env):
    R, C = 64, 7
    t = mv.MatrixTable(R, C, updater_type="adam")
    w0 = rand((R, C), 2)
    t.shard.copy_(w0)
    p = torch.nn.Parameter(w0.clone())
    lr, b1, b2 = 0.01, 0.9, 0.999
    opt = torch.optim.SparseAdam([p], lr=lr, betas=(b1, b2),
                                 eps=AdamUpdater.EPS)
    option = mv.AddOption.adam(lr=lr, beta1=b1, beta2=b2)
    for k in range(4):
        vals = rand((len(IDS), C), 30 + k)
        t.add_rows(IDS, vals, option=option)
        p.grad = torch.sparse_coo_tensor(torch.tensor([IDS]), vals, (R, C))
        opt.step()
    got = t.get()
    assert close(got, p.detach())
    touched = sorted(set(IDS))
    rest = torch.ones(R, dtype=torch.bool)
    rest[touched] = False
    assert not torch.allclose(got[touched], w0[touched], rtol=0, atol=1e-3)
    assert torch.equal(got[rest], w0[rest])
    m = t.updater.exp_avg.view(R, C)
    v = t.updater.exp_avg_sq.view(R, C)
    assert torch.equal(m[rest], torch.zeros(int(rest.sum()), C))
    assert torch.equal(v[rest], torch.zeros(int(rest.sum()), C))
    assert (v[touched] > 0).all()
    assert t.updater.step == 4


def test_keyed_untouched_rows_are_not_decayed(env):
    t = mv.MatrixTable(8, 3, updater_type="adam")
    w0 = rand((8, 3), 3)
    t.shard.copy_(w0)
    t.add_rows([1, 6], rand((2, 3), 4),
               option=mv.AddOption.adam(lr=0.1, weight_decay=0.5))
    got = t.get()
    rest = [0, 2, 3, 4, 5, 7]
    assert torch.equal(got[rest], w0[rest])
    # the named rows were decayed: w*(1 - .05) -+ .1 (first step: m/sqrt(v)
    # is the sign of g)
    g = rand((2, 3), 4)
    want = w0[[1, 6]] * 0.95 - 0.1 * torch.sign(g)
    assert torch.allclose(got[[1, 6]], want, rtol=1e-5, atol=1e-5)


def row_sums(ids, vals):
    sums = {}
    for k, r in enumerate(ids):
        sums[r] = sums[r] + vals[k] if r in sums else vals[k].clone()
    return sums


def test_mixed_whole_and_keyed_share_one_step_count(env):
    R, C = 9, 4
    hp = dict(lr=0.01, b1=0.8, b2=0.99, wd=0.01)
    option = mv.AddOption.adam(lr=0.01, beta1=0.8, beta2=0.99,
                               weight_decay=0.01)
    t = mv.MatrixTable(R, C, updater_type="adam")
    w = rand((R, C), 5).double()
    t.shard.copy_(w.float())
    w = w.float().double()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    ids = [7, 2, 7]
    seq = [("whole", rand((R, C), 40)), ("keyed", rand((len(ids), C), 41)),
           ("whole", rand((R, C), 42))]
    for step, (kind, g) in enumerate(seq, start=1):
        if kind == "whole":
            t.add(g, option=option)
            w, m, v = adam_ref(w, m, v, g.double(), step, **hp)
        else:
            t.add_rows(ids, g, option=option)
            for r, s in row_sums(ids, g).items():
                w[r], m[r], v[r] = adam_ref(w[r], m[r], v[r], s.double(),
                                            step, **hp)
        assert t.updater.step == step
    assert close(t.get(), w)
    assert close(t.updater.exp_avg.view(R, C), m)
    assert close(t.updater.exp_avg_sq.view(R, C), v)


def test_step_counter(env):
    t = mv.MatrixTable(6, 2, updater_type="adam")
    assert t.updater.step == 0
    t.add(torch.ones(6, 2))
    assert t.updater.step == 1
    t.add_rows([1, 1, 4], torch.ones(3, 2))
    assert t.updater.step == 2
    before = (t.get().clone(), t.updater.exp_avg.clone(),
              t.updater.exp_avg_sq.clone())
    t.add_rows([], torch.zeros(0, 2))
    t.add_rows([], torch.zeros(0, 2), option=mv.AddOption.adam(lr=0.5))
    assert t.updater.step == 2
    after = (t.get(), t.updater.exp_avg, t.updater.exp_avg_sq)
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    t.add(torch.ones(6, 2)).wait()
    assert t.updater.step == 3
    a = mv.ArrayTable(5, updater_type="adam")
    a.add(torch.ones(5))
    a.add(torch.ones(5))
    assert a.updater.step == 2


def test_deterministic_flag_and_assume_unique(env):
    a = mv.MatrixTable(6, 2, updater_type="adam")
    b = mv.MatrixTable(6, 2, updater_type="adam")
    # multiples of 1/8: the pre-sum is exact in any order
    vals = torch.tensor([[0.5, 1.25], [2.0, -0.125], [1.5, 0.25]])
    mv.set_flag("deterministic", True)
    try:
        a.add_rows([4, 1, 4], vals)
    finally:
        mv.set_flag("deterministic", False)
    b.add_rows([4, 1], torch.stack([vals[0] + vals[2], vals[1]]),
               assume_unique=True)
    assert torch.equal(a.get(), b.get())
    assert a.get()[4].abs().sum() > 0
    assert a.updater.step == b.updater.step == 1


def test_zero_gradient_on_fresh_table(env):
    t = mv.MatrixTable(5, 3, updater_type="adam")
    w0 = rand((5, 3), 6)
    t.shard.copy_(w0)
    t.add(torch.zeros(5, 3))            # v = 0: the denominator is eps
    t.add_rows([2, 2], torch.zeros(2, 3))
    got = t.get()
    assert torch.isfinite(got).all()
    assert torch.equal(got, w0)
    assert torch.equal(t.updater.exp_avg, torch.zeros(15))
    a = mv.ArrayTable(4, updater_type="adam")
    a.add(torch.zeros(4))
    assert torch.equal(a.get(), torch.zeros(4))


def test_float64_table(env):
    t = mv.MatrixTable(6, 3, dtype=torch.float64, updater_type="adam")
    w = rand((6, 3), 7, torch.float64)
    t.shard.copy_(w)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    option = mv.AddOption.adam(lr=0.5, beta1=0.75, beta2=0.875,
                               weight_decay=0.25)   # exact in the envelope
    hp = dict(lr=0.5, b1=0.75, b2=0.875, wd=0.25)
    g = rand((6, 3), 8, torch.float64)
    t.add(g, option=option)
    w, m, v = adam_ref(w, m, v, g, 1, **hp)
    ids = [0, 4, 4]
    vals = rand((3, 3), 9, torch.float64)
    t.add_rows(ids, vals, option=option)
    for r, s in row_sums(ids, vals).items():
        w[r], m[r], v[r] = adam_ref(w[r], m[r], v[r], s, 2, **hp)
    got = t.get()
    assert got.dtype == torch.float64
    assert torch.allclose(got, w, rtol=1e-12, atol=1e-12)
    assert torch.allclose(t.updater.exp_avg_sq.view(6, 3), v, rtol=1e-12,
                          atol=1e-12)


def test_sparse_matrix_table(env):
    t = mv.SparseMatrixTable(8, 3, updater_type="adam")
    option = mv.AddOption.adam(lr=0.1)
    vals = torch.tensor([[1.0, -2.0, 0.5], [3.0, 3.0, 3.0], [1.0, 1.0, -4.0]])
    t.add_rows([6, 1, 6], vals, option=option)
    # first step from zero state: m/sqrt(v) is the sign of the row's sum
    want = torch.zeros(8, 3)
    want[1] = -0.1
    want[6] = -0.1 * torch.sign(vals[0] + vals[2])
    out = torch.zeros(8, 3)
    t.get_into(out)
    assert torch.allclose(out, want, rtol=RTOL, atol=ATOL)
    assert torch.allclose(t.get_rows([6, 1, 0]), want[[6, 1, 0]], rtol=RTOL,
                          atol=ATOL)
    assert t.updater.step == 1


def test_updater_type_flag(env):
    mv.set_flag("updater_type", "adam")
    try:
        t = mv.ArrayTable(4)
    finally:
        mv.set_flag("updater_type", "default")
    assert isinstance(t.updater, AdamUpdater)
    t.add(torch.ones(4))
    assert torch.allclose(t.get(), torch.full((4,), -1e-3), rtol=RTOL,
                          atol=ATOL)


def test_envelope_round_trip():
    o = mv.AddOption.adam(lr=0.25, beta1=0.5, beta2=0.875, weight_decay=0.125,
                          worker_id=3)
    assert (o.learning_rate, o.momentum, o.rho, o.lambda_, o.worker_id) == \
        (0.25, 0.5, 0.875, 0.125, 3)
    b = o.to_bytes()
    assert len(b) == 20
    r = mv.AddOption.from_bytes(b)
    assert (r.worker_id, r.momentum, r.learning_rate, r.rho, r.lambda_) == \
        (3, 0.5, 0.25, 0.875, 0.125)
    d = mv.AddOption.adam()
    assert (d.learning_rate, d.momentum, d.rho, d.lambda_, d.worker_id) == \
        (1e-3, 0.9, 0.999, 0.0, 0)
    assert AdamUpdater.EPS == 1e-8


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_integer_tables_raise_at_construction(env, dtype):
    name = str(dtype).replace("torch.", "")
    with pytest.raises(TypeError, match=name):
        mv.ArrayTable(8, dtype=dtype, updater_type="adam")
    with pytest.raises(TypeError, match=name):
        mv.MatrixTable(8, 2, dtype=dtype, updater_type="adam")


# ---- two ranks (worker functions are top-level for spawn pickling) ----

def _sync_adam(rank, world):
    import multiverso_amd as mv
    mv.init(sync=True)
    R, C = 12, 4
    t = mv.MatrixTable(R, C, updater_type="adam")
    option = mv.AddOption.adam(lr=0.01, beta1=0.8, beta2=0.99,
                               weight_decay=0.01)
    hp = dict(lr=0.01, b1=0.8, b2=0.99, wd=0.01)
    # the oracle: both shards (rows 0-5, 6-11), each with its own t
    w = torch.zeros(R, C, dtype=torch.float64)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    steps = [0, 0]

    def apply(sums):
        """sums: {row: summed delta}; a shard that gets rows counts one."""
        for s in (0, 1):
            mine = {r: g for r, g in sums.items() if r // 6 == s}
            if not mine:
                continue
            steps[s] += 1
            for r, g in mine.items():
                w[r], m[r], v[r] = adam_ref(w[r], m[r], v[r], g.double(),
                                            steps[s], **hp)

    def both(seed):   # what rank 0 and rank 1 send
        return rand((R, C), seed), rand((R, C), seed + 1)

    d0, d1 = both(50)
    t.add((d0, d1)[rank], option=option)
    apply({r: d0[r] + d1[r] for r in range(R)})
    # keyed, both shards: rank 0 names 3, 9, 3 and rank 1 names 9, 7
    ids = ([3, 9, 3], [9, 7])
    vals = (rand((3, C), 60), rand((2, C), 61))
    t.add_rows(ids[rank], vals[rank], option=option)
    apply({3: vals[0][0] + vals[0][2], 9: vals[0][1] + vals[1][0],
           7: vals[1][1]})
    # keyed, shard 0 only: shard 1 applies nothing and keeps its t
    ids = ([1, 4], [4])
    vals = (rand((2, C), 62), rand((1, C), 63))
    t.add_rows(ids[rank], vals[rank], option=option)
    apply({1: vals[0][0], 4: vals[0][1] + vals[1][0]})
    assert steps == [3, 2]
    assert t.updater.step == steps[rank], (rank, t.updater.step)
    d0, d1 = both(70)
    t.add((d0, d1)[rank], option=option)
    apply({r: d0[r] + d1[r] for r in range(R)})
    assert t.updater.step == steps[rank] == 4 - rank
    got = t.get()
    assert close(got, w), (rank, got, w)
    mv.shutdown()


def test_two_ranks_sync_plane():
    run_dist(_sync_adam, 2)


def _async_adam(rank, world):
    import multiverso_amd as mv
    mv.init()
    assert mv.Zoo.get().async_engine is not None
    t = mv.MatrixTable(12, 4, updater_type="adam")
    t.add_rows([3], torch.ones(1, 4), option=mv.AddOption.adam(lr=0.1))
    mv.barrier()
    got = t.get()
    w = torch.zeros(4, dtype=torch.float64)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    for step in (1, 2):
        w, m, v = adam_ref(w, m, v, torch.ones(4, dtype=torch.float64), step,
                           lr=0.1)
    want = torch.zeros(12, 4, dtype=torch.float64)
    want[3] = w          # -0.2 up to eps
    assert close(got, want), (rank, got)
    assert abs(float(got[3, 0]) + 0.2) < 1e-6
    rest = [r for r in range(12) if r != 3]
    assert torch.equal(got[rest], torch.zeros(11, 4))
    mv.shutdown()


def test_two_ranks_async_plane():
    run_dist(_async_adam, 2)
