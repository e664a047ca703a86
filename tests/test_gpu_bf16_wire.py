"""GPU tests of the bf16 wire format: the kernels that read a bfloat16 delta
or vals and write a bfloat16 Get buffer over an fp32 shard, and the tables
built with ``wire_dtype=torch.bfloat16`` on one GPU.

Oracles. Narrowing: torch's CPU cast ``.to(torch.bfloat16)``, compared on the
int16 views. Updaters: the same binding run on the widened delta
(``delta.float()``, exact). add, sgd, momentum and adam must agree bit for
bit: sgd's product by +-1 is exact, momentum and adam place every fma
explicitly. adagrad, dcasgd and dcasgda leave contraction to the compiler,
which may differ per instantiation, so they keep the tolerances of
tests/test_gpu_kernels.py: rtol 1e-4 / atol 1e-5 on weights, rtol 1e-5 /
atol 1e-6 on state. Every such case prints its max abs difference."""

import pytest
import torch

from conftest import run_dist

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
W_TOL = dict(rtol=1e-4, atol=1e-5)
S_TOL = dict(rtol=1e-5, atol=1e-6)
# tail only, one vector, body plus tail, many blocks
SIZES = [1, 3, 4, 1029, 262147]
R, N = 300, 257
COLS = [1, 7, 8, 128]
# (cols, vals taken from a view one element, 2 bytes, off): the misaligned
# case is cols = 8, which would otherwise take the vector path
COLS_ALIGN = [(c, False) for c in COLS] + [(8, True)]
LR, LAM, RHO = 0.1, 0.5, 0.9


@pytest.fixture(scope="module")
def hip():
    from multiverso_amd import ops
    return ops.module(required=True)


def rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g)


def adam_scalars(t=3, lr=0.01, b1=0.9, b2=0.999, wd=0.01):
    return (b1, b2, lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** -0.5,
            1.0 - lr * wd, 1e-8)


# name -> (state kinds, scalars, exact); "r" state is randn, "p" is positive
UPDATERS = {
    "add": ("", (), True),
    "sgd": ("", (), True),
    "momentum": ("r", (0.9,), True),
    "adagrad": ("p", (LR, 0.1, 1e-6), False),
    "dcasgd": ("r", (LR, LAM), False),
    "dcasgda": ("rp", (LR, LAM, RHO, 1e-7), False),
    "adam": ("rp", adam_scalars(), True),
}


def fresh(name, shape, seed=40):
    """[w, state...] on the GPU."""
    out = [rand(shape, seed)]
    for k, kind in enumerate(UPDATERS[name][0]):
        s = rand(shape, seed + 1 + k)
        out.append(s if kind == "r" else s.abs() + 0.1)
    return [x.cuda() for x in out]


def run_update(hip, name, ws, delta, out=None):
    """The whole-shard binding of `name`; with `out`, its fused Add+Get."""
    scal = UPDATERS[name][1]
    if name in ("add", "sgd"):
        sign = 1.0 if name == "add" else -1.0
        if out is not None:
            hip.sgd_copy_update(ws[0], delta, out, sign)
        elif name == "add":
            hip.add_inplace(ws[0], delta)
        else:
            hip.sgd_update(ws[0], delta)
        return
    if out is None:
        getattr(hip, name + "_update")(*ws, delta, *scal)
    else:
        getattr(hip, name + "_copy_update")(*ws, delta, out, *scal)


def same(label, name, got, want):
    """got == want: bit for bit for the exact updaters, else within the
    weight / state tolerances."""
    exact = UPDATERS[name][2]
    for k, (a, b) in enumerate(zip(got, want)):
        diff = float((a.double() - b.double()).abs().max()) if a.numel() else 0
        print(label, name, "tensor", k, "max abs diff", diff,
              "bit-equal", torch.equal(a, b))
        if exact:
            assert torch.equal(a, b), (label, name, k)
        else:
            tol = W_TOL if k == 0 else S_TOL
            assert torch.allclose(a, b, **tol), (label, name, k, diff)


def narrowed_by_torch(x):
    return x.cpu().to(BF16)


# ---- narrowing ----

EDGES = [0x00000000, 0x80000000, 0x00000001, 0x00007FFF, 0x00008000,
         0x00008001, 0x00018000, 0x3F808000, 0x3F818000, 0x7F7F7FFF,
         0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0x7F800000, 0xFF800000,
         0x7FC00000, 0x7F800001]
N_NAN = 2   # the last two edges


def bit_patterns():
    g = torch.Generator(device="cpu").manual_seed(7)
    u = torch.cat([torch.randint(0, 2 ** 32, (4096,), generator=g),
                   torch.tensor(EDGES)])
    return (u - (u >= 2 ** 31) * 2 ** 32).to(torch.int32).view(torch.float32)


def check_narrowed(got, src):
    """got (bf16) is src (fp32) cast by torch: same bits wherever src is not
    a NaN, a NaN wherever it is."""
    got, src = got.cpu(), src.cpu()
    nan = src.isnan()
    assert int(nan.sum()) >= N_NAN
    assert bool(got[nan].isnan().all())
    want = src.to(BF16)
    assert torch.equal(got[~nan].view(torch.int16),
                       want[~nan].view(torch.int16))


@pytest.mark.parametrize("offset", [0, 1])
def test_nt_copy_narrows_like_torch(hip, offset):
    src = bit_patterns().cuda()
    buf = torch.zeros(src.numel() + 4, dtype=BF16, device="cuda")
    dst = buf[offset:offset + src.numel()]
    hip.nt_copy(dst, src)
    torch.cuda.synchronize()
    check_narrowed(dst, src)
    # nothing written around dst
    assert float(buf[:offset].abs().sum()) == 0
    assert float(buf[offset + src.numel():].abs().sum()) == 0


@pytest.mark.parametrize("offset", [0, 1])
def test_fused_out_narrows_like_torch(hip, offset):
    """sgd_copy_update and adam_copy_update with a bf16 out: out is the
    updated shard cast by torch, on raw bit patterns."""
    pat = bit_patterns()
    n = pat.numel()
    zero = torch.zeros(n, dtype=BF16, device="cuda")
    w = pat.cuda()
    out = torch.zeros(n + 4, dtype=BF16, device="cuda")[offset:offset + n]
    hip.sgd_copy_update(w, zero, out, 1.0)      # w += 0
    torch.cuda.synchronize()
    check_narrowed(out, w)
    keep = ~pat.isnan() & (pat.abs() >= 2.0 ** -126)
    assert torch.equal(w.cpu()[keep], pat[keep])   # the patterns survived
    ws = [pat.cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()]
    out = torch.zeros(n + 4, dtype=BF16, device="cuda")[offset:offset + n]
    hip.adam_copy_update(*ws, zero, out, *adam_scalars(wd=0.0))
    torch.cuda.synchronize()
    check_narrowed(out, ws[0])


# ---- whole-shard updaters ----

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(UPDATERS))
def test_bf16_delta_matches_widened_delta(hip, name, n):
    delta = rand(n, 43).to(BF16).cuda()
    got, want = fresh(name, n), fresh(name, n)
    before = got[0].clone()
    run_update(hip, name, got, delta)
    run_update(hip, name, want, delta.float())
    torch.cuda.synchronize()
    same(f"update n={n}", name, got, want)
    assert not torch.equal(got[0], before)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(UPDATERS))
def test_copy_update_with_bf16_out(hip, name, n):
    delta = rand(n, 43).to(BF16).cuda()
    got, want = fresh(name, n), fresh(name, n)
    out = torch.zeros(n, dtype=BF16, device="cuda")
    run_update(hip, name, got, delta, out)
    run_update(hip, name, want, delta.float())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), narrowed_by_torch(got[0]))
    same(f"copy_update n={n}", name, got, want)
    # a bf16 delta with an fp32 out, and the reverse
    a, b = fresh(name, n), fresh(name, n)
    out32 = torch.zeros(n, device="cuda")
    out16 = torch.zeros(n, dtype=BF16, device="cuda")
    run_update(hip, name, a, delta, out32)
    run_update(hip, name, b, delta.float(), out16)
    torch.cuda.synchronize()
    assert torch.equal(out32, a[0])
    assert torch.equal(out16.cpu(), narrowed_by_torch(b[0]))
    same(f"copy_update mixed n={n}", name, a, b)


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_misaligned_delta_and_out(hip, name):
    """delta = buf[1:] and out = obuf[1:] are 2 bytes off the 8-byte vector
    alignment: the launch goes all-scalar and must give the aligned
    results."""
    n = 1029
    d = rand(n, 43).to(BF16).cuda()
    buf = torch.zeros(n + 1, dtype=BF16, device="cuda")
    buf[1:].copy_(d)
    delta = buf[1:]
    assert delta.data_ptr() % 8 == 2 and delta.is_contiguous()
    obuf = torch.zeros(n + 2, dtype=BF16, device="cuda")
    aligned, off = fresh(name, n), fresh(name, n)
    out = torch.zeros(n, dtype=BF16, device="cuda")
    run_update(hip, name, aligned, d, out)
    run_update(hip, name, off, delta, obuf[1:n + 1])
    torch.cuda.synchronize()
    for a, b in zip(aligned, off):
        assert torch.equal(a, b)
    assert torch.equal(obuf[1:n + 1], out)
    assert float(obuf[0]) == 0 and float(obuf[n + 1]) == 0
    # the plain update too
    aligned, off = fresh(name, n), fresh(name, n)
    run_update(hip, name, aligned, d)
    run_update(hip, name, off, delta)
    torch.cuda.synchronize()
    for a, b in zip(aligned, off):
        assert torch.equal(a, b)


def test_argument_checks(hip):
    w = torch.zeros(8, device="cuda")
    d16 = torch.zeros(8, dtype=BF16, device="cuda")
    w64 = torch.zeros(8, dtype=torch.float64, device="cuda")
    wi = torch.zeros(8, dtype=torch.int32, device="cuda")
    # bf16 only where the shard is fp32
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        hip.sgd_update(w64, d16)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        hip.add_inplace(wi, d16)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        hip.adam_update(w64, w64.clone(), w64.clone(), d16, *adam_scalars())
    # state is never bf16, and fp16 is no wire format
    with pytest.raises(RuntimeError, match="m dtype mismatch"):
        hip.momentum_update(w, d16.clone(), d16, 0.9)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        hip.sgd_update(w, d16.to(torch.float16))
    with pytest.raises(RuntimeError, match="size mismatch"):
        hip.sgd_copy_update(w, d16, d16[:4].contiguous(), 1.0)
    with pytest.raises(RuntimeError, match="must be fp32"):
        hip.nt_copy(d16, d16)


# ---- row kernels ----

def id_lists():
    """(duplicated, unique): N local row ids in [0, R), the first with one
    row listed 40 times, the second all distinct; both shuffled."""
    g = torch.Generator(device="cpu").manual_seed(5)
    perm = torch.randperm(R, generator=g)
    hot, rest = perm[0], perm[1:]
    dup = torch.cat([hot.repeat(40), rest[:N - 40]])
    dup = dup[torch.randperm(N, generator=g)]
    return dup.cuda(), perm[:N].clone().cuda()


def eighths(shape, seed):
    """Multiples of 1/8 in [-2, 2]: bf16 values whose sums of 40 are exact
    in fp32 in any order."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-16, 17, shape, generator=g).float() / 8


def off_by_one(vals16):
    """The same bf16 values in a buffer view 2 bytes off."""
    buf = torch.zeros(vals16.numel() + 1, dtype=BF16, device=vals16.device)
    buf[1:].copy_(vals16.reshape(-1))
    v = buf[1:].view(vals16.shape)
    assert v.data_ptr() % 4 == 2 and v.is_contiguous()
    return v


@pytest.mark.parametrize("cols", COLS)
def test_row_gather_to_bf16(hip, cols):
    dup, _ = id_lists()
    shard = rand((R, cols), 60).cuda()
    got = hip.row_gather(shard, dup, BF16)
    wide = hip.row_gather(shard, dup)
    torch.cuda.synchronize()
    assert got.dtype == BF16 and got.shape == (N, cols)
    assert wide.dtype == torch.float32
    assert torch.equal(got.cpu(), narrowed_by_torch(wide))
    # preallocated, and 2 bytes off
    obuf = torch.zeros(N * cols + 2, dtype=BF16, device="cuda")
    out = obuf[1:N * cols + 1].view(N, cols)
    hip.row_gather_out(out, shard, dup)
    torch.cuda.synchronize()
    assert torch.equal(out, got)
    assert float(obuf[0]) == 0 and float(obuf[-1]) == 0


@pytest.mark.parametrize("assume_unique", [False, True])
@pytest.mark.parametrize("cols,misaligned", COLS_ALIGN)
def test_row_scatter_add_bf16_vals(hip, cols, assume_unique, misaligned):
    dup, uniq = id_lists()
    ids = uniq if assume_unique else dup
    vals = eighths((N, cols), 61)
    v16 = vals.to(BF16).cuda()
    assert torch.equal(v16.float().cpu(), vals)
    if misaligned:
        v16 = off_by_one(v16)
    got, want = eighths((R, cols), 62).cuda(), eighths((R, cols), 62).cuda()
    hip.row_scatter_add(got, ids, v16, -1.0, assume_unique)
    hip.row_scatter_add(want, ids, vals.cuda(), -1.0, assume_unique)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    ref = eighths((R, cols), 62).index_add_(0, ids.cpu(), -vals)
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("assume_unique", [False, True])
@pytest.mark.parametrize("cols", COLS)
def test_row_scatter_adagrad_bf16_vals(hip, cols, assume_unique):
    # distinct ids in both forms: the atomic form's duplicates race by
    # design (hogwild), which no oracle pins down
    _, ids = id_lists()
    v16 = rand((N, cols), 63).to(BF16).cuda()
    got = [rand((R, cols), 64).cuda(), (rand((R, cols), 65).abs() + 0.1).cuda()]
    want = [x.clone() for x in got]
    hip.row_scatter_adagrad(*got, ids, v16, LR, 0.1, 1e-6, assume_unique)
    hip.row_scatter_adagrad(*want, ids, v16.float(), LR, 0.1, 1e-6,
                            assume_unique)
    torch.cuda.synchronize()
    same(f"row adagrad cols={cols} unique={assume_unique}", "adagrad", got,
         want)
    assert not torch.equal(got[0], rand((R, cols), 64).cuda())


@pytest.mark.parametrize("cols", COLS)
def test_row_scatter_adagrad_bf16_duplicates(hip, cols):
    """The atomic form with a real collision: the list with one row 40 times.
    With lr = 1 and values in eighths every g*g is a multiple of 1/64, so G
    is exact in any arrival order: it must equal the fp32-vals call and the
    host sum bit for bit. A row listed once takes one step and keeps the
    weight tolerance. The hot row's 40 steps race by design: each is
    -rho*g*rsq(G_seen + eps) with G0 + g*g <= G_seen <= G_final, so two runs
    differ by at most sum(rho*|g|*(rsq(G0 + g*g + eps) - rsq(G_final + eps)))
    per column, plus 1e-5 for the fp32 roundings of 40 atomic adds."""
    dup, _ = id_lists()
    rho, eps = 0.1, 1e-6
    vals = eighths((N, cols), 68)
    v16 = vals.to(BF16).cuda()
    assert torch.equal(v16.float().cpu(), vals)
    w0, G0 = rand((R, cols), 64), eighths((R, cols), 69).abs() + 0.125
    got, want = [w0.cuda(), G0.cuda()], [w0.cuda(), G0.cuda()]
    hip.row_scatter_adagrad(*got, dup, v16, 1.0, rho, eps, False)
    hip.row_scatter_adagrad(*want, dup, vals.cuda(), 1.0, rho, eps, False)
    torch.cuda.synchronize()
    got, want = [x.cpu() for x in got], [x.cpu() for x in want]
    Gf = G0.clone().index_add_(0, dup.cpu(), vals * vals)
    assert torch.equal(got[1], Gf) and torch.equal(want[1], Gf)
    counts = torch.bincount(dup.cpu(), minlength=R)
    hot = int(counts.argmax())
    assert int(counts[hot]) == 40 and int((counts > 1).sum()) == 1
    once = counts <= 1
    assert torch.allclose(got[0][once], want[0][once], **W_TOL)
    g = vals[dup.cpu() == hot].double()
    hi = (rho * g.abs() / (G0[hot].double() + g * g + eps).sqrt()).sum(0)
    lo = (rho * g.abs() / (Gf[hot].double() + eps).sqrt()).sum(0)
    diff = (got[0][hot].double() - want[0][hot].double()).abs()
    print(f"row adagrad duplicates cols={cols} hot-row max diff",
          float(diff.max()), "bound", float((hi - lo).min()))
    assert bool((diff <= hi - lo + 1e-5).all())
    assert not torch.equal(got[0][hot], w0[hot])


@pytest.mark.parametrize("name", ["momentum", "adam", "dcasgd"])
@pytest.mark.parametrize("cols,misaligned", COLS_ALIGN)
def test_row_update_bf16_vals(hip, name, cols, misaligned):
    dup, _ = id_lists()
    sids, perm = torch.sort(dup, stable=True)
    v16 = rand((N, cols), 66).to(BF16).cuda()
    wide = v16.float()
    if misaligned:
        v16 = off_by_one(v16)
    got, want = fresh(name, (R, cols), 67), fresh(name, (R, cols), 67)
    untouched = got[0].clone()
    fn = getattr(hip, f"row_{name}_update")
    scal = UPDATERS[name][1]
    fn(*got, sids, v16, *scal, perm)
    fn(*want, sids, wide, *scal, perm)
    torch.cuda.synchronize()
    same(f"row cols={cols} misaligned={misaligned}", name, got, want)
    listed = torch.zeros(R, dtype=torch.bool, device="cuda")
    listed[dup] = True
    assert torch.equal(got[0][~listed], untouched[~listed])
    assert not torch.equal(got[0][listed], untouched[listed])


# ---- table level on one GPU ----

def table_option(name):
    import multiverso_amd as mv
    return mv.AddOption.adam(lr=0.01, weight_decay=0.1) if name == "adam" \
        else None


@pytest.fixture()
def env():
    import multiverso_amd as mv
    mv.init()
    yield mv
    mv.shutdown()


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_tables_whole_ops(env, name):
    mv = env
    opt = table_option(name)
    for make, shape in [
            (lambda **kw: mv.MatrixTable(64, 8, updater_type=name, **kw),
             (64, 8)),
            (lambda **kw: mv.ArrayTable(1029, updater_type=name, **kw),
             (1029,))]:
        t, o = make(wire_dtype=BF16), make()
        assert t.shard.is_cuda and t.shard.dtype == torch.float32
        deltas = [rand(shape, 70 + k).cuda() for k in range(4)]
        # deferred Add, materialised by the next Add
        t.add(deltas[0], option=opt)
        o.add(deltas[0].to(BF16).float(), option=opt)
        # deferred Add fused with a Get into a fresh bf16 buffer; the delta
        # arrives as bf16 and is taken as it is
        d16 = deltas[1].to(BF16)
        t.add(d16, option=opt)
        assert t._deferred is not None and t._deferred[0].dtype == BF16
        assert t._deferred[0].data_ptr() == d16.data_ptr()
        o.add(d16.float(), option=opt)
        got = t.get()
        want = o.get()
        assert t._deferred is None
        assert got.dtype == BF16 and got.shape == want.shape
        assert torch.equal(got.cpu(), narrowed_by_torch(want))
        assert torch.equal(t.shard, o.shard)
        # fused into the caller's bf16 buffer
        out16 = torch.zeros(shape, dtype=BF16, device="cuda")
        t.add(deltas[2], option=opt)
        o.add(deltas[2].to(BF16).float(), option=opt)
        assert t.get(out=out16) is out16
        want = o.get()
        assert torch.equal(out16.cpu(), narrowed_by_torch(want))
        # an fp32 out materialises the Add and receives the rounded values
        out32 = torch.zeros(shape, device="cuda")
        t.add(deltas[3], option=opt)
        o.add(deltas[3].to(BF16).float(), option=opt)
        assert t.get(out=out32) is out32
        want = o.get()
        assert torch.equal(out32.cpu(), narrowed_by_torch(want).float())
        assert torch.equal(t.shard, o.shard)
        # a plain Get, no Add pending
        assert torch.equal(t.get().cpu(), narrowed_by_torch(want))


def test_mutation_guard_on_bf16_delta(env):
    mv = env
    from multiverso_amd.log import FatalError
    t = mv.MatrixTable(64, 8, updater_type="sgd", wire_dtype=BF16)
    d = torch.ones(64, 8, dtype=BF16, device="cuda")
    t.add(d)
    d.mul_(2.0)
    with pytest.raises(FatalError):
        t.get()


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("assume_unique", [False, True])
@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_tables_keyed_ops(env, name, assume_unique, deterministic):
    mv = env
    opt = table_option(name)
    t = mv.MatrixTable(64, 8, updater_type=name, wire_dtype=BF16)
    o = mv.MatrixTable(64, 8, updater_type=name)
    ids = [5, 63, 0, 17] if assume_unique else [5, 63, 5, 0, 17, 5, 63]
    # fp32 values that bf16 cannot hold: add_rows rounds them once, the
    # oracle is fed the rounded values. adam's row kernel and the
    # deterministic pre-sum add duplicates in a fixed order, so the fp32 sums
    # agree bit for bit; only sgd's atomic scatter of duplicates has no fixed
    # order, and there multiples of 1/8 keep every sum exact
    racing = name == "sgd" and not deterministic and not assume_unique
    mv.set_flag("deterministic", deterministic)
    try:
        for k in range(2):
            shape = (len(ids), 8)
            v = (eighths(shape, 80 + k) if racing
                 else rand(shape, 80 + k)).cuda()
            rounded = v.to(BF16).float()
            assert racing or not torch.equal(rounded, v)
            t.add_rows(ids, v, option=opt, assume_unique=assume_unique)
            o.add_rows(ids, rounded, option=opt, assume_unique=assume_unique)
    finally:
        mv.set_flag("deterministic", False)
    torch.cuda.synchronize()
    assert torch.equal(t.shard, o.shard)
    assert float(t.shard[5].abs().sum()) > 0
    got = t.get_rows([63, 5, 1, 5])
    assert got.dtype == BF16 and got.shape == (4, 8)
    assert torch.equal(got.cpu(), narrowed_by_torch(o.get_rows([63, 5, 1, 5])))


def test_deterministic_sum_stays_fp32(env):
    mv = env
    v = torch.tensor([[1.0], [2.0 ** -9], [2.0 ** -9]]).expand(3, 8)
    mv.set_flag("deterministic", True)
    try:
        t = mv.MatrixTable(64, 8, wire_dtype=BF16)
        t.add_rows([9, 9, 9], v.contiguous().cuda())
    finally:
        mv.set_flag("deterministic", False)
    assert torch.equal(t.shard[9].cpu(), torch.full((8,), 1.0 + 2.0 ** -8))


# ---- async engine, two ranks sharing the GPU ----

def _async_wire(rank, world):
    import multiverso_amd as mv
    mv.init()
    zoo = mv.Zoo.get()
    assert zoo.device.type == "cuda" and zoo.async_engine is not None
    t = mv.MatrixTable(10, 4, updater_type="sgd", wire_dtype=BF16)
    assert t.shard.is_cuda and t.shard.dtype == torch.float32
    base = torch.arange(40, dtype=torch.float32).view(10, 4)
    t.add(base * (rank + 1))          # acked: applied on both servers
    mv.barrier()
    got = t.get()
    assert got.is_cuda and got.dtype == BF16
    assert torch.equal(got.cpu(), (-3 * base).to(BF16)), (rank, got)
    out32 = torch.zeros(10, 4, device="cuda")
    t.get(out=out32)
    assert torch.equal(out32.cpu(), -3 * base)
    # tables without the bf16 wire still cast into a Get buffer of another
    # dtype, whichever side owns the chunk
    p = mv.MatrixTable(10, 4)
    p.add(base * (rank + 1))
    q = mv.ArrayTable(7, dtype=torch.float64)
    q.add(torch.arange(7, dtype=torch.float64) * (rank + 1))
    mv.barrier()
    for dt in (torch.float64, torch.float16, BF16):
        out = torch.zeros(10, 4, dtype=dt, device="cuda")
        assert p.get(out=out) is out
        assert torch.equal(out.cpu(), (3 * base).to(dt)), (rank, dt, out)
    out = torch.zeros(7, device="cuda")
    assert q.get(out=out) is out
    assert torch.equal(out.cpu(), 3 * torch.arange(7.0)), (rank, out)
    assert p.get().dtype == torch.float32 and q.get().dtype == torch.float64
    # keyed, uneven shards (7 rows over 2 ranks), unequal op counts
    k = mv.MatrixTable(7, 8, wire_dtype=BF16)
    for _ in range(1 if rank == 0 else 3):
        k.add_rows([0, 6, 6, 2 + rank], torch.ones(4, 8, device="cuda"))
    mv.barrier()
    rows = k.get_rows([6, 0, 2, 3, 1])
    assert rows.is_cuda and rows.dtype == BF16
    want = torch.tensor([8.0, 4.0, 1.0, 3.0, 0.0]).view(5, 1).expand(5, 8)
    assert torch.equal(rows.cpu().float(), want), (rank, rows)
    assert k.shard.dtype == torch.float32
    mv.barrier()
    mv.shutdown()


def test_async_engine_bf16_wire():
    run_dist(_async_wire, 2, gpu_share=True)
