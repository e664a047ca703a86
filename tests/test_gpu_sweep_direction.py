"""The sweep direction of the whole-shard updater kernels is a hint only.

``reverse=True`` makes k_elem visit the elements from the top down (in units
of one wave's 64 vectors). What can go wrong is the index mapping: an
element skipped, done twice or written out of range, at the ragged last wave
and when the grid cap makes the blocks loop. So every binding is run twice
on identical inputs, forward and reversed, and every tensor it writes must
be bit for bit the same; the forward side is held to the torch formulas by
test_gpu_kernels.py. Every operand is a view into the middle of a larger
tensor filled with a sentinel, and the sentinel on both sides must survive.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK = 256          # threads per block of every elementwise launch
UPD_GRID = 768       # grid cap of the fp32 updaters (vectors of 4 floats)
ELEM_GRID = 1024     # grid cap of the f64 / int forms (scalars)

# floats: the tail alone, one vector, vector + tail; the ragged last wave
# (64 vectors); several blocks; one grid-stride iteration plus a ragged
# second one, past the 256-thread grid in vectors (fp32), past the former
# fat-block grid of 1024 x 768 vectors, and past the 256 x 1024 grid
SIZES = [1, 3, 4, 5, 4 * 63, 4 * 64, 4 * 64 + 1, 4 * 65 + 3, 4 * 1023,
         4 * 1024 + 2, BLOCK * UPD_GRID * 4 + 7, 1024 * 768 * 4 + 7,
         BLOCK * ELEM_GRID * 4 + 7]
# scalar paths (f64, int, unaligned bf16) count elements, not vectors
SCALAR_SIZES = [1, 3, 63, 64, 65, 4 * 65 + 3, 4 * 1024 + 2,
                BLOCK * UPD_GRID + 7, BLOCK * ELEM_GRID + 7]

PAD = 64             # guard elements on each side; a multiple of 4


@pytest.fixture(scope="module")
def hip():
    from multiverso_amd import ops
    return ops.module(required=True)


def sentinel(dtype):
    return 7 if dtype in (torch.int32, torch.int64) else 12345.0


class Guarded:
    """A tensor's values as a view into the middle of a sentinel-filled
    allocation; ``off`` shifts the view by that many elements (bf16: 1 makes
    it 2 bytes off the 8-byte alignment the vector path needs)."""

    def __init__(self, values, off=0):
        n = values.numel()
        self.big = torch.full((n + 2 * PAD + off,), sentinel(values.dtype),
                              dtype=values.dtype, device="cuda")
        self.lo = PAD + off
        self.view = self.big[self.lo:self.lo + n]
        self.view.copy_(values)
        assert self.view.is_contiguous()

    def guards_intact(self):
        s = sentinel(self.big.dtype)
        n = self.view.numel()
        return bool((self.big[:self.lo] == s).all()
                    and (self.big[self.lo + n:] == s).all())


def rand(n, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if dtype in (torch.int32, torch.int64):
        return torch.randint(-1000, 1000, (n,), generator=g, dtype=dtype)
    return torch.randn(n, generator=g).to(dtype)


def adam_scalars():
    b1, b2, lr, wd, t = 0.9, 0.999, 1e-2, 0.01, 3
    return (b1, b2, lr / (1 - b1 ** t), (1 - b2 ** t) ** -0.5, 1 - lr * wd,
            1e-8)


# name -> (kinds of the state tensors, scalar arguments). "pos" state holds
# squares (non-negative), "any" a copy of weights or a momentum.
UPDATERS = {
    "add": ((), ()),
    "sgd": ((), ()),
    "momentum": (("any",), (0.9,)),
    "adagrad": (("pos",), (0.1, 0.05, 1e-6)),
    "dcasgd": (("any",), (0.1, 0.04)),
    "dcasgda": (("any", "pos"), (0.1, 0.04, 0.95, 1e-7)),
    "adam": (("any", "pos"), adam_scalars()),
}


def launch(hip, name, data, state, delta, out, reverse):
    args = UPDATERS[name][1]
    if name in ("add", "sgd"):
        if out is not None:
            hip.sgd_copy_update(data, delta, out, 1.0 if name == "add"
                                else -1.0, reverse=reverse)
        elif name == "add":
            hip.add_inplace(data, delta, reverse=reverse)
        else:
            hip.sgd_update(data, delta, reverse=reverse)
    elif out is not None:
        getattr(hip, name + "_copy_update")(data, *state, delta, out, *args,
                                            reverse=reverse)
    else:
        getattr(hip, name + "_update")(data, *state, delta, *args,
                                       reverse=reverse)


def both_ways(hip, name, n, copy, dtype=torch.float32,
              delta_dtype=None, out_dtype=None, off=0):
    """Run one binding forward and reversed on identical inputs; assert
    equal bits in everything it writes and intact guards."""
    delta_dtype = delta_dtype or dtype
    out_dtype = out_dtype or dtype
    data0 = rand(n, 1, dtype)
    state0 = [rand(n, 2 + k, dtype).abs() if kind == "pos"
              else rand(n, 2 + k, dtype)
              for k, kind in enumerate(UPDATERS[name][0])]
    delta0 = rand(n, 9, dtype).to(delta_dtype)
    results = []
    for reverse in (False, True):
        data = Guarded(data0)
        state = [Guarded(s) for s in state0]
        delta = Guarded(delta0, off if delta_dtype == torch.bfloat16 else 0)
        out = None
        if copy:
            out = Guarded(torch.full((n,), float("nan"), dtype=out_dtype),
                          off if out_dtype == torch.bfloat16 else 0)
        launch(hip, name, data.view, [s.view for s in state], delta.view,
               out.view if copy else None, reverse)
        torch.cuda.synchronize()
        written = [data] + state + ([out] if copy else [])
        for k, g in enumerate(written + [delta]):
            assert g.guards_intact(), (name, n, reverse, k)
        assert torch.equal(delta.view, delta0.cuda()), (name, n, reverse)
        if copy:   # every element of the Get buffer was written
            assert not torch.isnan(out.view.float()).any(), (name, n, reverse)
        results.append([g.view.clone() for g in written])
    for k, (fwd, rev) in enumerate(zip(*results)):
        assert torch.equal(fwd, rev), (name, n, k,
                                       int((fwd != rev).sum().item()))
    return results[0]


@pytest.mark.parametrize("copy", [False, True], ids=["plain", "copy"])
@pytest.mark.parametrize("name", list(UPDATERS))
def test_reverse_equals_forward(hip, name, copy):
    for n in SIZES:
        got = both_ways(hip, name, n, copy)
        if copy:
            assert torch.equal(got[-1], got[0]), (name, n)  # out == shard


@pytest.mark.parametrize("copy", [False, True], ids=["plain", "copy"])
def test_reverse_sgd_double(hip, copy):
    for n in SCALAR_SIZES:
        both_ways(hip, "sgd", n, copy, dtype=torch.float64)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float64],
                         ids=["i32", "i64", "f64"])
def test_reverse_add_scalar_forms(hip, dtype):
    """The add-only integer tables and the double add (scalar k_elem)."""
    for n in SCALAR_SIZES:
        both_ways(hip, "add", n, False, dtype=dtype)


@pytest.mark.parametrize("wire", ["delta", "out", "both"])
@pytest.mark.parametrize("name", ["sgd", "momentum", "adam"])
def test_reverse_bf16_wire(hip, name, wire):
    """bf16 delta, bf16 Get buffer, both: the 8-byte vector path."""
    bf = torch.bfloat16
    for n in SIZES[:-2]:
        both_ways(hip, name, n, True,
                  delta_dtype=bf if wire in ("delta", "both") else None,
                  out_dtype=bf if wire in ("out", "both") else None)


@pytest.mark.parametrize("wire", ["delta", "out", "both"])
def test_reverse_bf16_unaligned_view(hip, wire):
    """A bf16 view one element off takes the scalar fallback."""
    bf = torch.bfloat16
    for name in ("sgd", "momentum"):
        for n in SCALAR_SIZES:
            both_ways(hip, name, n, True, off=1,
                      delta_dtype=bf if wire in ("delta", "both") else None,
                      out_dtype=bf if wire in ("out", "both") else None)
    both_ways(hip, "sgd", 4 * 65 + 3, False, off=1, delta_dtype=bf)


def table_sequence(mv, updater):
    """Four Add+Get steps and two plain Adds with flush() on a MatrixTable,
    beside the same sequence in torch. Returns (table, gets, want_gets,
    want_shard, parities) with the parity read after every table op."""
    from multiverso_amd.updaters import AddOption
    rows, cols = 257, 37          # 9509 floats: vector body + tail of 1
    mu = 0.9
    opt = AddOption(momentum=mu) if updater == "momentum" else None
    t = mv.MatrixTable(rows, cols, updater_type=updater,
                       random_init=(-0.1, 0.1))
    device = t.shard.device
    w = t.shard.detach().clone().cpu().view(rows, cols)
    m = torch.zeros_like(w)
    gets, want, parities = [], [], []

    def ref_step(d):
        nonlocal w, m
        if updater == "sgd":
            w = w - d
        else:
            m = mu * m + (1 - mu) * d
            w = w - m

    for k in range(6):
        g = torch.Generator(device="cpu").manual_seed(100 + k)
        d = torch.randn(rows, cols, generator=g) * 1e-2
        t.add(d.to(device), opt)
        ref_step(d)
        if k in (2, 4):           # plain Adds: materialized by flush()
            t.flush()
        else:                     # Add+Get: the fused kernel on a GPU
            gets.append(t.get().cpu())
            want.append(w.clone())
        parities.append(t.updater.reverse)
        if k == 1:                # row-keyed ops leave the parity alone
            t.add_rows([3, 200], torch.ones(2, cols, device=device), opt)
            got = t.get_rows([3, 200])
            if updater == "sgd":
                w[[3, 200]] -= 1.0
            else:                 # keyed momentum: only the named rows move
                m[[3, 200]] = mu * m[[3, 200]] + (1 - mu) * 1.0
                w[[3, 200]] -= m[[3, 200]]
            gets.append(got.cpu())
            want.append(w[[3, 200]].clone())
            parities.append(t.updater.reverse)
    return t, gets, want, w, parities


# one flip per whole-shard GPU launch, none for add_rows / get_rows
GPU_PARITIES = [True, False, False, True, False, True, False]

# (rtol, atol) of test_gpu_kernels.py for the updater: test_sgd compares
# with torch.equal (every step is one rounding of w - d, here as there), so
# sgd is exact; momentum takes test_momentum's tolerance for the data
TABLE_TOL = {"sgd": (0.0, 0.0), "momentum": (1e-6, 1e-5)}


@pytest.mark.parametrize("updater", ["sgd", "momentum"])
def test_table_sequence_alternates(updater):
    import multiverso_amd as mv
    mv.init(sync=True)
    try:
        t, gets, want, w, parities = table_sequence(mv, updater)
        assert t.shard.is_cuda
        torch.cuda.synchronize()
        rtol, atol = TABLE_TOL[updater]
        for k, (g, r) in enumerate(zip(gets, want)):
            assert torch.allclose(g, r, rtol=rtol, atol=atol), \
                (k, (g - r).abs().max())
        assert torch.allclose(t.shard.cpu(), w, rtol=rtol, atol=atol)
        assert parities == GPU_PARITIES
    finally:
        mv.shutdown()
