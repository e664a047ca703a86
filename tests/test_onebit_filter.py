"""1-bit Add wire with error feedback (``add_filter="onebit"``), CPU tier:
the torch codec of onebit_filter against the oracle in onebit_oracle.py
(written from the format, importing nothing from the package), the error
feedback invariant, and ArrayTable / MatrixTable on one rank and on two ranks
over both planes.

Table oracles. Which scale bits an encoder emits depends on the order of its
fp32 sums, so a table's expected content is built from the payloads the codec
emits for the same pieces (the codec tests pin those to the format) taken
apart by the oracle's own decoder and summed in fp32 on the CPU."""

import pytest
import torch

import multiverso_amd as mv
from multiverso_amd import onebit_filter
from multiverso_amd.comm import ShardSpec
from multiverso_amd.dashboard import Dashboard

import onebit_oracle as oracle
from conftest import run_dist

CODEC_SIZES = [1, 63, 64, 1023, 1024, 1025, 3000]
# uneven shards over 2 ranks, every piece with a partial last block:
# 2051 -> 1025 + 1026 elements, 5 x 411 -> 822 + 1233
ARRAY_SIZE = 2051
MATRIX_SHAPE = (5, 411)


@pytest.fixture()
def env():
    mv.init()
    yield
    mv.shutdown()


def rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


# ---- codec ----

def test_payload_bytes():
    for n, want in [(1, 136), (1024, 136), (1025, 272), (3000, 408)]:
        assert onebit_filter.payload_bytes(n) == want


@pytest.mark.parametrize("n", CODEC_SIZES)
def test_codec_against_oracle(n):
    d, r0 = rand(n, 1), 0.5 * rand(n, 2)
    r = r0.clone()
    payload = onebit_filter.encode(d, r)
    assert payload.dtype == torch.uint8
    assert payload.numel() == 136 * ((n + 1023) // 1024)
    worst = oracle.check_encode(d, r0, payload, r, f"n={n}")
    print(f"n={n}: worst scale deviation {worst:.3e} "
          f"(bound {oracle.SCALE_RTOL:.3e})")
    # fixed summation order: the same input, the same payload
    r2 = r0.clone()
    assert torch.equal(onebit_filter.encode(d, r2), payload)
    assert oracle.same_bits(r2, r)
    # into a caller's buffer
    buf = torch.zeros(payload.numel() + 8, dtype=torch.uint8)
    r3 = r0.clone()
    out = onebit_filter.encode(d, r3, out=buf[8:])
    assert out.data_ptr() == buf[8:].data_ptr()
    assert torch.equal(buf[8:], payload) and not bool(buf[:8].any())


def test_codec_one_sided_blocks():
    """A block with no negative (no non-negative) value: that scale is 0."""
    n = 1500
    d = rand(n, 3).abs() + 0.1
    d[1024:] = -d[1024:]
    r0 = torch.zeros(n)
    r = r0.clone()
    payload = onebit_filter.encode(d, r)
    oracle.check_encode(d, r0, payload, r)
    scales, _ = oracle.split(payload, n)
    assert float(scales[0, 0]) == 0.0 and float(scales[0, 1]) > 0
    assert float(scales[1, 1]) == 0.0 and float(scales[1, 0]) < 0


@pytest.mark.parametrize("n", [1, 1025, 3000])
@pytest.mark.parametrize("nparts", [1, 2, 3])
def test_decode_sum(n, nparts):
    payloads = [onebit_filter.encode(rand(n, 10 + p), 0.5 * rand(n, 20 + p))
                for p in range(nparts)]
    want = oracle.decode_sum(payloads, n)
    got = onebit_filter.decode_sum(torch.cat(payloads), n, nparts)
    assert got.dtype == torch.float32 and got.shape == (n,)
    assert oracle.same_bits(got, want)
    # a sequence of payloads, and a caller's buffer
    out = torch.zeros(n)
    assert onebit_filter.decode_sum(payloads, n, nparts, out=out) is out
    assert oracle.same_bits(out, want)
    with pytest.raises(ValueError):
        onebit_filter.decode_sum(torch.cat(payloads)[:-1], n, nparts)


def test_dashboard_accounting():
    Dashboard.reset()
    onebit_filter.encode(rand(3000, 1), torch.zeros(3000))
    assert Dashboard.get("onebit_filter.bytes_in").count == 1
    assert Dashboard.get("onebit_filter.bytes_in").elapsed_ms == 12000
    assert Dashboard.get("onebit_filter.bytes_out").elapsed_ms == 408


# ---- error feedback ----

def test_error_feedback(env):
    """table + residual tracks the sum of the deltas: each step rounds twice
    per element in fp32 (v = r + d, r = v - q), each by at most 2**-24 |v|
    (|v - q| <= max|v|: q is the mean of values with v's sign), and the bound
    lets those add up linearly over the k steps."""
    k, n = 20, 3000
    t = mv.ArrayTable(n, add_filter="onebit")
    total = torch.zeros(n, dtype=torch.float64)
    vmax = 0.0
    for step in range(k):
        d = rand(n, 100 + step)
        r = t.residual if t.residual is not None else torch.zeros(n)
        vmax = max(vmax, float((r + d).abs().max()))
        t.add(d)
        total += d.double()
    assert t.residual.shape == (n,) and t.residual.dtype == torch.float32
    got = t.get().double() + t.residual.double()
    diff = float((got - total).abs().max())
    bound = 2 * k * 2.0 ** -24 * vmax
    print(f"error feedback: max |table + residual - sum d| = {diff:.3e}, "
          f"bound {bound:.3e} (max|v| = {vmax:.3f})")
    assert diff <= bound
    # and the table alone is NOT the sum: the filter really quantises
    assert float((t.get().double() - total).abs().max()) > 1e-3


# ---- tables ----

def make_tables(updater, **kw):
    """(table, its flat size, unit of its ShardSpec) for both table kinds."""
    a = mv.ArrayTable(ARRAY_SIZE, updater_type=updater, **kw)
    m = mv.MatrixTable(*MATRIX_SHAPE, updater_type=updater, **kw)
    return [(a, (ARRAY_SIZE,), 1), (m, MATRIX_SHAPE, MATRIX_SHAPE[1])]


def decoded_delta(delta, units, unit, world, device="cpu"):
    """What the owners decode from a worker's first Add of ``delta`` (zero
    residual): each server's piece through the codec on ``device``, its
    payload through the oracle's decoder. Flat fp32 on the CPU."""
    flat = delta.reshape(-1).to(device)
    res = torch.zeros_like(flat)
    spec = ShardSpec(units, world)
    out = torch.empty(flat.numel())
    for s in range(world):
        off, cnt = spec.range_of(s)
        lo, hi = off * unit, (off + cnt) * unit
        payload = onebit_filter.encode(flat[lo:hi], res[lo:hi])
        out[lo:hi] = oracle.decode(payload, hi - lo)
    return out


def option_for(updater):
    return (mv.AddOption.adam(lr=0.01, weight_decay=0.1)
            if updater == "adam" else None)


@pytest.mark.parametrize("updater", ["default", "sgd", "adam"])
def test_tables_local(env, updater):
    opt = option_for(updater)
    for (t, shape, unit), (o, _, _) in zip(
            make_tables(updater, add_filter="onebit"), make_tables(updater)):
        assert t.add_filter == "onebit" and t.residual is None
        d = rand(shape, 30)
        q = decoded_delta(d, shape[0], unit, 1)
        t.add(d, option=opt)
        o.add(q.view(shape), option=opt)
        got = t.get()
        assert got.shape == torch.Size(shape)
        assert oracle.same_bits(got, o.get())
        if updater == "default":
            assert oracle.same_bits(got.view(-1), q)
        assert t.residual.numel() == d.numel()
        assert oracle.same_bits(t.residual, d.view(-1) - q)
        assert o.residual is None


def two_rank_scenario(rank, world, plane, device="cpu"):
    """One Add from each rank into filtered tables, checked on every rank.
    ``plane``: "sync" (collectives) or "async" (the engine)."""
    for updater in (["default", "sgd", "adam"] if plane == "sync"
                    else ["default", "sgd"]):
        opt = option_for(updater)
        for (t, shape, unit), (o, _, _) in zip(
                make_tables(updater, add_filter="onebit"),
                make_tables(updater)):
            deltas = [rand(shape, 40 + r) for r in range(world)]
            qs = [decoded_delta(d, shape[0], unit, world, device)
                  for d in deltas]
            t.add(deltas[rank].to(device), option=opt)
            if plane == "sync":
                # one update with the decoded sum: rank 0 brings it, the
                # others bring zeros, which the reduce-scatter adds exactly
                total = qs[0]
                for q in qs[1:]:
                    total = total + q
                o.add((total if rank == 0 else torch.zeros_like(total))
                      .view(shape), option=opt)
            else:
                # one update per arriving delta; the two orders of default
                # and sgd give the same bits (two terms commute in fp32)
                o.add(qs[rank].view(shape), option=opt)
            mv.barrier()
            got, want = t.get(), o.get()
            assert got.shape == torch.Size(shape)
            assert oracle.same_bits(got, want), (plane, updater, shape, rank)
            if updater == "default":
                assert oracle.same_bits(got.reshape(-1), qs[0] + qs[1])
            assert float(got.abs().sum()) > 0
            assert t.residual.numel() == deltas[rank].numel()
            assert t.residual.device.type == torch.device(device).type
            assert oracle.same_bits(t.residual,
                                    deltas[rank].reshape(-1) - qs[rank])
            mv.barrier()
    # async_op on the sync plane, a second Add on the same residual
    if plane == "sync":
        (t, shape, unit), _ = make_tables("default", add_filter="onebit")
        t.add(rand(shape, 50 + rank)).wait()
        r1 = t.residual.clone()
        h = t.add(rand(shape, 52 + rank), async_op=True)
        h.wait()
        assert not torch.equal(t.residual, r1)
        mv.barrier()
        assert float(t.get().abs().sum()) > 0
        mv.barrier()


def _sync_plane(rank, world):
    mv.init(sync=True)
    two_rank_scenario(rank, world, "sync")
    mv.shutdown()


def _async_plane(rank, world):
    mv.init()
    assert mv.Zoo.get().async_engine is not None
    two_rank_scenario(rank, world, "async")
    mv.shutdown()


def test_two_ranks_sync_plane():
    run_dist(_sync_plane, 2)


def test_two_ranks_async_plane():
    run_dist(_async_plane, 2)


# ---- interface ----

def test_add_rows_is_unfiltered(env):
    t = mv.MatrixTable(*MATRIX_SHAPE, add_filter="onebit")
    t.add(rand(MATRIX_SHAPE, 60))
    before, res = t.get().clone(), t.residual.clone()
    vals = rand((3, MATRIX_SHAPE[1]), 61)
    t.add_rows([0, 4, 2], vals)
    assert oracle.same_bits(t.residual, res)
    assert torch.equal(t.get_rows([0, 4, 2]), before[[0, 4, 2]] + vals)
    assert torch.equal(t.get()[[1, 3]], before[[1, 3]])


def test_refusals(env):
    for dtype in (torch.float64, torch.int32):
        with pytest.raises(TypeError, match="float32"):
            mv.ArrayTable(8, dtype=dtype, add_filter="onebit")
        with pytest.raises(TypeError, match="float32"):
            mv.MatrixTable(4, 2, dtype=dtype, add_filter="onebit")
    with pytest.raises(TypeError, match="follow-up"):
        mv.ArrayTable(8, wire_dtype=torch.bfloat16, add_filter="onebit")
    with pytest.raises(TypeError, match="follow-up"):
        mv.MatrixTable(4, 2, wire_dtype=torch.bfloat16, add_filter="onebit")
    with pytest.raises(ValueError, match="add_filter"):
        mv.ArrayTable(8, add_filter="twobit")
    with pytest.raises(ValueError, match="add_filter"):
        mv.MatrixTable(4, 2, add_filter="")
    with pytest.raises(TypeError):
        mv.SparseMatrixTable(4, 2, add_filter="onebit")


def test_no_filter_no_residual(env):
    for t, shape, _ in make_tables("default"):
        d = rand(shape, 70)
        t.add(d)
        assert t.add_filter is None and t.residual is None
        assert torch.equal(t.get(), d)
