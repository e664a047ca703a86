"""GPU tests of the block top-k Add wire: the k_topk_encode and
k_topk_decode_sum kernels against the reference in test_topk_filter.py (which
imports nothing from the package) and against the CPU torch codec, and the
tables built with ``add_filter="topk:8"`` on one GPU. Every comparison is bit
for bit: the format leaves an implementation no freedom."""

import pytest
import torch

from conftest import run_dist
from test_topk_filter import (ARRAY_SIZE, KEEPS, MATRIX_SHAPE, SIZES,
                              check_encode, rand, ref_decode_sum, ref_encode,
                              same_bits, special_input, split,
                              tables_scenario)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from multiverso_amd import ops, topk_filter
    ops.module(required=True)
    return topk_filter


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("n", SIZES)
def test_encode_against_reference(codec, n, keep):
    d, r0 = rand(n, 1), 0.5 * rand(n, 2)
    payload = check_encode(d, r0, keep, "cuda")
    assert payload.is_cuda
    # the CPU codec writes the same bytes, and a second launch does too
    rc, rg = r0.clone(), r0.cuda()
    assert torch.equal(codec.encode(d, rc, keep), payload.cpu())
    assert torch.equal(codec.encode(d.cuda(), rg, keep), payload)
    assert same_bits(rg, rc)


@pytest.mark.parametrize("keep", [4, 32])
@pytest.mark.parametrize("kind", ["equal", "ties", "last_digit", "specials"])
def test_special_inputs(codec, kind, keep):
    d, r0 = special_input(kind)
    check_encode(d, r0, keep, "cuda")


def test_encode_misaligned_pieces(codec):
    """d and r one element (4 bytes) off, as a piece of a table is, and a
    payload 8 bytes into its buffer; nothing is written around the residual
    piece or the payload."""
    n, m = 1025, 32
    d, r0 = rand(n, 4), 0.5 * rand(n, 5)
    dbuf, rbuf = torch.zeros(n + 2, device="cuda"), torch.ones(n + 2).cuda()
    dbuf[1:n + 1].copy_(d)
    rbuf[1:n + 1].copy_(r0)
    assert dbuf[1:].data_ptr() % 16 == 4 and rbuf[1:].data_ptr() % 16 == 4
    size = 6 * m * 2
    pbuf = torch.full((size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    payload = codec.encode(dbuf[1:n + 1], rbuf[1:n + 1], m,
                           out=pbuf[8:8 + size])
    vals, poss, res = ref_encode(d, r0, m)
    assert same_bits(split(payload, n, m)[0], vals)
    assert torch.equal(split(payload, n, m)[1], poss)
    assert same_bits(rbuf[1:n + 1], res)
    assert float(rbuf[0]) == 1 and float(rbuf[n + 1]) == 1
    assert bool((pbuf[:8] == 0xA5).all()) and bool((pbuf[8 + size:] == 0xA5)
                                                   .all())


@pytest.mark.parametrize("n", [1, 1025, 4099])
def test_decode_sum(codec, n):
    payloads = [codec.encode(rand(n, 10 + p).cuda(),
                             torch.zeros(n, device="cuda"), 256)
                for p in range(3)]
    want = ref_decode_sum([split(p, n, 256) for p in payloads], n)
    got = codec.decode_sum(torch.cat(payloads), n, 3, 256)
    assert got.is_cuda and got.data_ptr() % 16 == 0
    assert same_bits(got, want)
    # an out 4 bytes off the 16-byte alignment: scalar stores, n elements
    buf = torch.full((n + 2,), 7.0, device="cuda")
    out = buf[1:n + 1]
    assert out.data_ptr() % 16 == 4
    assert codec.decode_sum(payloads, n, 3, 256, out=out) is out
    assert same_bits(out, want)
    assert float(buf[0]) == 7 and float(buf[n + 1]) == 7


# ---- tables on one GPU ----

@pytest.fixture()
def env():
    import multiverso_amd as mv
    mv.init()
    yield mv
    mv.shutdown()


def test_tables_whole_ops(env):
    """Plain (materialised by the next op), deferred and fused Add+Get."""
    mv = env
    tables_scenario(0, 1, "cuda")
    for make, shape in [(lambda **kw: mv.ArrayTable(ARRAY_SIZE, **kw),
                         (ARRAY_SIZE,)),
                        (lambda **kw: mv.MatrixTable(*MATRIX_SHAPE, **kw),
                         MATRIX_SHAPE)]:
        t, total = make(add_filter="topk:8"), torch.zeros(shape)
        res = torch.zeros(total.numel())
        for step in range(3):
            d = rand(shape, 80 + step)
            vals, poss, res = ref_encode(d.view(-1), res, 8)
            total += ref_decode_sum([(vals, poss)], res.numel()).view(shape)
            dg = d.cuda()
            t.add(dg)
            assert t._deferred is not None
            dg.zero_()          # the decoded tensor is the table's own
        out = torch.zeros(shape, device="cuda")
        assert t.get(out=out) is out and t._deferred is None    # fused
        assert same_bits(out, total) and same_bits(t.shard, total)
        assert same_bits(t.residual, res)


# ---- async engine, two ranks sharing the GPU ----

def _async_topk(rank, world):
    import multiverso_amd as mv
    mv.init()
    zoo = mv.Zoo.get()
    assert zoo.device.type == "cuda" and zoo.async_engine is not None
    tables_scenario(rank, world, "cuda")
    mv.shutdown()


def test_async_engine_topk():
    run_dist(_async_topk, 2, gpu_share=True)
