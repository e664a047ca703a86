"""GPU tests of the 1-bit Add wire: the k_onebit_encode and
k_onebit_decode_sum kernels against the oracle in onebit_oracle.py (which
imports nothing from the package), against the CPU torch codec, and the
tables built with ``add_filter="onebit"`` on one GPU.

What the format fixes bit for bit — signs, pad bits, the new residual given
the emitted scales, the decoded sum — is compared bit for bit. A scale is the
fp32 mean of up to 1024 same-signed values in the kernel's own (fixed)
summation order, so it is held to relative 2**-14 of the fp64 mean:
(1024 - 1) * 2**-24 for the sum plus 2**-24 for the divide."""

import pytest
import torch

import onebit_oracle as oracle
from conftest import run_dist
from test_onebit_filter import (ARRAY_SIZE, MATRIX_SHAPE, option_for, rand,
                                two_rank_scenario)

pytestmark = pytest.mark.gpu

# one lane, a partial / a full / one past a full ballot word, a partial / a
# full / one past a full block, several blocks with a ragged end, many blocks
ENCODE_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4099, 262147]


@pytest.fixture(scope="module")
def codec():
    from multiverso_amd import onebit_filter, ops
    ops.module(required=True)
    return onebit_filter


@pytest.mark.parametrize("n", ENCODE_SIZES)
def test_encode_against_oracle(codec, n):
    d, r0 = rand(n, 1), 0.5 * rand(n, 2)
    r = r0.cuda()
    payload = codec.encode(d.cuda(), r)
    torch.cuda.synchronize()
    assert payload.is_cuda and payload.dtype == torch.uint8
    assert payload.numel() == 136 * ((n + 1023) // 1024)
    worst = oracle.check_encode(d, r0, payload, r, f"n={n}")
    print(f"n={n}: worst scale deviation {worst:.3e} "
          f"(bound {oracle.SCALE_RTOL:.3e})")
    # the same input gives the same payload and residual, bit for bit
    r2 = r0.cuda()
    again = codec.encode(d.cuda(), r2)
    torch.cuda.synchronize()
    assert torch.equal(again, payload)
    assert oracle.same_bits(r2, r)


def test_encode_one_sided_blocks(codec):
    n = 1500
    d = rand(n, 3).abs() + 0.1
    d[1024:] = -d[1024:]
    r = torch.zeros(n, device="cuda")
    payload = codec.encode(d.cuda(), r)
    oracle.check_encode(d, torch.zeros(n), payload, r)
    scales, _ = oracle.split(payload, n)
    assert float(scales[0, 0]) == 0.0 and float(scales[0, 1]) > 0
    assert float(scales[1, 1]) == 0.0 and float(scales[1, 0]) < 0


def test_encode_misaligned_pieces(codec):
    """d and r one element (4 bytes) off, as a piece of a table is; nothing is
    written around the residual piece or the payload."""
    n = 1025
    d, r0 = rand(n, 4), 0.5 * rand(n, 5)
    dbuf = torch.zeros(n + 2, device="cuda")
    rbuf = torch.zeros(n + 2, device="cuda")
    dbuf[1:n + 1].copy_(d)
    rbuf[1:n + 1].copy_(r0)
    dv, rv = dbuf[1:n + 1], rbuf[1:n + 1]
    assert dv.data_ptr() % 16 == 4 and rv.data_ptr() % 16 == 4
    pbuf = torch.zeros(272 + 16, dtype=torch.uint8, device="cuda")
    payload = codec.encode(dv, rv, out=pbuf[8:8 + 272])
    torch.cuda.synchronize()
    oracle.check_encode(d, r0, payload, rv, "misaligned")
    aligned = codec.encode(d.cuda(), r0.cuda())
    assert torch.equal(payload, aligned)
    assert float(rbuf[0]) == 0 and float(rbuf[n + 1]) == 0
    assert not bool(pbuf[:8].any()) and not bool(pbuf[8 + 272:].any())


@pytest.mark.parametrize("n", [1, 1025, 4099])
@pytest.mark.parametrize("nparts", [1, 2, 3, 8])
def test_decode_sum(codec, n, nparts):
    payloads = [codec.encode(rand(n, 10 + p).cuda(),
                             (0.5 * rand(n, 20 + p)).cuda())
                for p in range(nparts)]
    want = oracle.decode_sum(payloads, n)
    got = codec.decode_sum(torch.cat(payloads), n, nparts)
    torch.cuda.synchronize()
    assert got.is_cuda and got.data_ptr() % 16 == 0
    assert oracle.same_bits(got, want)
    # an out 4 bytes off the 16-byte alignment: scalar stores
    buf = torch.zeros(n + 2, device="cuda")
    out = buf[1:n + 1]
    assert out.data_ptr() % 16 == 4
    assert codec.decode_sum(payloads, n, nparts, out=out) is out
    torch.cuda.synchronize()
    assert oracle.same_bits(out, want)
    assert float(buf[0]) == 0 and float(buf[n + 1]) == 0


@pytest.mark.parametrize("n", [1, 1025, 4099, 262147])
def test_payload_matches_cpu_codec(codec, n):
    """Signs are identical; a scale may differ in its last bits (each codec
    has its own summation order), and both are within the bound of the fp64
    mean. Where no scale differs the payloads are byte-identical."""
    d, r0 = rand(n, 6), 0.5 * rand(n, 7)
    rc, rg = r0.clone(), r0.cuda()
    cpu = codec.encode(d, rc)
    gpu = codec.encode(d.cuda(), rg).cpu()
    oracle.check_encode(d, r0, cpu, rc, "cpu")
    oracle.check_encode(d, r0, gpu, rg, "gpu")
    nb = (n + 1023) // 1024
    assert torch.equal(cpu[8 * nb:], gpu[8 * nb:])
    sc, _ = oracle.split(cpu, n)
    sg, _ = oracle.split(gpu, n)
    differ = int((sc.view(torch.int32) != sg.view(torch.int32)).sum())
    print(f"n={n}: {differ} of {2 * nb} scales differ between GPU and CPU")
    if differ == 0:
        assert torch.equal(cpu, gpu)
    assert torch.allclose(sc, sg, rtol=2 * oracle.SCALE_RTOL, atol=0)


# ---- tables on one GPU ----

@pytest.fixture()
def env():
    import multiverso_amd as mv
    mv.init()
    yield mv
    mv.shutdown()


@pytest.mark.parametrize("updater", ["default", "sgd", "adam"])
def test_tables_whole_ops(env, codec, updater):
    mv = env
    opt = option_for(updater)
    for make, shape in [
            (lambda **kw: mv.ArrayTable(ARRAY_SIZE, updater_type=updater,
                                        **kw), (ARRAY_SIZE,)),
            (lambda **kw: mv.MatrixTable(*MATRIX_SHAPE, updater_type=updater,
                                         **kw), MATRIX_SHAPE)]:
        t, o = make(add_filter="onebit"), make()
        assert t.shard.is_cuda and t.residual is None
        n = t.shard.numel()
        res = torch.zeros(n, device="cuda")   # the test's own residual

        def step(seed):
            """Add a delta to t, and what it decodes to (this test's encode on
            the same kernel, the oracle's decode) to o."""
            d = rand(shape, seed).cuda()
            q = oracle.decode(codec.encode(d.reshape(-1), res), n)
            t.add(d, option=opt)
            assert t._deferred is not None
            assert t._deferred[0].data_ptr() != d.data_ptr()
            d.zero_()           # the decoded tensor is the table's own
            o.add(q.view(shape).cuda(), option=opt)

        step(80)                # deferred, materialised by the next Add
        step(81)                # deferred, fused with the Get below
        got = t.get()
        assert t._deferred is None and got.dtype == torch.float32
        assert oracle.same_bits(got, o.get())
        assert oracle.same_bits(t.shard, o.shard)
        out = torch.zeros(shape, device="cuda")     # fused into an fp32 out
        step(82)
        assert t.get(out=out) is out
        assert oracle.same_bits(out, o.get())
        host = torch.zeros(shape)       # a CPU out materialises the Add
        step(83)
        assert t.get(out=host) is host
        assert oracle.same_bits(host, o.get())
        assert t.residual.is_cuda and t.residual.numel() == n
        assert oracle.same_bits(t.residual, res)
        assert o.residual is None


def test_add_rows_leaves_residual(env):
    mv = env
    t = mv.MatrixTable(*MATRIX_SHAPE, add_filter="onebit")
    t.add(rand(MATRIX_SHAPE, 60).cuda())
    before, res = t.get().clone(), t.residual.clone()
    vals = rand((3, MATRIX_SHAPE[1]), 61).cuda()
    t.add_rows([0, 4, 2], vals)
    assert oracle.same_bits(t.residual, res)
    assert torch.equal(t.get_rows([0, 4, 2]), before[[0, 4, 2]] + vals)


# ---- async engine, two ranks sharing the GPU ----

def _async_onebit(rank, world):
    import multiverso_amd as mv
    mv.init()
    zoo = mv.Zoo.get()
    assert zoo.device.type == "cuda" and zoo.async_engine is not None
    two_rank_scenario(rank, world, "async", device="cuda")
    mv.shutdown()


def test_async_engine_onebit():
    run_dist(_async_onebit, 2, gpu_share=True)
