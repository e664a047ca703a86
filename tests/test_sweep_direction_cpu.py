"""CPU tier of the sweep-direction change: the updater's parity is a GPU
performance hint, so a CPU table computes what it always did and never
touches it."""

import pytest
import torch

from test_gpu_sweep_direction import (GPU_PARITIES, TABLE_TOL,
                                      table_sequence)


@pytest.mark.parametrize("updater", ["sgd", "momentum"])
def test_table_sequence_cpu(updater):
    import multiverso_amd as mv
    mv.init(sync=True)
    try:
        t, gets, want, w, parities = table_sequence(mv, updater)
        rtol, atol = TABLE_TOL[updater]
        for k, (g, r) in enumerate(zip(gets, want)):
            assert torch.allclose(g, r, rtol=rtol, atol=atol), \
                (k, (g - r).abs().max())
        assert torch.allclose(t.shard.cpu(), w, rtol=rtol, atol=atol)
        # the CPU fallbacks neither read nor flip the parity (this tier
        # runs with the GPU masked; unmasked, the table sits on the GPU)
        assert parities == (GPU_PARITIES if t.shard.is_cuda else [False] * 7)
    finally:
        mv.shutdown()


def test_updater_parity_flips_per_call():
    from multiverso_amd.updaters import create_updater
    u = create_updater("sgd", torch.zeros(8))
    assert u.reverse is False
    assert [u._sweep() for _ in range(4)] == [False, True, False, True]
