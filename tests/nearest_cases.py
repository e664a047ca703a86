"""Inputs shared by the nearest_rows tests (not a test file). Every case is
built once per process and must be left unchanged by its users."""

import functools

import torch

from nearest_oracle import margin

# (rows, cols, Q, k): torch.randn data. The oracle gap at the k-th score
# exceeds twice the tolerance, so both metrics must return the oracle's id
# set exactly; random_case asserts that precondition on the oracle alone.
RANDOM = [(5000, 8, 16, 64), (700, 200, 3, 10), (300, 257, 1, 64),
          (130, 65, 17, 1)]
# may take check()'s weaker branch: all ties under cosine (every row is
# +-1 after normalisation), and a bound loosened by 2048 columns
LOOSE = [(64, 1, 2, 64), (1000, 2048, 2, 5)]
# integer data in [-3, 3], many duplicate rows, metric "dot": fp32 is exact,
# results equal the oracle's bit for bit, tie order included. The second has
# fewer rows per shard than k at 2 and 3 ranks; 100 = 33 + 33 + 34.
EXACT = [(500, 24, 5, 64), (100, 7, 3, 64), (130, 65, 17, 5)]

_SEEDS = {(5000, 8, 16, 64): 11, (700, 200, 3, 10): 12,
          (300, 257, 1, 64): 13, (130, 65, 17, 1): 14}


def _randn(shape, seed):
    R, C, Q, k = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, C, generator=g), torch.randn(Q, C, generator=g), k


@functools.lru_cache(maxsize=None)
def random_case(shape):
    """(table, queries, k) of a RANDOM shape."""
    table, queries, k = _randn(shape, _SEEDS[shape])
    for metric in ("dot", "cosine"):
        m = margin(table, queries, k, metric)
        assert m > 1.0, (shape, metric, "seed leaves no gap: g/(2 tol) =", m)
    return table, queries, k


@functools.lru_cache(maxsize=None)
def loose_case(shape):
    return _randn(shape, 21)


@functools.lru_cache(maxsize=None)
def sweep_case(Q):
    """(130, 65, Q, 5) for the sweep over Q = 1..16; the gap is asserted as
    for the RANDOM shapes."""
    table, queries, k = _randn((130, 65, Q, 5), 100 + Q)
    for metric in ("dot", "cosine"):
        m = margin(table, queries, k, metric)
        assert m > 1.0, (Q, metric, "seed leaves no gap: g/(2 tol) =", m)
    return table, queries, k


@functools.lru_cache(maxsize=None)
def exact_case(shape):
    R, C, Q, k = shape
    g = torch.Generator().manual_seed(31 + R)
    base = torch.randint(-3, 4, (max(R // 12, 2), C), generator=g)
    table = base[torch.randint(0, base.shape[0], (R,), generator=g)].float()
    queries = torch.randint(-3, 4, (Q, C), generator=g).float()
    return table, queries, k
