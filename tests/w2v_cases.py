"""Inputs of the word2vec oracle tests, shared by test_w2v_oracle.py (which
checks their properties on the CPU) and test_gpu_w2v_oracle.py (which runs
them through the kernels). Nothing here imports multiverso_amd; the
expected values come from w2v_oracle.py alone.

Every case keeps its groups row-disjoint (no input or output row is named
by two groups), so the result does not depend on the order in which waves
run, with plain stores or atomics. Rows may repeat inside a group."""

from types import SimpleNamespace

import numpy as np

import w2v_oracle as oracle

LR = 0.05
EPS32 = float(np.finfo(np.float32).eps)

RAGGED_DIMS = [1, 7, 63, 64, 65, 200, 512, 513, 769, 1025, 1537, 2048]
GRID_G = 8192 + 37          # the grid caps at 8192 waves: 37 take a 2nd trip
SAMPLER_SEEDS = [1, (1 << 62) + 12345]
SAMPLER_DRAWS = {1: [2, 1, 2, 2, 1, 1, 2, 2],
                 (1 << 62) + 12345: [2, 1, 0, 2, 1, 1, 2, 2]}
NS_G, NS_NEG, NS_POOL = 24, 5, 4093
NS_DIMS = [64, 145, 769]
NS_SKIP_GROUPS = {3: 1, 11: 0, 20: 4}   # group -> which of its draws it owns


def _values(rng, rows, dim):
    return (rng.standard_normal((rows, dim)) * 0.1).astype(np.float32)


def _gsq(rng, rows, dim):
    """Accumulators: zero on even rows, up to 1e-2 on odd ones."""
    g = (rng.random((rows, dim)) * 1e-2 + 1e-4).astype(np.float32)
    g[0::2] = 0
    return g


def zero_columns(dim):
    """Two columns that are zero in every input row of the ragged case, so
    that h, the output gradient and the output accumulator stay exactly 0
    there. Not dim-1: that is the column the clamped loads duplicate, and a
    zero there would hide a leak. Narrower rows than 7 have none."""
    return [dim // 3, dim // 2] if dim >= 7 else []


def ragged(dim):
    """Six groups for k_w2v: 0-3 inputs (one id twice), 0-5 outputs (one row
    twice), labels 1-code and two fractional ones, rows nobody names."""
    rng = np.random.RandomState(1000 + dim)
    c = SimpleNamespace(dim=dim, lr=LR)
    c.in_buf, c.out_buf = _values(rng, 11, dim), _values(rng, 16, dim)
    c.in_gsq, c.out_gsq = _gsq(rng, 11, dim), _gsq(rng, 16, dim)
    zc = zero_columns(dim)
    c.in_buf[:, zc] = 0
    c.out_gsq[:, zc] = 0
    ins = [[0], [1, 2], [3, 4, 3], [], [5], [6, 7, 8]]
    outs = [[0, 1, 2], [3, 4, 3, 5, 6], [7], [8, 9], [], [10, 11, 12, 13]]
    labels = [[1, 0, 0], [0, 1, 1, 0, 1], [0], [1, 0], [], [.25, .75, 1, 0]]
    _ragged_lists(c, ins, outs, labels)
    c.unnamed_in, c.unnamed_out = [9, 10], [14, 15]
    return c


def _ragged_lists(c, ins, outs, labels):
    c.in_idx = [r for g in ins for r in g]
    c.in_off = list(np.cumsum([0] + [len(g) for g in ins]))
    c.out_idx = [r for g in outs for r in g]
    c.out_label = [float(y) for g in labels for y in g]
    c.out_off = list(np.cumsum([0] + [len(g) for g in outs]))


def grid_stride(skipgram):
    """GRID_G groups at dim 64, one output (the centre, label 1) each.
    skipgram: one input per group; else 1 or 2 alternating. Ids are
    permutations, so that a group's rows are not at its own number."""
    G, dim = GRID_G, 64
    rng = np.random.RandomState(77 + skipgram)
    c = SimpleNamespace(dim=dim, lr=LR, neg=0, seed=99)
    counts = [1] * G if skipgram else [1 + g % 2 for g in range(G)]
    n_in = sum(counts)
    c.in_buf, c.out_buf = _values(rng, n_in + 3, dim), _values(rng, G + 3, dim)
    c.in_gsq, c.out_gsq = _gsq(rng, n_in + 3, dim), _gsq(rng, G + 3, dim)
    c.in_idx = [(i * 5) % n_in for i in range(n_in)]
    assert np.gcd(5, n_in) == 1 and np.gcd(7, G) == 1
    c.in_off = list(np.cumsum([0] + counts))
    c.centers = [(g * 7) % G for g in range(G)]
    c.pool = [G]                      # never drawn: neg = 0
    c.out_idx, c.out_label = list(c.centers), [1.0] * G
    c.out_off = list(range(G + 1))
    c.unnamed_in = list(range(n_in, n_in + 3))
    c.unnamed_out = list(range(G, G + 3))
    return c


def sampler(seed):
    """One group, a pool of three rows, eight draws: the draws repeat rows
    inside the group and exercise the modulus."""
    dim = 64
    rng = np.random.RandomState(5)
    c = SimpleNamespace(dim=dim, lr=LR, neg=8, seed=seed)
    c.in_buf, c.out_buf = _values(rng, 2, dim), _values(rng, 5, dim)
    c.in_gsq, c.out_gsq = _gsq(rng, 2, dim), _gsq(rng, 5, dim)
    c.in_idx, c.in_off = [0], [0, 1]
    c.centers, c.pool = [0], [3, 1, 2]
    c.out_idx, c.out_label, c.out_off = oracle.expand_ns(
        c.centers, c.pool, c.neg, seed)
    c.unnamed_in, c.unnamed_out = [1], [4]
    return c


def collision_free_seed(start, G=NS_G, neg=NS_NEG, pool_n=NS_POOL,
                        tries=1000):
    """The first seed >= start at which no pool position is drawn by two
    groups (a group may draw one twice)."""
    for seed in range(start, start + tries):
        seen = set()
        for g in range(G):
            mine = set(oracle.ns_draws(seed, g, neg, pool_n))
            if seen & mine:
                break
            seen |= mine
        else:
            return seed
    raise AssertionError(f"no collision-free seed in {tries} tries")


def ns_multi(dim, cbow, start_seed):
    """NS_G groups drawing NS_NEG negatives each from NS_POOL distinct rows.
    Three groups have as centre a row they draw themselves (the skip);
    the other centres lie outside the pool."""
    G, neg, P = NS_G, NS_NEG, NS_POOL
    seed = collision_free_seed(start_seed)
    rng = np.random.RandomState(dim + 2 * cbow)
    c = SimpleNamespace(dim=dim, lr=LR, neg=neg, seed=seed)
    counts = [1 + g % 3 for g in range(G)] if cbow else [1] * G
    n_in = sum(counts)
    c.in_buf = _values(rng, n_in + 2, dim)
    c.out_buf = _values(rng, P + G + 2, dim)
    c.in_gsq = _gsq(rng, n_in + 2, dim)
    c.out_gsq = _gsq(rng, P + G + 2, dim)
    c.in_idx = [(i * 5) % n_in for i in range(n_in)]
    assert np.gcd(5, n_in) == 1
    c.in_off = list(np.cumsum([0] + counts))
    if cbow:
        c.in_idx[c.in_off[2] + 2] = c.in_idx[c.in_off[2]]  # an id twice
    c.pool = [(i * 1234 + 77) % P for i in range(P)]        # P is prime
    assert sorted(c.pool) == list(range(P))
    c.centers = [P + g for g in range(G)]
    for g, k in NS_SKIP_GROUPS.items():
        c.centers[g] = c.pool[oracle.ns_draws(seed, g, neg, P)[k]]
    c.out_idx, c.out_label, c.out_off = oracle.expand_ns(
        c.centers, c.pool, neg, seed)
    named_in = set(c.in_idx)
    c.unnamed_in = [r for r in range(n_in + 2) if r not in named_in]
    c.unnamed_out = [P + G, P + G + 1]
    return c


def assert_row_disjoint(c):
    """No input row and no output row is named by two groups."""
    for idx, off in ((c.in_idx, c.in_off), (c.out_idx, c.out_off)):
        seen = set()
        for g in range(len(off) - 1):
            mine = set(idx[off[g]:off[g + 1]])
            assert not (seen & mine), (g, sorted(seen & mine))
            seen |= mine


def run_oracle(c, adagrad):
    return oracle.train(c.in_buf, c.out_buf, c.in_gsq, c.out_gsq, c.in_idx,
                        c.in_off, c.out_idx, c.out_label, c.out_off, c.lr,
                        adagrad, c.lr)


def bound(ref32, want):
    """(err_ref, tolerance) of one buffer: the kernel may be 8 times as far
    from the fp64 oracle as the sequential fp32 reference is (the butterfly
    sums in another order, expf, rsqrt against sqrt and divide), and never
    needs to be closer than 4 ulp of the buffer's largest value."""
    err_ref = float(np.max(np.abs(ref32.astype(np.float64) - want)))
    return err_ref, max(8 * err_ref, 4 * EPS32 * float(np.max(np.abs(want))))
