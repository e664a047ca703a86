"""CPU tests of the word2vec oracle (w2v_oracle.py) and of the inputs the GPU
tests feed the kernels (w2v_cases.py): the fp64 oracle against the torch
reference _w2v_train_torch, the sampler against a second implementation,
and the properties every GPU case relies on."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2v_cases as cases  # noqa: E402
import w2v_oracle as oracle  # noqa: E402

from multiverso_amd.apps.wordembedding.model import _w2v_train_torch  # noqa: E402

EPS32 = cases.EPS32


def _run_torch(c, adagrad, lr, lr0):
    bufs = [torch.from_numpy(x.copy())
            for x in (c.in_buf, c.out_buf, c.in_gsq, c.out_gsq)]
    _w2v_train_torch(bufs[0], bufs[1], bufs[2] if adagrad else None,
                     bufs[3] if adagrad else None,
                     torch.tensor(c.in_idx, dtype=torch.int64),
                     torch.tensor(c.in_off, dtype=torch.int32),
                     torch.tensor(c.out_idx, dtype=torch.int64),
                     torch.tensor(c.out_label, dtype=torch.float32),
                     torch.tensor(c.out_off, dtype=torch.int32),
                     lr, adagrad, lr0)
    return [b.numpy() for b in bufs]


def _random_ragged(seed, dim):
    """Random ragged groups over shared rows (the oracle and the torch
    reference are both sequential, so rows may be shared between groups):
    0-3 inputs and 0-4 outputs per group, an id twice in one group."""
    rng = np.random.RandomState(seed)
    c = cases.SimpleNamespace(dim=dim)
    n_in, n_out, G = 9, 11, 7
    c.in_buf, c.out_buf = cases._values(rng, n_in, dim), cases._values(rng, n_out, dim)
    c.in_gsq, c.out_gsq = cases._gsq(rng, n_in, dim), cases._gsq(rng, n_out, dim)
    ins = [list(rng.randint(0, n_in, rng.randint(0, 4))) for _ in range(G)]
    outs = [list(rng.randint(0, n_out, rng.randint(0, 5))) for _ in range(G)]
    ins[1] = [4, 2, 4]
    outs[1] = [6, 6, 1]
    labels = [list(rng.randint(0, 2, len(o)).astype(float)) for o in outs]
    cases._ragged_lists(c, ins, outs, labels)
    return c


@pytest.mark.parametrize("adagrad", [False, True])
@pytest.mark.parametrize("seed,dim", [(0, 5), (1, 64), (2, 145)])
def test_oracle_matches_torch_reference(seed, dim, adagrad):
    """Two independent sequential implementations, fp64 numpy and fp32
    torch, with lr != lr0: the decayed rate drives the plain step, the
    initial one the adagrad step. A row is named at most about ten times
    over the 7 groups, and each update rounds a handful of times at the
    size of the row's values; the error of e (a dot product of `dim` terms
    of size 1e-2) is smaller still. 64 eps of the buffer's largest value
    covers that, and a wrong rate, label or order is off by 1e-3 or more."""
    c = _random_ragged(seed, dim)
    lr, lr0 = 0.0125, 0.05
    want = oracle.train(c.in_buf, c.out_buf, c.in_gsq, c.out_gsq, c.in_idx,
                        c.in_off, c.out_idx, c.out_label, c.out_off, lr,
                        adagrad, lr0)
    got = _run_torch(c, adagrad, lr, lr0)
    if adagrad:
        assert want[4] > 1e-3, want[4]
    for k, name in enumerate(["in_buf", "out_buf", "in_gsq", "out_gsq"]):
        if k >= 2 and not adagrad:
            assert want[k] is None
            continue
        tol = 64 * EPS32 * float(np.abs(want[k]).max())
        err = float(np.abs(got[k] - want[k]).max())
        assert err <= tol, (name, err, tol)
    # and the rates are told apart: swapping them must not fit
    swapped = oracle.train(c.in_buf, c.out_buf, c.in_gsq, c.out_gsq,
                           c.in_idx, c.in_off, c.out_idx, c.out_label,
                           c.out_off, lr0, adagrad, lr)
    assert float(np.abs(swapped[0] - want[0]).max()) > 1e-3


def _ns_draws_uint64(seed, g, neg, pool_n):
    """Second implementation: numpy.uint64, which wraps on overflow."""
    mul, add = np.uint64(oracle.LCG_MUL), np.uint64(oracle.LCG_ADD)
    with np.errstate(over="ignore"):
        r = np.uint64(seed) + np.uint64(g) * mul + add
        out = []
        for _ in range(neg):
            r = r * mul + add
            out.append(int((r >> np.uint64(8)) % np.uint64(pool_n)))
    return out


@pytest.mark.parametrize("seed", [0, 1, 12345, (1 << 32) - 1,
                                  (1 << 62) + 12345, (1 << 63) - 1])
def test_ns_draws_matches_uint64_arithmetic(seed):
    for g in (0, 1, 23, 8228, 1 << 22):
        for pool_n in (1, 3, 4093, 1 << 20):
            assert (oracle.ns_draws(seed, g, 9, pool_n)
                    == _ns_draws_uint64(seed, g, 9, pool_n)), (g, pool_n)


def test_ns_draws_known_sequences():
    for seed, draws in cases.SAMPLER_DRAWS.items():
        assert oracle.ns_draws(seed, 0, 8, 3) == draws


def test_expand_ns_skips_but_consumes():
    """Seed 1, group 0, pool of 3 draws positions [2,1,2,2,1,1,2,2]. With
    the centre at the row in position 1, those three draws vanish and the
    others keep their places in the sequence; a skip that did not consume
    its draw would shift everything after it."""
    pool = [10, 11, 12]
    idx, lab, off = oracle.expand_ns([11], pool, 8, 1)
    assert idx == [11, 12, 12, 12, 12, 12]
    assert lab == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert off == [0, 6]
    # centre outside the pool: nothing dropped; second group: its own stream
    idx, lab, off = oracle.expand_ns([7, 7], pool, 8, 1)
    assert off == [0, 9, 18]
    assert idx[1:9] == [pool[p] for p in oracle.ns_draws(1, 0, 8, 3)]
    assert idx[10:18] == [pool[p] for p in oracle.ns_draws(1, 1, 8, 3)]
    assert idx[1:9] != idx[10:18]
    # neg = 0: the centre alone
    assert oracle.expand_ns([5, 6], pool, 0, 1) == ([5, 6], [1.0, 1.0],
                                                    [0, 1, 2])


@pytest.mark.parametrize("adagrad", [False, True])
def test_empty_input_list_gives_zero_hidden(adagrad):
    """A group without inputs has h = 0, as in the kernel: its outputs see
    f = 1/2 and a zero gradient, so nothing changes and nothing is NaN."""
    c = cases.SimpleNamespace()
    rng = np.random.RandomState(3)
    c.in_buf, c.out_buf = cases._values(rng, 2, 8), cases._values(rng, 3, 8)
    c.in_gsq, c.out_gsq = cases._gsq(rng, 2, 8), cases._gsq(rng, 3, 8)
    cases._ragged_lists(c, [[]], [[0, 1]], [[1, 0]])
    before = [x.copy() for x in (c.in_buf, c.out_buf, c.in_gsq, c.out_gsq)]
    got = _run_torch(c, adagrad, 0.05, 0.05)
    want = oracle.train(c.in_buf, c.out_buf, c.in_gsq, c.out_gsq, c.in_idx,
                        c.in_off, c.out_idx, c.out_label, c.out_off, 0.05,
                        adagrad, 0.05)
    for k in range(4):
        assert np.array_equal(got[k], before[k]), k
        if want[k] is not None:
            assert np.array_equal(want[k], before[k].astype(np.float64)), k


@pytest.mark.parametrize("adagrad", [False, True])
def test_group_without_outputs_changes_nothing(adagrad):
    c = cases.SimpleNamespace()
    rng = np.random.RandomState(4)
    c.in_buf, c.out_buf = cases._values(rng, 3, 8), cases._values(rng, 2, 8)
    c.in_gsq, c.out_gsq = cases._gsq(rng, 3, 8), cases._gsq(rng, 2, 8)
    cases._ragged_lists(c, [[0, 1, 1]], [[]], [[]])
    before = [x.copy() for x in (c.in_buf, c.out_buf, c.in_gsq, c.out_gsq)]
    got = _run_torch(c, adagrad, 0.05, 0.05)
    want = oracle.train(c.in_buf, c.out_buf, c.in_gsq, c.out_gsq, c.in_idx,
                        c.in_off, c.out_idx, c.out_label, c.out_off, 0.05,
                        adagrad, 0.05)
    for k in range(4):
        assert np.array_equal(got[k], before[k]), k
        if want[k] is not None:
            assert np.array_equal(want[k], before[k].astype(np.float64)), k


# ---- the inputs of the GPU tests ------------------------------------------

def _all_cases():
    yield from (cases.ragged(d) for d in cases.RAGGED_DIMS)
    yield from (cases.sampler(s) for s in cases.SAMPLER_SEEDS)
    yield cases.ns_multi(64, False, cases.SAMPLER_SEEDS[0])
    yield cases.ns_multi(145, True, cases.SAMPLER_SEEDS[1])


def test_gpu_cases_are_row_disjoint_and_in_range():
    for c in list(_all_cases()) + [cases.grid_stride(False),
                                   cases.grid_stride(True)]:
        cases.assert_row_disjoint(c)
        assert 0 <= min(c.in_idx) and max(c.in_idx) < len(c.in_buf)
        if c.out_idx:
            assert 0 <= min(c.out_idx) and max(c.out_idx) < len(c.out_buf)
        assert not set(c.unnamed_in) & set(c.in_idx)
        assert not set(c.unnamed_out) & set(c.out_idx)
        assert c.in_off[-1] == len(c.in_idx)
        assert c.out_off[-1] == len(c.out_idx) == len(c.out_label)


def test_gpu_cases_keep_clear_of_the_adagrad_threshold():
    for c in _all_cases():
        assert cases.run_oracle(c, True)[4] > 1e-3


def test_ragged_case_zero_columns_keep_accumulator_zero():
    c = cases.ragged(200)
    zc = cases.zero_columns(200)
    assert len(zc) == 2
    want = cases.run_oracle(c, True)
    named = sorted(set(c.out_idx))
    assert np.all(want[3][named][:, zc] == 0)
    assert np.array_equal(want[1][named][:, zc],
                          c.out_buf[named][:, zc].astype(np.float64))
    # elsewhere those rows did move
    assert np.all(np.abs(want[1][[0, 3, 10]] - c.out_buf[[0, 3, 10]]).max(1)
                  > 1e-3)


def test_collision_free_seeds():
    small = cases.collision_free_seed(cases.SAMPLER_SEEDS[0])
    large = cases.collision_free_seed(cases.SAMPLER_SEEDS[1])
    assert small == 1 and large == (1 << 62) + 12345 + 20
    with pytest.raises(AssertionError):
        # 24 * 5 draws from 4 positions must collide
        cases.collision_free_seed(1, pool_n=4, tries=5)


def test_ns_multi_case_exercises_the_skip():
    c = cases.ns_multi(64, True, 1)
    lens = np.diff(c.out_off)
    for g in range(cases.NS_G):
        draws = oracle.ns_draws(c.seed, g, c.neg, cases.NS_POOL)
        hits = sum(c.pool[p] == c.centers[g] for p in draws)
        assert lens[g] == 1 + c.neg - hits
        assert (hits >= 1) == (g in cases.NS_SKIP_GROUPS)
    # the repeated id sits inside one group
    assert len(set(c.in_idx)) == len(c.in_idx) - 1
