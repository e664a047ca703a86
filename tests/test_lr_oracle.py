"""CPU tests of the logistic-regression oracle (lr_oracle.py) and of the
inputs the GPU tests feed the kernels (lr_cases.py): the fp64 oracle against
the project's own CPU path (objective.gradient + index_add_), the sequential
fp32 reference against the oracle, and the properties every GPU case relies
on."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lr_cases as cases  # noqa: E402

from multiverso_amd.apps.logreg.config import LogRegConfig  # noqa: E402
from multiverso_amd.apps.logreg.objective import (  # noqa: E402
    Batch, create_objective)

REG = {0: "none", 1: "l1", 2: "l2"}


def _objective(c, reg_type):
    p = cases.FTRL
    return create_objective(LogRegConfig(
        input_size=c.rows, output_size=c.K, objective_type=c.kind,
        regular_type=REG[reg_type], regular_coef=cases.REG_COEF,
        alpha=p["alpha"], beta=p["beta"], lambda1=p["l1"], lambda2=p["l2"]))


def _cpu_step(c, table, lr, reg_type):
    """One minibatch the way the model's unfused path takes it."""
    keys = torch.from_numpy(c.keys)
    b = Batch(keys, torch.from_numpy(c.vals),
              torch.from_numpy(c.ptr).long(), torch.from_numpy(c.labels),
              None if c.wts is None else torch.from_numpy(c.wts))
    grad, loss = _objective(c, reg_type).gradient(b, table[keys])
    table.index_add_(0, keys, grad, alpha=-1.0 if c.kind == "ftrl" else -lr)
    return loss


def _cpu_cases():
    out = []
    for weighted in (False, True):
        out.append(("sigmoid", 1, weighted, 0))
        for K in (2, 3, 17, 64):
            out.append(("softmax", K, weighted, 0))
    for reg_type in (1, 2):
        out.append(("sigmoid", 1, True, reg_type))
        for K in cases.REG_KS:
            out.append(("softmax", K, True, reg_type))
    for K in (1, 2, 3, 17, 32):
        out.append(("ftrl", K, K in cases.FTRL_WEIGHTED_KS, 0))
    return out


def _case(kind, K, weighted, reg_type):
    if kind == "ftrl":
        return cases.ftrl(K, weighted)
    if reg_type == 1:
        return cases.sparse_l1(kind, K)
    return cases.sparse(kind, K, weighted, reg_type != 0)


@pytest.mark.parametrize("kind,K,weighted,reg_type", _cpu_cases())
def test_cpu_path_matches_oracle(kind, K, weighted, reg_type):
    """objective.gradient then index_add_ against the chained oracle: the
    whole table within the bound, the mean loss within the per-sample loss
    bound plus B additions (torch's mean, in whatever order it sums). FTRL
    at K > 1 is the loss summed over the outputs."""
    c = _case(kind, K, weighted, reg_type)
    (want, wloss), (ref, rloss) = cases.chained(
        [c], cases.table(c), [cases.LR], reg_type)
    got = torch.from_numpy(cases.table(c).copy())
    loss = _cpu_step(c, got, cases.LR, reg_type)
    err_ref, tol = cases.bound(ref, want)
    err = float(np.max(np.abs(got.numpy().astype(np.float64) - want)))
    assert err <= tol, (err, err_ref, tol)
    _, ltol = cases.bound(rloss[0], wloss[0])
    want_mean = float(wloss[0].mean())
    assert abs(loss - want_mean) <= cases.mean_tol(ltol, want_mean, c.B), \
        (loss, want_mean, ltol)
    assert np.array_equal(got.numpy()[c.unnamed], cases.table(c)[c.unnamed])


def _forward_cases():
    out = [cases.sparse("sigmoid", 1, w) for w in (False, True)]
    out += [cases.sparse("softmax", K, w) for K in cases.SOFTMAX_KS
            for w in (False, True)]
    out += [cases.ftrl(K, w) for K in cases.FTRL_KS
            for w in ((False, True) if K in cases.FTRL_WEIGHTED_KS
                      else (False,))]
    out += [cases.grid(k) for k in ("sigmoid", "softmax", "ftrl")]
    return out


def _small(err_ref, want):
    """Finite, non-zero, and no more than 64 ulp of the buffer's largest
    value (of 1 where that is smaller)."""
    return 0 < err_ref <= 64 * cases.EPS32 * max(1.0, np.max(np.abs(want)))


def test_fp32_reference_close_to_oracle_forward():
    for c in _forward_cases():
        want, ref = cases.forward(c)
        for name in ("err", "loss"):
            assert ref[name].dtype == np.float32
            assert want[name].shape == ref[name].shape
            err_ref, _ = cases.bound(ref[name], want[name])
            assert _small(err_ref, want[name]), (c.kind, c.K, name, err_ref)


def test_fp32_reference_close_to_oracle_scatter():
    todo = [(cases.sparse("sigmoid", 1, True), 0),
            (cases.sparse("softmax", 3, True), 0),
            (cases.sparse("softmax", 64, False), 0),
            (cases.sparse_l1("softmax", 17), 1),
            (cases.sparse("softmax", 17, True, True), 2),
            (cases.ftrl(1, True), 0), (cases.ftrl(17, True), 0),
            (cases.grid("ftrl"), 0)]
    for c, reg_type in todo:
        want, ref = cases.scatter(c, reg_type)
        assert ref.dtype == np.float32 and ref.shape == want.shape
        err_ref, _ = cases.bound(ref, want)
        assert _small(err_ref, want), (c.kind, c.K, reg_type, err_ref)
        assert np.array_equal(ref[c.unnamed], cases.table(c)[c.unnamed])


def test_fp32_reference_close_to_oracle_dense():
    from lr_oracle import dense_fwd, dense_fwd32, dense_post, dense_post32
    for K in (1, 2, 16):
        c = cases.dense(K, 200, 37, True)
        want, ref = (f(c.X, c.W, c.labels, c.wts)
                     for f in (dense_fwd, dense_fwd32))
        p = cases.post(K, 37, True)
        wantp, refp = (f(p.logits, p.labels, p.wts)
                       for f in (dense_post, dense_post32))
        for w, r in zip(want + wantp, ref + refp):
            assert r.dtype == np.float32 and r.shape == w.shape
            assert _small(cases.bound(r, w)[0], w)


@pytest.mark.parametrize("kind", ["sigmoid", "softmax", "ftrl"])
def test_saturated_case(kind):
    """The constructed scores are there, exactly those samples are left out
    of the loss comparison, and the oracle's loss is finite and >= 0."""
    c = cases.saturated(kind)
    want, ref = cases.forward(c)
    s = want["s"][c.sat, 1 % c.K]
    assert np.allclose(s, cases.SAT_SCORES, rtol=1e-5), s
    keep = cases.unsaturated(c, want["s"])
    assert keep.sum() == cases.B_REGULAR
    assert set(c.labels[c.sat]) == {0.0, 1.0}
    # log(1 - p + 1e-12) is +1e-12 in fp64 once p < 1e-12 and rounds to
    # log(1) = 0 in fp32: the formula itself, not a fault of either
    for f, floor in ((want, -2 * 1e-12), (ref, 0.0)):
        assert np.all(np.isfinite(f["loss"])) and np.all(f["loss"] >= floor)
        assert np.all(np.isfinite(f["err"]))
    err_ref, _ = cases.bound(ref["loss"][keep], want["loss"][keep])
    assert _small(err_ref, want["loss"][keep])


def _sparse_cases():
    out = _forward_cases()
    out += [cases.sparse(k, K, True, True) for k, K in
            (("sigmoid", 1), ("softmax", 3), ("softmax", 17))]
    out += [cases.sparse_l1(k, K) for k, K in
            (("sigmoid", 1), ("softmax", 3), ("softmax", 17))]
    out += [cases.saturated(k) for k in ("sigmoid", "softmax", "ftrl")]
    for kind, K in (("sigmoid", 1), ("softmax", 3), ("ftrl", 1), ("ftrl", 3)):
        out += cases.model(kind, K)[0]
    return out


def test_case_conditions():
    for c in _sparse_cases():
        label = (c.kind, c.K, c.B)
        assert c.ptr.dtype == np.int32 and c.keys.dtype == np.int64, label
        assert c.vals.dtype == np.float32 and len(c.vals) == len(c.keys)
        assert c.ptr[0] == 0 and c.ptr[-1] == len(c.keys), label
        lens = np.diff(c.ptr)
        assert np.all(lens >= 0) and len(lens) == c.B, label
        if c.B in (cases.B_REGULAR, cases.B_REGULAR + 4):
            assert set(cases.REQUIRED_LENGTHS) <= set(lens), label
        elif c.B == cases.GRID_B:
            assert set(lens) == {0, 1, 2, 3}, label
        assert not set(c.unnamed) & set(c.keys), label
        assert c.keys.min() >= 0 and c.keys.max() < c.rows - 2, label
        if hasattr(c, "W") or hasattr(c, "zn"):
            assert cases.table(c).shape == (
                c.rows, c.K * (2 if c.kind == "ftrl" else 1)), label
        labels = c.labels.astype(np.int64)
        assert labels.min() == 0 and labels.max() == max(c.K, 2) - 1, label
        if c.kind == "ftrl" or c.unique:
            assert len(np.unique(c.keys)) == len(c.keys), label
        elif c.B == cases.B_REGULAR:
            # duplicates within a sample and across samples
            sid = np.repeat(np.arange(c.B), lens)
            pairs = len(set(zip(sid, c.keys)))
            assert pairs < len(c.keys), label
            assert len(np.unique(c.keys)) < pairs, label
        if c.kind == "ftrl" and hasattr(c, "zn"):
            cases.assert_ftrl_margins(c)


def test_model_cases_unique_within_minibatch():
    for kind, K in (("sigmoid", 1), ("softmax", 3), ("ftrl", 1), ("ftrl", 3)):
        batches, t0 = cases.model(kind, K)
        assert [c.B for c in batches] == [cases.MODEL_MB] * 2
        for c in batches:
            assert len(np.unique(c.keys)) == len(c.keys)
            assert c.keys.max() < t0.shape[0] - 2


def test_l1_cases_margins():
    for kind, K in (("sigmoid", 1), ("softmax", 3), ("softmax", 17)):
        c = cases.sparse_l1(kind, K)
        cases.assert_l1_margins(c)
        named = c.W[c.keys]
        assert np.any(named == 0) and np.any(named > 0) and np.any(named < 0)


def test_n_chain_matches_launch_geometry():
    """k_lr_dense_post: min(ceil(B/4), 512) blocks of 4 waves;
    k_lr_dense_fwd: min(ceil(B/16), 256) blocks of 16 waves."""
    assert cases.n_chain(37, 4, 512) == 1 + 4 + 10
    assert cases.n_chain(cases.GRID_B_POST, 4, 512) == 2 + 4 + 512
    assert cases.n_chain(37, 16, 256) == 1 + 16 + 3
    assert cases.n_chain(cases.GRID_B_DENSE, 16, 256) == 2 + 16 + 256


def test_ftrl_multiclass_loss_sums_all_outputs():
    """What the class-0 term alone would miss is far above the bound."""
    c = cases.ftrl(3, True)
    want, ref = cases.forward(c)
    _, tol = cases.bound(ref["loss"], want["loss"])
    p = 1 / (1 + np.exp(-want["s"]))
    y0 = (c.labels == 0).astype(np.float64)
    class0 = -(y0 * np.log(p[:, 0] + 1e-12)
               + (1 - y0) * np.log(1 - p[:, 0] + 1e-12))
    assert np.max(want["loss"] - class0) > 1000 * tol
