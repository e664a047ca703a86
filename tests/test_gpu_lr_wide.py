"""The class-per-lane logistic-regression kernels (k_lr_*_wide*) against the
fp64 oracle on the inputs of lr_cases.py, under the rule of
test_gpu_lr_oracle.py (lr_cases.bound). Every CPL bucket is reached: 1 (FTRL
33, 64), 2, 3, 4, 6, 8, 12, 16. Figures: profiles/lr_wide.md."""

import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lr_cases as cases  # noqa: E402
import lr_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ["softmax", "ftrl"]
FORWARD = [("softmax", K) for K in (65, 128, 129, 200, 300, 500, 700, 1024)] \
    + [("ftrl", K) for K in (33, 64, 65, 1024)]
P = cases.FTRL
FTRL_ARGS = (P["alpha"], P["beta"], P["l1"], P["l2"])


def _cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _call(entry, c, **bad):
    """One wide entry point on case c, the named arguments replaced: (err,
    loss, table) as numpy; dense_post: (-, mean loss, diff)."""
    from multiverso_amd import ops
    hip, K = ops.module(required=True), bad.pop("K", c.K)
    a = dict(w=_cuda(cases.table(c)).view(-1), labels=_cuda(c.labels),
             wts=_cuda(c.wts), loss=torch.full((c.B,), np.nan, device="cuda"),
             err=torch.full((c.B * K,), np.nan, device="cuda"))
    a.update(bad)
    if entry == "dense_post":       # c.W holds the logits [B, K]
        a["loss"] = torch.zeros((), device="cuda")
        hip.lr_dense_post_wide(a["w"], a["labels"], a["wts"], a["loss"],
                               1.0 / c.B)
    else:
        csr = (a["w"], a.get("keys", _cuda(c.keys)),
               a.get("vals", _cuda(c.vals)), _cuda(c.ptr))
        fwd = csr + (a["labels"], a["wts"], a["err"], a["loss"])
        if entry == "softmax_forward":
            hip.lr_softmax_wide_forward(*fwd, K)
        elif entry == "ftrl_forward":
            hip.lr_ftrl_wide_forward(*fwd, *FTRL_ARGS, K)
        elif entry == "softmax_scatter":
            hip.lr_softmax_wide_scatter(*csr, a["err"], cases.LR, 2,
                                        cases.REG_COEF, K)
        else:
            hip.lr_ftrl_wide_scatter(*csr, a["err"], *FTRL_ARGS, K)
    return (a["err"].cpu().numpy(), a["loss"].cpu().numpy(),
            a["w"].cpu().numpy().reshape(cases.table(c).shape))


def _within(label, got, want, ref, tol=None):
    want = np.asarray(want, np.float64)
    err_ref, btol = cases.bound(np.asarray(ref), want)
    tol = btol if tol is None else tol
    err = float(np.max(np.abs(np.asarray(got, np.float64).reshape(want.shape)
                              - want)))
    print(f"LR_WIDE {label} err={err:.3e} err_ref={err_ref:.3e} tol={tol:.3e}")
    assert err <= tol, (label, err, err_ref, tol)


def _case(kind, K, weighted, unique=False):
    return (cases.ftrl(K, weighted) if kind == "ftrl"
            else cases.sparse("softmax", K, weighted, unique))


def _check_forward(c, label):
    want, ref = cases.forward(c)
    err, loss, after = _call(c.kind + "_forward", c)
    _within(label + " err", err, want["err"], ref["err"])
    _within(label + " loss", loss, want["loss"], ref["loss"])
    assert np.array_equal(after, cases.table(c)), "forward wrote the table"
    return err, loss


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind,K", FORWARD)
def test_forward(kind, K, weighted):
    """Segments of 0, 1, 63, 64, 65, 128, 129 and 200 features."""
    _check_forward(_case(kind, K, weighted), f"{kind}_wide K={K}")


@pytest.mark.parametrize("kind", KINDS)
def test_label_positions_and_repeatability(kind):
    """Labels 64, K-1, 63 and 0 at K = 129 (the p_y select); a second call
    returns the same bits."""
    base = _case(kind, 129, True)
    c = SimpleNamespace(**{k: v for k, v in base.__dict__.items()
                           if not k.startswith("_")})
    c.labels = base.labels.copy()
    c.labels[:4] = [64, 128, 63, 0]
    first = _check_forward(c, f"{kind}_wide labels")
    for a, b in zip(first, _call(kind + "_forward", c)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("kind", KINDS)
def test_saturated(kind):
    """Scores of +-30 and +-100 in class 1 at K = 65: all stays finite."""
    K, s = 65, np.array(cases.SAT_SCORES)
    c = SimpleNamespace(kind=kind, K=K, B=4, keys=np.arange(4), wts=None,
                        vals=np.ones(4, np.float32),
                        ptr=np.arange(5, dtype=np.int32),
                        labels=np.array([0, 1, 1, 0], np.float32))
    c.W = np.zeros((4, K), np.float32)
    c.W[:, 1] = s
    c.zn = np.concatenate([c.W * 0, c.W * 0 + 0.04], 1)
    c.zn[:, 1] = -s * ((P["beta"] + 0.2) / P["alpha"] + P["l2"]) \
        - np.sign(s) * P["l1"]
    err, loss, _ = _call(kind + "_forward", c)
    assert np.all(np.isfinite(err)) and np.all(np.isfinite(loss)), (err, loss)
    assert np.all(loss >= 0), loss


@pytest.mark.parametrize("K", [65, 200])
@pytest.mark.parametrize("kind", KINDS)
def test_scatter(kind, K):
    """Unique keys, L2 for softmax; err is the oracle's, rounded to fp32."""
    c = _case(kind, K, True, True)
    want, ref = cases.scatter(c, 0 if kind == "ftrl" else 2)
    got = _call(kind + "_scatter", c,
                err=_cuda(cases.oracle_err32(c).reshape(-1)))[2]
    _within(f"{kind}_wide_scatter K={K}", got, want, ref)
    assert np.array_equal(got[c.unnamed], cases.table(c)[c.unnamed])


@pytest.mark.parametrize("K,B,weighted", [
    (65, 37, False), (128, 37, True), (129, 37, False), (1024, 37, True),
    (65, cases.GRID_B_POST, True)])
def test_dense_post(K, B, weighted):
    """512 blocks of 4 waves at most: at B = 2085, 37 take a second sample."""
    c = cases.post(K, B, weighted)
    want = oracle.dense_post(c.logits, c.labels, c.wts)
    ref = oracle.dense_post32(c.logits, c.labels, c.wts)
    _, loss, diff = _call("dense_post", SimpleNamespace(
        kind="softmax", W=c.logits, **c.__dict__))
    _within(f"dense_post_wide K={K} diff", diff, want[0], ref[0])
    _within(f"dense_post_wide K={K} B={B} mean loss", loss, want[1].mean(),
            ref[1].mean(), cases.mean_tol(cases.bound(ref[1], want[1])[1],
                                          float(want[1].mean()),
                                          cases.n_chain(B, 4, 512)))


def _model(kind, sparse, rows):
    from multiverso_amd.apps.logreg.config import LogRegConfig
    from multiverso_amd.apps.logreg.model import PSModel
    cfg = LogRegConfig(input_size=rows, output_size=100, objective_type=kind,
                       updater_type="sgd", learning_rate=cases.MODEL_LR0,
                       minibatch_size=cases.MODEL_MB, sparse=sparse,
                       use_ps=True, alpha=P["alpha"], beta=P["beta"],
                       lambda1=P["l1"], lambda2=P["l2"])
    return PSModel(cfg, torch.device("cuda:0"))


@pytest.mark.parametrize("kind", KINDS + ["dense"])
def test_model_chunk(kind):
    """100 classes: the model picks the fused kernels, and its chunk reports
    the oracle's loss, as the unfused objective.gradient loop does, under the
    tolerance of test_gpu_lr_oracle.py::test_model_fused_chunk."""
    import multiverso_amd as mv
    from multiverso_amd import ops
    from multiverso_amd.apps.logreg.objective import Batch, DenseBatch
    mv.init(sync=True)
    try:
        if kind == "dense":
            c = cases.dense(100, 65, 37, False)
            wloss = [oracle.dense_fwd(c.X, c.W, c.labels, c.wts)[1]]
            rloss = [oracle.dense_fwd32(c.X, c.W, c.labels, c.wts)[1]]
            chain = cases.n_chain(c.B, 4, 512)
            m, b = _model("softmax", False, c.d), DenseBatch(_cuda(c.X),
                                                             _cuda(c.labels))
            assert m._dense_fused_ok()
            loss = m._dense_minibatches_fused([b], _cuda(c.W))
            loss_loop = m.objective.gradient(b, _cuda(c.W))[1]
        else:
            batches, t0 = cases.model(kind, 100)
            (want, wloss), (ref, rloss) = cases.chained(
                batches, t0, cases.model_lrs(len(batches)))
            chain = cases.MODEL_MB
            m, m_loop = (_model(kind, True, t0.shape[0]) for _ in range(2))
            tb = [Batch(_cuda(c.keys), _cuda(c.vals), _cuda(c.ptr).long(),
                        _cuda(c.labels)) for c in batches]
            fused, loop, loss_loop = _cuda(t0), _cuda(t0), 0.0
            assert m._fused_kind(fused) == kind
            loss = m._train_chunk_fused(tb, [b.keys for b in tb], fused, kind)
            for b in tb:
                grad, ll = m_loop.objective.gradient(b, loop[b.keys])
                loss_loop += ll
                ops.scatter_add_rows(loop, b.keys, grad, -1.0 if kind == "ftrl"
                                     else -m_loop.sched.next_lr())
            _within(f"model {kind} table", fused.cpu().numpy(), want, ref)
    finally:
        mv.shutdown()
    want_loss = sum(float(w.mean()) for w in wloss)
    tol = sum(cases.mean_tol(cases.bound(r, w)[1], float(w.mean()), chain)
              for r, w in zip(rloss, wloss)) + 2 * 2.0 ** -24 * want_loss
    _within(f"model {kind} loss", loss, want_loss, want_loss, tol)
    _within(f"model {kind} loop loss", loss_loop, want_loss, want_loss, tol)


@pytest.mark.parametrize("what", ["lower edge", "K=2", "K=1025", "cpu",
                                  "err size"])
@pytest.mark.parametrize("entry", ["softmax_forward", "softmax_scatter",
                                   "ftrl_forward", "ftrl_scatter"])
def test_refuses(entry, what):
    """err and the table are sized for the K asked for, so K alone offends."""
    c = _case(entry.split("_")[0], 65, True)
    K = {"lower edge": 32 if c.kind == "ftrl" else 64, "K=2": 2,
         "K=1025": 1025}.get(what)
    bad = {"cpu": dict(vals=torch.from_numpy(c.vals)),
           "err size": dict(err=torch.zeros(c.B * c.K + 1, device="cuda")),
           }.get(what) or dict(
        K=K, err=torch.zeros(c.B * K, device="cuda"),
        w=torch.zeros(c.rows * K * (2 if c.kind == "ftrl" else 1),
                      device="cuda"))
    with pytest.raises(RuntimeError):
        _call(entry, c, **bad)


@pytest.mark.parametrize("label", [-1, 65])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_refuses_label_out_of_range(kind, label):
    c = _case(kind, 65, True)
    labels = np.where(np.arange(c.B) == 3, label, c.labels).astype(np.float32)
    with pytest.raises(RuntimeError):
        _call(kind + "_forward", c, labels=_cuda(labels))


@pytest.mark.parametrize("what", ["K=64", "K=1025", "cpu"])
def test_dense_post_refuses(what):
    K = {"K=64": 64, "K=1025": 1025}.get(what, 65)
    c = SimpleNamespace(kind="softmax", K=K, B=4, wts=None,
                        W=np.zeros((4, K), np.float32),
                        labels=np.zeros(4, np.float32))
    with pytest.raises(RuntimeError):
        _call("dense_post", c, **(dict(w=torch.zeros(4 * K))
                                  if what == "cpu" else {}))
