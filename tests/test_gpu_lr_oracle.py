"""GPU tests of the fused logistic-regression kernels (k_lr_* in kernels.hip)
against the fp64 oracle (lr_oracle.py) on the inputs of lr_cases.py: every
template instantiation the launchers reach (softmax 2..16 / 32 / 64, FTRL
1..16 / 32, dense forward 1..16 with and without non-temporal loads), ragged
CSR batches with empty and longer-than-a-wave samples, L1 / L2 in the
scatter, launches larger than each grid, saturated scores, the model's fused
chunk against its objective.gradient loop, and the bindings' refusals.

Each comparison covers a whole buffer. The kernel must be within
max(8 * err_ref, 4 * eps * max|oracle|) of the oracle, err_ref being the
distance of the sequential fp32 reference from the oracle (w2v_cases.bound);
rows no key names, and everything a forward kernel only reads, must come
back bit-identical. The measured figures are in profiles/lr_oracle.md."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lr_cases as cases  # noqa: E402
import lr_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["sigmoid", "softmax", "ftrl"]
# (waves per block, most blocks) of the two dense kernels' launches
POST_GEOMETRY = (4, 512)        # grid_for_cap(B * 64, 512) blocks of BLOCK=256
DENSE_GEOMETRY = (16, 256)      # min(ceil(B / 16), 256) blocks of 1024


def _hip():
    from multiverso_amd import ops
    return ops.module(required=True)


def _cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _batch(c):
    return SimpleBatch(_cuda(c.keys), _cuda(c.vals), _cuda(c.ptr),
                       _cuda(c.labels), _cuda(c.wts))


class SimpleBatch:
    def __init__(self, keys, vals, ptr, labels, wts):
        self.keys, self.vals, self.ptr = keys, vals, ptr
        self.labels, self.wts = labels, wts


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32),
                          np.asarray(b).view(np.int32))


def _compare(label, name, got, want, ref, failures, keep=None):
    """One buffer against the oracle; prints the figures, notes a miss."""
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    if keep is not None:
        got, want, ref = got[keep], want[keep], ref[keep]
    err_ref, tol = cases.bound(ref, want)
    err = float(np.max(np.abs(got - want)))
    print(f"LR_ORACLE {label} {name} err={err:.3e} err_ref={err_ref:.3e} "
          f"tol={tol:.3e} share={err / tol:.2f}")
    if not err <= tol:          # also catches NaN
        failures.append((name, err, err_ref, tol))
    return tol


def _compare_mean(label, got, want_loss, ltol, chain, failures):
    want = float(np.mean(want_loss))
    tol = cases.mean_tol(ltol, want, chain)
    err = abs(float(got) - want)
    print(f"LR_ORACLE {label} mean_loss err={err:.3e} loss_tol={ltol:.3e} "
          f"n_chain={chain} tol={tol:.3e} share={err / tol:.2f}")
    if not err <= tol:
        failures.append(("mean_loss", err, ltol, tol))


# ---- running the kernels ------------------------------------------------------

def _run_forward(c, table=None):
    """(err [B, K], loss [B], table after) as numpy."""
    hip, b = _hip(), _batch(c)
    t = _cuda(cases.table(c) if table is None else table)
    err = torch.full((c.B * c.K,), float("nan"), device="cuda")
    loss = torch.full((c.B,), float("nan"), device="cuda")
    flat = t.view(-1)
    if c.kind == "sigmoid":
        hip.lr_sigmoid_forward(flat, b.keys, b.vals, b.ptr, b.labels, b.wts,
                               err, loss)
    elif c.kind == "softmax":
        hip.lr_softmax_forward(flat, b.keys, b.vals, b.ptr, b.labels, b.wts,
                               err, loss, c.K)
    else:
        p = cases.FTRL
        hip.lr_ftrl_forward(flat, b.keys, b.vals, b.ptr, b.labels, b.wts,
                            err, loss, p["alpha"], p["beta"], p["l1"],
                            p["l2"], c.K)
    torch.cuda.synchronize()
    return (err.cpu().numpy().reshape(c.B, c.K), loss.cpu().numpy(),
            t.cpu().numpy())


def _run_scatter(c, err, reg_type=0):
    """The table after a scatter of err (fp32 [B, K]), as numpy."""
    hip, b = _hip(), _batch(c)
    t = _cuda(cases.table(c))
    flat, e = t.view(-1), _cuda(err.astype(np.float32).reshape(-1))
    if c.kind == "sigmoid":
        hip.lr_sigmoid_scatter(flat, b.keys, b.vals, b.ptr, e, cases.LR,
                               reg_type, cases.REG_COEF)
    elif c.kind == "softmax":
        hip.lr_softmax_scatter(flat, b.keys, b.vals, b.ptr, e, cases.LR,
                               reg_type, cases.REG_COEF, c.K)
    else:
        p = cases.FTRL
        hip.lr_ftrl_scatter(flat, b.keys, b.vals, b.ptr, e, p["alpha"],
                            p["beta"], p["l1"], p["l2"], c.K)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _check_forward(c, label):
    want, ref = cases.forward(c)
    err, loss, after = _run_forward(c)
    failures = []
    _compare(label, "err", err, want["err"], ref["err"], failures)
    _compare(label, "loss", loss, want["loss"], ref["loss"], failures)
    assert _same_bits(after, cases.table(c)), f"{label}: forward wrote w"
    assert not failures, (label, failures)
    return loss


def _check_scatter(c, label, reg_type=0):
    want, ref = cases.scatter(c, reg_type)
    got = _run_scatter(c, cases.oracle_err32(c), reg_type)
    failures = []
    _compare(label, "w", got, want, ref, failures)
    assert _same_bits(got[c.unnamed], cases.table(c)[c.unnamed]), \
        f"{label}: an unnamed row changed"
    assert not failures, (label, failures)


# ---- sparse forward: every instantiation ------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
def test_sigmoid_forward(weighted):
    _check_forward(cases.sparse("sigmoid", 1, weighted),
                   f"sigmoid_fwd wts={weighted}")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", cases.SOFTMAX_KS)
def test_softmax_forward(K, weighted):
    """Exact K = 2..16; 17 and 32 in the 32-bucket, 33, 63 and 64 in the
    64-bucket, whose `k < KK` guards are live."""
    _check_forward(cases.sparse("softmax", K, weighted),
                   f"softmax_fwd K={K} wts={weighted}")


FTRL_FWD = [(K, w) for K in cases.FTRL_KS
            for w in ((False, True) if K in cases.FTRL_WEIGHTED_KS
                      else (False,))]


@pytest.mark.parametrize("K,weighted", FTRL_FWD)
def test_ftrl_forward(K, weighted):
    """Exact K = 1..16; 17 and 32 in the 32-bucket. At K >= 2 the loss is
    the binary NLL summed over all K outputs, as Objective.loss has it: the
    class-0 term alone misses by the other outputs' NLL (2.97 at K = 3
    against a bound of 3.1e-6, profiles/lr_oracle.md)."""
    _check_forward(cases.ftrl(K, weighted), f"ftrl_fwd K={K} wts={weighted}")


def test_ftrl_forward_k1_equals_sigmoid_forward():
    """With alpha = beta = 1, l1 = l2 = 0 and n = 0 the state (-w | 0)
    reconstructs to exactly w, and the K = 1 FTRL forward is the sigmoid
    forward: same sum, same sigmoid, no cross-lane loss sum. err and loss
    agree bit for bit."""
    c = cases.sparse("sigmoid", 1, True)
    err_s, loss_s, _ = _run_forward(c)
    hip, b = _hip(), _batch(c)
    zn = _cuda(np.concatenate([-c.W, np.zeros_like(c.W)], 1))
    err = torch.empty(c.B, device="cuda")
    loss = torch.empty(c.B, device="cuda")
    hip.lr_ftrl_forward(zn.view(-1), b.keys, b.vals, b.ptr, b.labels, b.wts,
                        err, loss, 1.0, 1.0, 0.0, 0.0, 1)
    torch.cuda.synchronize()
    assert _same_bits(err.cpu().numpy(), err_s[:, 0])
    assert _same_bits(loss.cpu().numpy(), loss_s)


# ---- sparse scatter ---------------------------------------------------------------

@pytest.mark.parametrize("kind,K", [("sigmoid", 1)] + [
    ("softmax", K) for K in (2, 3, 10, 17, 33, 64)])
def test_scatter_duplicate_keys(kind, K):
    """No regularisation; keys repeat within and across samples, so the
    atomics carry the result. err is the oracle's, rounded to fp32."""
    _check_scatter(cases.sparse(kind, K, True), f"{kind}_scatter K={K}")


@pytest.mark.parametrize("reg_type", [1, 2], ids=["l1", "l2"])
@pytest.mark.parametrize("kind,K", [("sigmoid", 1), ("softmax", 3),
                                    ("softmax", 17)])
def test_scatter_regularised(kind, K, reg_type):
    """Unique keys (the kernel reads w while other lanes add to it); under
    L1 a tenth of the weights are exactly 0."""
    c = (cases.sparse_l1(kind, K) if reg_type == 1
         else cases.sparse(kind, K, True, True))
    _check_scatter(c, f"{kind}_scatter K={K} reg={reg_type}", reg_type)


@pytest.mark.parametrize("K,weighted", FTRL_FWD)
def test_ftrl_scatter(K, weighted):
    _check_scatter(cases.ftrl(K, weighted),
                   f"ftrl_scatter K={K} wts={weighted}")


@pytest.mark.parametrize("kind", KINDS)
def test_forward_into_scatter(kind):
    """The forward kernel's own err handed to the scatter kernel."""
    c = (cases.ftrl(3, True) if kind == "ftrl"
         else cases.sparse(kind, {"sigmoid": 1, "softmax": 3}[kind], True))
    (want, _), (ref, _) = cases.chained([c], cases.table(c), [cases.LR])
    err, _, _ = _run_forward(c)
    got = _run_scatter(c, err)
    failures = []
    _compare(f"{kind}_chained K={c.K}", "w", got, want, ref, failures)
    assert _same_bits(got[c.unnamed], cases.table(c)[c.unnamed])
    assert not failures, failures


# ---- more samples than waves: the loops' second trip ------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_grid_stride_forward(kind):
    _check_forward(cases.grid(kind), f"{kind}_fwd B={cases.GRID_B}")


@pytest.mark.parametrize("kind", KINDS)
def test_grid_stride_scatter(kind):
    _check_scatter(cases.grid(kind), f"{kind}_scatter B={cases.GRID_B}")


# ---- saturated scores ---------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_saturated(kind):
    """Scores of +-30 and +-100 on four samples: err within the bound
    everywhere, loss finite and >= 0 everywhere and within the bound where
    |s| <= 8 (softmax: largest logit gap <= 8)."""
    c = cases.saturated(kind)
    want, ref = cases.forward(c)
    keep = cases.unsaturated(c, want["s"])
    err, loss, _ = _run_forward(c)
    failures = []
    label = f"{kind}_saturated"
    _compare(label, "err", err, want["err"], ref["err"], failures)
    _compare(label, "loss", loss, want["loss"], ref["loss"], failures, keep)
    assert np.all(np.isfinite(loss)) and np.all(loss >= 0), loss[c.sat]
    assert not failures, failures


# ---- dense ----------------------------------------------------------------------------

def _check_dense_fwd(c, nt, label):
    want = oracle.dense_fwd(c.X, c.W, c.labels, c.wts)
    ref = oracle.dense_fwd32(c.X, c.W, c.labels, c.wts)
    x, w = _cuda(c.X), _cuda(c.W)
    diff = torch.full((c.B, c.K), float("nan"), device="cuda")
    acc = torch.zeros((), device="cuda")
    took = _hip().lr_dense_fwd(x, w, _cuda(c.labels), _cuda(c.wts), diff,
                               acc, 1.0 / c.B, nt)
    torch.cuda.synchronize()
    assert took, f"{label}: the fused forward declined"
    failures = []
    _compare(label, "diff", diff.cpu().numpy(), want[0], ref[0], failures)
    _, ltol = cases.bound(ref[1], want[1])
    _compare_mean(label, acc, want[1], ltol,
                  cases.n_chain(c.B, *DENSE_GEOMETRY), failures)
    assert _same_bits(x.cpu().numpy(), c.X) and _same_bits(w.cpu().numpy(), c.W)
    assert not failures, (label, failures)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("K", cases.DENSE_KS)
def test_dense_forward(K, nt, weighted):
    """All 32 instantiations; d = 200 is three full lane trips and a part.
    n_chain = 1 + 16 + 3: one sample per wave, 16 waves per block, 3 blocks."""
    _check_dense_fwd(cases.dense(K, 200, 37, weighted), nt,
                     f"dense_fwd K={K} nt={nt} wts={weighted}")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", cases.DENSE_EDGE_DS)
@pytest.mark.parametrize("K", cases.DENSE_EDGE_KS)
def test_dense_forward_row_edges(K, d, weighted):
    _check_dense_fwd(cases.dense(K, d, 37, weighted), False,
                     f"dense_fwd K={K} d={d} wts={weighted}")


@pytest.mark.parametrize("K", [1, 3])
def test_dense_forward_grid_stride(K):
    """256 blocks of 16 waves: 37 waves take a second sample.
    n_chain = 2 + 16 + 256."""
    _check_dense_fwd(cases.dense(K, 65, cases.GRID_B_DENSE, True), K == 3,
                     f"dense_fwd K={K} B={cases.GRID_B_DENSE}")


def _check_dense_post(c, label):
    want = oracle.dense_post(c.logits, c.labels, c.wts)
    ref = oracle.dense_post32(c.logits, c.labels, c.wts)
    logits = _cuda(c.logits)
    acc = torch.zeros((), device="cuda")
    _hip().lr_dense_post(logits, _cuda(c.labels), _cuda(c.wts), acc,
                         1.0 / c.B)
    torch.cuda.synchronize()
    failures = []
    _compare(label, "diff", logits.cpu().numpy(), want[0], ref[0], failures)
    _, ltol = cases.bound(ref[1], want[1])
    _compare_mean(label, acc, want[1], ltol,
                  cases.n_chain(c.B, *POST_GEOMETRY), failures)
    assert not failures, (label, failures)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", cases.POST_KS)
def test_dense_post(K, weighted):
    """n_chain = 1 + 4 + 10: one sample per wave, 4 waves per block, 10
    blocks for 37 samples."""
    _check_dense_post(cases.post(K, 37, weighted),
                      f"dense_post K={K} wts={weighted}")


@pytest.mark.parametrize("K", [1, 5])
def test_dense_post_grid_stride(K):
    """512 blocks of 4 waves: 37 waves take a second sample.
    n_chain = 2 + 4 + 512."""
    _check_dense_post(cases.post(K, cases.GRID_B_POST, True),
                      f"dense_post K={K} B={cases.GRID_B_POST}")


# ---- the model's fused chunk against its objective.gradient loop ----------------------

@pytest.mark.parametrize("kind,K", [("sigmoid", 1), ("softmax", 3),
                                    ("ftrl", 1), ("ftrl", 3)])
def test_model_fused_chunk(kind, K):
    """PSModel._train_chunk_fused and the unfused loop of train_chunk on
    the same device and the same two minibatches: both tables within the
    bound of the chained oracle, both returned losses (the sum of the two
    batch means) within the sum of the batches' loss bounds, 16 additions
    per mean and 2 more for the sum. FTRL at K = 3 is the loss summed over
    the outputs, end to end."""
    import multiverso_amd as mv
    from multiverso_amd import ops
    from multiverso_amd.apps.logreg.config import LogRegConfig
    from multiverso_amd.apps.logreg.model import PSModel
    from multiverso_amd.apps.logreg.objective import Batch
    batches, t0 = cases.model(kind, K)
    lrs = cases.model_lrs(len(batches))
    (want, wloss), (ref, rloss) = cases.chained(batches, t0, lrs)
    p = cases.FTRL
    cfg = LogRegConfig(input_size=t0.shape[0], output_size=K,
                       objective_type=kind, updater_type="sgd",
                       learning_rate=cases.MODEL_LR0,
                       minibatch_size=cases.MODEL_MB, sparse=True,
                       use_ps=True, alpha=p["alpha"], beta=p["beta"],
                       lambda1=p["l1"], lambda2=p["l2"])
    mv.init(sync=True)
    try:
        dev = torch.device("cuda:0")
        m_fused, m_loop = PSModel(cfg, dev), PSModel(cfg, dev)
        tb = [Batch(_cuda(c.keys), _cuda(c.vals), _cuda(c.ptr).long(),
                    _cuda(c.labels)) for c in batches]
        lidxs = [b.keys for b in tb]

        fused = _cuda(t0)
        assert m_fused._fused_kind(fused) == kind
        loss_fused = m_fused._train_chunk_fused(tb, lidxs, fused, kind)

        loop, loss_loop = _cuda(t0), 0.0
        for b, lidx in zip(tb, lidxs):
            grad, loss = m_loop.objective.gradient(b, loop[lidx])
            loss_loop += loss
            lr = m_loop.sched.next_lr()
            ops.scatter_add_rows(loop, lidx, grad,
                                 -1.0 if kind == "ftrl" else -lr)
        torch.cuda.synchronize()
    finally:
        mv.shutdown()
    want_loss = sum(float(w.mean()) for w in wloss)
    loss_tol = sum(cases.mean_tol(cases.bound(r, w)[1], float(w.mean()),
                                  cases.MODEL_MB)
                   for r, w in zip(rloss, wloss)) \
        + 2 * 2.0 ** -24 * want_loss
    failures = []
    for name, table, loss in (("fused", fused, loss_fused),
                              ("loop", loop, loss_loop)):
        label = f"model {kind} K={K} {name}"
        _compare(label, "local", table.cpu().numpy(), want, ref, failures)
        err = abs(loss - want_loss)
        print(f"LR_ORACLE {label} loss err={err:.3e} tol={loss_tol:.3e} "
              f"share={err / loss_tol:.2f}")
        if not err <= loss_tol:
            failures.append((name + " loss", loss, want_loss, loss_tol))
        unnamed = batches[0].unnamed
        assert _same_bits(table.cpu().numpy()[unnamed], t0[unnamed])
    assert not failures, failures


# ---- refusals: every one raises before any launch ------------------------------------------

def _call(entry, c, **bad):
    """Call one lr_* entry point on case c with the named arguments
    replaced."""
    hip, b = _hip(), _batch(c)
    K, p = c.K, cases.FTRL
    a = dict(w=_cuda(cases.table(c)).view(-1), keys=b.keys, vals=b.vals,
             ptr=b.ptr, labels=b.labels, wts=b.wts,
             err=torch.zeros(c.B * K, device="cuda"),
             loss=torch.zeros(c.B, device="cuda"), K=K)
    a.update(bad)
    csr = (a["w"], a["keys"], a["vals"], a["ptr"])
    fwd = csr + (a["labels"], a["wts"], a["err"], a["loss"])
    ftrl = (p["alpha"], p["beta"], p["l1"], p["l2"], a["K"])
    if entry == "sigmoid_forward":
        hip.lr_sigmoid_forward(*fwd)
    elif entry == "softmax_forward":
        hip.lr_softmax_forward(*fwd, a["K"])
    elif entry == "ftrl_forward":
        hip.lr_ftrl_forward(*fwd, *ftrl)
    elif entry == "sigmoid_scatter":
        hip.lr_sigmoid_scatter(*csr, a["err"], cases.LR, 0, 0.0)
    elif entry == "softmax_scatter":
        hip.lr_softmax_scatter(*csr, a["err"], cases.LR, 0, 0.0, a["K"])
    else:
        hip.lr_ftrl_scatter(*csr, a["err"], *ftrl)


ENTRIES = ["sigmoid_forward", "softmax_forward", "ftrl_forward",
           "sigmoid_scatter", "softmax_scatter", "ftrl_scatter"]


def _entry_case(entry):
    if entry.startswith("ftrl"):
        return cases.ftrl(3, True)
    return cases.sparse(*(("sigmoid", 1) if entry.startswith("sigmoid")
                          else ("softmax", 3)), True)


def _bad_csr(c):
    """One offending keys / vals / ptr tensor each."""
    n, m = len(c.keys), len(c.ptr)
    keys, ptr = torch.from_numpy(c.keys), torch.from_numpy(c.ptr)
    strided_keys = torch.zeros(2 * n, dtype=torch.int64, device="cuda")[::2]
    strided_ptr = torch.zeros(2 * m, dtype=torch.int32, device="cuda")[::2]
    return {
        "keys on the CPU": dict(keys=keys),
        "strided keys": dict(keys=strided_keys),
        "int32 keys": dict(keys=keys.to(torch.int32).cuda()),
        "ptr on the CPU": dict(ptr=ptr),
        "strided ptr": dict(ptr=strided_ptr),
        "int64 ptr": dict(ptr=ptr.long().cuda()),
        "empty ptr": dict(ptr=torch.empty(0, dtype=torch.int32,
                                          device="cuda")),
        "one value short": dict(vals=torch.zeros(n - 1, device="cuda")),
    }


BAD_CSR = ["keys on the CPU", "strided keys", "int32 keys", "ptr on the CPU",
           "strided ptr", "int64 ptr", "empty ptr", "one value short"]


@pytest.mark.parametrize("what", BAD_CSR)
@pytest.mark.parametrize("entry", ENTRIES)
def test_refuses_bad_csr(entry, what):
    c = _entry_case(entry)
    bad = _bad_csr(c)
    assert sorted(bad) == sorted(BAD_CSR)
    with pytest.raises(RuntimeError):
        _call(entry, c, **bad[what])


@pytest.mark.parametrize("entry", ENTRIES)
def test_refuses_err_of_wrong_size(entry):
    c = _entry_case(entry)
    with pytest.raises(RuntimeError):
        _call(entry, c, err=torch.zeros(c.B * c.K + 1, device="cuda"))


def test_ftrl_forward_refuses_wts_of_wrong_size():
    c = cases.ftrl(3, True)
    with pytest.raises(RuntimeError):
        _call("ftrl_forward", c, wts=torch.ones(c.B - 1, device="cuda"))


@pytest.mark.parametrize("entry,K", [
    ("softmax_scatter", 1), ("softmax_scatter", 65), ("softmax_forward", 65),
    ("ftrl_scatter", 0), ("ftrl_scatter", 33), ("ftrl_forward", 33)])
def test_refuses_class_count_out_of_range(entry, K):
    """err and the table are sized for the K asked for, so that K alone
    offends."""
    c = _entry_case(entry)
    cols = K * (2 if entry.startswith("ftrl") else 1)
    with pytest.raises(RuntimeError):
        _call(entry, c, K=K, err=torch.zeros(c.B * K, device="cuda"),
              w=torch.zeros(c.rows * max(cols, 1), device="cuda"))


@pytest.mark.parametrize("entry", ["softmax_forward", "softmax_scatter",
                                   "ftrl_forward", "ftrl_scatter"])
def test_refuses_table_of_broken_rows(entry):
    c = _entry_case(entry)
    n = cases.table(c).size
    with pytest.raises(RuntimeError):
        _call(entry, c, w=torch.zeros(n + 1, device="cuda"))
