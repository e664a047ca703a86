"""Independent oracle of the fused logistic-regression kernels (k_lr_* in
kernels.hip): plain numpy float64 written from the formulas, not from
apps/logreg/objective.py, and a sequential float32 reference of the same
operations whose distance from the oracle sets the tolerance
(w2v_cases.bound). Nothing here imports multiverso_amd or torch.

A sparse batch is CSR: sample i owns keys/vals[ptr[i]:ptr[i+1]]. Weights are
[rows, K]; FTRL state is [rows, 2K] with z in the first K columns and n in
the last K. reg_type: 0 none, 1 L1 (coef * sign(w)), 2 L2 (coef * w), both
evaluated on the weights before the update."""

import numpy as np

EPS = 1e-12
F32 = np.float32


def sample_ids(ptr):
    """The sample of every list entry."""
    ptr = np.asarray(ptr, dtype=np.int64)
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


# ---- fp64 oracle ------------------------------------------------------------

def _f64(*xs):
    return [None if x is None else np.asarray(x, dtype=np.float64) for x in xs]


def scores(W, keys, vals, ptr):
    """s[i, k] = sum_j vals[j] * W[keys[j], k], entries added in list order."""
    W, vals = _f64(W, vals)
    s = np.zeros((len(ptr) - 1, W.shape[1]))
    np.add.at(s, sample_ids(ptr), vals[:, None] * W[np.asarray(keys)])
    return s


def ftrl_weights(zn, K, alpha, beta, l1, l2):
    """[rows, K] weights of a (z | n) state."""
    zn, = _f64(zn)
    z, n = zn[:, :K], zn[:, K:]
    w = (np.sign(z) * l1 - z) / ((beta + np.sqrt(np.maximum(n, 0))) / alpha
                                 + l2)
    return np.where(np.abs(z) > l1, w, 0.0)


def _nll(p, y):
    return -(y * np.log(p + EPS) + (1 - y) * np.log(1 - p + EPS))


def _wt(wts, B):
    return np.ones(B) if wts is None else _f64(wts)[0]


def sigmoid_fwd(s, labels, wts):
    """s [B] -> (err [B], loss [B])."""
    s, y = _f64(s, labels)
    with np.errstate(over="ignore"):
        p = 1 / (1 + np.exp(-s))
    return (p - y) * _wt(wts, len(s)), _nll(p, y)


def softmax_fwd(s, labels, wts):
    """s [B, K] -> (err [B, K], loss [B])."""
    s, = _f64(s)
    B, K = s.shape
    y = np.asarray(labels).astype(np.int64)
    e = np.exp(s - s.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    onehot = np.zeros((B, K))
    onehot[np.arange(B), y] = 1
    return ((p - onehot) * _wt(wts, B)[:, None],
            -np.log(p[np.arange(B), y] + EPS))


def ftrl_targets(labels, K, dtype=np.float64):
    """y_k of the FTRL objective: the label itself at K == 1, else one-hot."""
    labels = np.asarray(labels)
    if K == 1:
        return labels.astype(dtype)[:, None]
    y = np.zeros((len(labels), K), dtype=dtype)
    y[np.arange(len(labels)), labels.astype(np.int64)] = 1
    return y


def ftrl_fwd(s, labels, wts):
    """A sigmoid per output; the loss is the binary NLL summed over all K."""
    s, = _f64(s)
    B, K = s.shape
    y = ftrl_targets(labels, K)
    with np.errstate(over="ignore"):
        p = 1 / (1 + np.exp(-s))
    return (p - y) * _wt(wts, B)[:, None], _nll(p, y).sum(1)


def _reg(W0, reg_type, coef):
    if reg_type == 1:
        return coef * np.sign(W0)
    if reg_type == 2:
        return coef * W0
    return np.zeros_like(W0)


def scatter(W, keys, vals, ptr, err, lr, reg_type=0, coef=0.0):
    """W[keys[j], k] -= lr * (vals[j] * err[i, k] + reg) for every (j, k);
    err is [B, K]. Returns the new weights."""
    W0, vals, err = _f64(W, vals, err)
    keys = np.asarray(keys)
    g = vals[:, None] * err[sample_ids(ptr)] + _reg(W0, reg_type, coef)[keys]
    W = W0.copy()
    np.subtract.at(W, keys, lr * g)
    return W


def ftrl_scatter(zn, keys, vals, ptr, err, K, alpha, beta, l1, l2):
    """z -= (sqrt(nc + g^2) - sqrt(nc)) / alpha * w - g and n += g^2 with
    g = vals[j] * err[i, k], nc = max(n, 0), for keys no two entries share."""
    zn0, vals, err = _f64(zn, vals, err)
    keys = np.asarray(keys)
    assert len(np.unique(keys)) == len(keys)
    w = ftrl_weights(zn0, K, alpha, beta, l1, l2)[keys]
    g = vals[:, None] * err[sample_ids(ptr)]
    nc = np.maximum(zn0[keys, K:], 0)
    zn = zn0.copy()
    zn[keys, :K] -= (np.sqrt(nc + g * g) - np.sqrt(nc)) / alpha * w - g
    zn[keys, K:] += g * g
    return zn


def dense_fwd(X, W, labels, wts):
    """(err [B, K], loss [B]) of s = X @ W; sigmoid at K == 1, else softmax."""
    X, W = _f64(X, W)
    return dense_post(X @ W, labels, wts)


def dense_post(s, labels, wts):
    s, = _f64(s)
    if s.shape[1] == 1:
        err, loss = sigmoid_fwd(s[:, 0], labels, wts)
        return err[:, None], loss
    return softmax_fwd(s, labels, wts)


# ---- sequential fp32 reference ----------------------------------------------
# Every value is a numpy float32 and every operation rounds to float32.
# Features accumulate in list order, classes in index order, and scatter
# entries apply in list order, each reading what the one before left.

def _f32(*xs):
    return [None if x is None else np.asarray(x, dtype=F32) for x in xs]


def scores32(W, keys, vals, ptr):
    W, vals = _f32(W, vals)
    s = np.zeros((len(ptr) - 1, W.shape[1]), dtype=F32)
    for i in range(len(ptr) - 1):
        acc = s[i]
        for j in range(ptr[i], ptr[i + 1]):
            acc += vals[j] * W[keys[j]]
    return s


def ftrl_weights32(zn, K, alpha, beta, l1, l2):
    zn, = _f32(zn)
    z, n = zn[:, :K], zn[:, K:]
    alpha_inv = F32(1.0 / alpha)
    w = (np.sign(z) * F32(l1) - z) / (
        (F32(beta) + np.sqrt(np.maximum(n, F32(0)))) * alpha_inv + F32(l2))
    return np.where(np.abs(z) > F32(l1), w, F32(0))


def _nll32(p, y):
    one, eps = F32(1), F32(EPS)
    return -(y * np.log(p + eps) + (one - y) * np.log(one - p + eps))


def _sigmoid32(s):
    with np.errstate(over="ignore"):
        return F32(1) / (F32(1) + np.exp(-s))


def _wt32(wts, B):
    return np.ones(B, dtype=F32) if wts is None else _f32(wts)[0]


def sigmoid_fwd32(s, labels, wts):
    s, y = _f32(s, labels)
    p = _sigmoid32(s)
    return (p - y) * _wt32(wts, len(s)), _nll32(p, y)


def softmax_fwd32(s, labels, wts):
    s, = _f32(s)
    B, K = s.shape
    y = np.asarray(labels).astype(np.int64)
    e = np.exp(s - s.max(1, keepdims=True))
    se = np.zeros(B, dtype=F32)
    for k in range(K):
        se += e[:, k]
    p = e / se[:, None]
    onehot = np.zeros((B, K), dtype=F32)
    onehot[np.arange(B), y] = 1
    err = (p - onehot) * _wt32(wts, B)[:, None]
    loss = -np.log(p[np.arange(B), y] + F32(EPS))
    assert err.dtype == F32 and loss.dtype == F32
    return err, loss


def ftrl_fwd32(s, labels, wts):
    s, = _f32(s)
    B, K = s.shape
    y = ftrl_targets(labels, K, F32)
    p = _sigmoid32(s)
    nll = _nll32(p, y)
    loss = np.zeros(B, dtype=F32)
    for k in range(K):
        loss += nll[:, k]
    return (p - y) * _wt32(wts, B)[:, None], loss


def scatter32(W, keys, vals, ptr, err, lr, reg_type=0, coef=0.0):
    W0, vals, err = _f32(W, vals, err)
    reg = _reg(W0, reg_type, F32(coef)).astype(F32)
    W = W0.copy()
    lr = F32(lr)
    for i in range(len(ptr) - 1):
        for j in range(ptr[i], ptr[i + 1]):
            k = keys[j]
            W[k] += -lr * (vals[j] * err[i] + reg[k])
    assert W.dtype == F32
    return W


def ftrl_scatter32(zn, keys, vals, ptr, err, K, alpha, beta, l1, l2):
    zn, vals, err = _f32(zn, vals, err)
    zn = zn.copy()
    alpha_inv = F32(1.0 / alpha)
    for i in range(len(ptr) - 1):
        for j in range(ptr[i], ptr[i + 1]):
            row = zn[keys[j]]
            z, n = row[:K].copy(), row[K:].copy()
            w = ftrl_weights32(row[None, :], K, alpha, beta, l1, l2)[0]
            g = vals[j] * err[i]
            g2 = g * g
            nc = np.maximum(n, F32(0))
            row[:K] = z - (alpha_inv * (np.sqrt(nc + g2) - np.sqrt(nc)) * w
                           - g)
            row[K:] = n + g2
    assert zn.dtype == F32
    return zn


def dense_fwd32(X, W, labels, wts):
    X, W = _f32(X, W)
    s = np.zeros((X.shape[0], W.shape[1]), dtype=F32)
    for e in range(X.shape[1]):
        s += X[:, e, None] * W[e]
    return dense_post32(s, labels, wts)


def dense_post32(s, labels, wts):
    s, = _f32(s)
    if s.shape[1] == 1:
        err, loss = sigmoid_fwd32(s[:, 0], labels, wts)
        return err[:, None], loss
    return softmax_fwd32(s, labels, wts)
