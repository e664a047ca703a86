"""Inputs of the logistic-regression oracle tests, shared by
test_lr_oracle.py (which checks their properties on the CPU) and
test_gpu_lr_oracle.py (which runs them through the kernels). Nothing here
imports multiverso_amd; expected values come from lr_oracle.py alone.

Every case is seeded, built once (lru_cache) and left unchanged. A case is a
SimpleNamespace: the CSR batch (keys int64, vals fp32, ptr int32, labels,
wts or None), the weights W [rows, K] or the FTRL state zn [rows, 2K], and
`unnamed`, the two trailing rows no key names."""

import functools
from types import SimpleNamespace

import numpy as np

import lr_oracle as oracle
from w2v_cases import EPS32, bound  # noqa: F401  (the project's one rule)

B_REGULAR = 40
REQUIRED_LENGTHS = [0, 1, 63, 64, 65, 128, 129, 200]
SOFTMAX_KS = list(range(2, 17)) + [17, 32, 33, 63, 64]
FTRL_KS = list(range(1, 17)) + [17, 32]
FTRL_WEIGHTED_KS = (1, 3, 17)
REG_KS = [3, 17]
LR = 0.05
REG_COEF = 0.01
MARGIN = 1e-3               # distance every sign / threshold decision keeps
W_SCALE = 1.5               # scores ~ N(0, 1.5^2): |s| stays below about 6
FTRL = dict(alpha=0.5, beta=0.5, l1=0.3, l2=0.01)

# The grids cap at these many waves (kernels.hip: grid_for at 2048 blocks of
# 4 waves; k_lr_dense_post at 512 blocks of 4; k_lr_dense_fwd at 256 blocks
# of 16): 37 samples more take the loop's second trip.
GRID_B = 8192 + 37
GRID_B_POST = 2048 + 37
GRID_B_DENSE = 4096 + 37

DENSE_KS = list(range(1, 17))
DENSE_EDGE_DS = [1, 63, 64, 65]
DENSE_EDGE_KS = [1, 2, 16]
POST_KS = [1, 2, 16, 17, 32, 33, 63, 64]
SAT_SCORES = [30.0, -30.0, 100.0, -100.0]
SAT_LIMIT = 8.0


def _lengths(rng, B=B_REGULAR):
    lens = REQUIRED_LENGTHS + list(rng.randint(0, 13, B - len(REQUIRED_LENGTHS)))
    return [int(n) for n in rng.permutation(lens)]


def _labels(rng, B, K):
    """Class labels (0/1 at K == 1) that cover class 0 and class K-1."""
    y = rng.randint(0, max(K, 2), B)
    y[0], y[1] = 0, max(K, 2) - 1
    return y.astype(np.float32)


def _wts(rng, B):
    return (rng.random_sample(B) + 0.5).astype(np.float32)


def _batch(rng, lens, rows, K, weighted, unique):
    """CSR batch over `rows` named rows plus two unnamed ones; vals scaled
    by 1/sqrt(len). unique: no row is named twice in the whole batch."""
    nnz = sum(lens)
    c = SimpleNamespace(K=K, B=len(lens))
    c.ptr = np.cumsum([0] + lens).astype(np.int32)
    if unique:
        assert rows >= nnz
        c.keys = rng.permutation(rows)[:nnz].astype(np.int64)
    else:
        c.keys = rng.randint(0, rows, nnz).astype(np.int64)
    scale = np.repeat(1 / np.sqrt(np.maximum(lens, 1)), lens)
    c.vals = (rng.standard_normal(nnz) * scale).astype(np.float32)
    c.labels = _labels(rng, c.B, K)
    c.wts = _wts(rng, c.B) if weighted else None
    c.rows = rows + 2
    c.unnamed = [rows, rows + 1]
    c.unique = unique
    return c


def _weights(rng, rows, K):
    return (rng.standard_normal((rows, K)) * W_SCALE).astype(np.float32)


def _ftrl_state(rng, rows, K):
    """(z | n): |z| keeps MARGIN from l1 with both sides present, n >= 0
    but for five small negative entries (the clamp)."""
    l1 = FTRL["l1"]
    z = rng.standard_normal((rows, K)) * W_SCALE
    near = np.abs(np.abs(z) - l1) < 2 * MARGIN
    z[near] = np.sign(z[near]) * (l1 + 4 * MARGIN)
    z.flat[0], z.flat[1] = 0.5 * l1, -3 * l1        # both sides, always
    n = rng.random_sample((rows, K)) * 0.25
    n.flat[rng.choice(n.size, 5, replace=False)] = -1e-3
    return np.concatenate([z, n], 1).astype(np.float32)


def assert_ftrl_margins(c):
    K, l1 = c.K, FTRL["l1"]
    z, n = c.zn[:, :K].astype(np.float64), c.zn[:, K:]
    assert np.all(np.abs(np.abs(z) - l1) >= MARGIN)
    assert np.any(np.abs(z) > l1) and np.any(np.abs(z) < l1)
    assert 1 <= np.sum(n < 0) <= 5 and np.all(n >= -1e-3)


def assert_l1_margins(c):
    nz = c.W != 0
    assert np.any(~nz) and np.all(np.abs(c.W[nz]) >= MARGIN)


# ---- the sparse cases ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sparse(kind, K, weighted, unique=False):
    """The regular ragged batch of 40 samples. kind: sigmoid | softmax."""
    rng = np.random.RandomState(
        [{"sigmoid": 1, "softmax": 2}[kind], K, weighted, unique])
    lens = _lengths(rng)
    rows = sum(lens) if unique else 300
    c = _batch(rng, lens, rows, K, weighted, unique)
    c.kind = kind
    c.W = _weights(rng, c.rows, K)
    return c


@functools.lru_cache(maxsize=None)
def sparse_l1(kind, K):
    """Unique keys; a tenth of the weights exactly 0.0 (sign 0), every other
    at least MARGIN from it."""
    base = sparse(kind, K, True, True)
    c = SimpleNamespace(**base.__dict__)
    rng = np.random.RandomState([7, K])
    W = base.W.copy()
    small = np.abs(W) < MARGIN
    W[small] = np.where(W[small] < 0, -MARGIN, MARGIN)
    W[rng.random_sample(W.shape) < 0.1] = 0.0
    W[c.keys[0]] = 0.0                  # a named row, for certain
    c.W = W
    assert_l1_margins(c)
    return c


@functools.lru_cache(maxsize=None)
def ftrl(K, weighted):
    rng = np.random.RandomState([3, K, weighted])
    lens = _lengths(rng)
    c = _batch(rng, lens, sum(lens), K, weighted, True)
    c.kind = "ftrl"
    c.zn = _ftrl_state(rng, c.rows, K)
    assert_ftrl_margins(c)
    return c


@functools.lru_cache(maxsize=None)
def grid(kind):
    """GRID_B samples of 0..3 features, unique keys: 37 waves take a second
    trip of the sample loop. sigmoid, softmax K=3, ftrl K=2."""
    K = {"sigmoid": 1, "softmax": 3, "ftrl": 2}[kind]
    rng = np.random.RandomState([4, K])
    lens = [int(n) for n in rng.randint(0, 4, GRID_B)]
    c = _batch(rng, lens, sum(lens), K, True, True)
    c.kind = kind
    if kind == "ftrl":
        c.zn = _ftrl_state(rng, c.rows, K)
        assert_ftrl_margins(c)
    else:
        c.W = _weights(rng, c.rows, K)
    return c


@functools.lru_cache(maxsize=None)
def saturated(kind):
    """The regular batch with four more samples of one feature (value 1)
    each, whose rows put a score at +30, -30, +100 and -100; both labels
    occur among them. sigmoid, softmax K=5, ftrl K=3."""
    K = {"sigmoid": 1, "softmax": 5, "ftrl": 3}[kind]
    rng = np.random.RandomState([5, K])
    lens = _lengths(rng) + [1] * len(SAT_SCORES)
    c = _batch(rng, lens, sum(lens), K, True, True)
    c.kind = kind
    c.sat = list(range(B_REGULAR, B_REGULAR + len(SAT_SCORES)))
    c.vals[c.ptr[c.sat]] = 1.0
    sat_rows = c.keys[c.ptr[c.sat]]
    c.labels[c.sat] = [0, 0, 1, 1] if K == 1 else [0, 1, 1, 0]
    if kind == "ftrl":
        c.zn = _ftrl_state(rng, c.rows, K)
        p = FTRL
        for r, s in zip(sat_rows, SAT_SCORES):
            # z that reconstructs to w = s in output 1 % K; 0 elsewhere
            c.zn[r, :K], c.zn[r, K:] = 0.0, 0.04
            c.zn[r, 1 % K] = -s * ((p["beta"] + 0.2) / p["alpha"] + p["l2"]) \
                - np.sign(s) * p["l1"]
        assert_ftrl_margins(c)
    else:
        c.W = _weights(rng, c.rows, K)
        for r, s in zip(sat_rows, SAT_SCORES):
            c.W[r] = 0.0
            c.W[r, 1 % K] = s
    # the rule below leaves out exactly the four: a regular sample that
    # comes near the limit by chance has its values halved
    while True:
        near = np.flatnonzero(_gap(c, _forward_on(c, table(c), False)["s"])
                              [:B_REGULAR] > 0.75 * SAT_LIMIT)
        if not len(near):
            return c
        for i in near:
            c.vals[c.ptr[i]:c.ptr[i + 1]] *= np.float32(0.5)


def _gap(c, s):
    s = np.asarray(s).reshape(c.B, -1)
    return (s.max(1) - s.min(1)) if c.kind == "softmax" else np.abs(s).max(1)


def unsaturated(c, s):
    """The samples whose loss is compared: |s| <= 8 (softmax: the largest
    gap between two logits <= 8). Exactly the constructed ones fall out."""
    keep = _gap(c, s) <= SAT_LIMIT
    assert sorted(np.flatnonzero(~keep)) == c.sat, np.flatnonzero(~keep)
    return keep


# ---- the dense cases ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dense(K, d, B, weighted):
    """X [B, d] scaled by 1/sqrt(d), W [d, K]."""
    rng = np.random.RandomState([6, K, d, B, weighted])
    c = SimpleNamespace(K=K, d=d, B=B)
    c.X = (rng.standard_normal((B, d)) / np.sqrt(d)).astype(np.float32)
    c.W = _weights(rng, d, K)
    c.labels = _labels(rng, B, K)
    c.wts = _wts(rng, B) if weighted else None
    return c


@functools.lru_cache(maxsize=None)
def post(K, B, weighted):
    """Logits [B, K] for k_lr_dense_post."""
    rng = np.random.RandomState([8, K, B, weighted])
    c = SimpleNamespace(K=K, B=B)
    c.logits = (rng.standard_normal((B, K)) * 2).astype(np.float32)
    c.labels = _labels(rng, B, K)
    c.wts = _wts(rng, B) if weighted else None
    return c


def n_chain(B, waves_per_block, max_blocks):
    """Additions on the longest path of the dense kernels' loss: a wave adds
    its samples, a block its waves (LDS atomics), the grid its blocks
    (global atomics). blocks: one wave per sample, capped."""
    blocks = min(-(-B // waves_per_block), max_blocks)
    per_wave = -(-B // (blocks * waves_per_block))
    return per_wave + waves_per_block + blocks


def mean_tol(loss_tol, want_mean, chain):
    """Tolerance of a batch-mean loss summed in fp32 in an unknown order: a
    mean of per-sample errors cannot exceed their maximum (loss_tol), and
    `chain` additions of positive terms lose at most chain * 2^-24 of the
    sum (the classical bound of recursive summation)."""
    return loss_tol + chain * 2.0 ** -24 * abs(want_mean)


# ---- expected values ------------------------------------------------------------

def _forward_on(c, table, lib32):
    """s, err [B, K] and loss [B] of case c's batch on `table` (W or zn)."""
    sfx = "32" if lib32 else ""
    if c.kind == "ftrl":
        table = getattr(oracle, "ftrl_weights" + sfx)(table, c.K, **FTRL)
    s = getattr(oracle, "scores" + sfx)(table, c.keys, c.vals, c.ptr)
    if c.kind == "sigmoid":
        err, loss = getattr(oracle, "sigmoid_fwd" + sfx)(
            s[:, 0], c.labels, c.wts)
        err = err[:, None]
    else:
        err, loss = getattr(oracle, c.kind + "_fwd" + sfx)(
            s, c.labels, c.wts)
    return dict(s=s, err=err, loss=loss)


def _scatter_on(c, table, err, lr, reg_type, lib32):
    sfx = "32" if lib32 else ""
    if c.kind == "ftrl":
        return getattr(oracle, "ftrl_scatter" + sfx)(
            table, c.keys, c.vals, c.ptr, err, c.K, **FTRL)
    return getattr(oracle, "scatter" + sfx)(
        table, c.keys, c.vals, c.ptr, err, lr, reg_type, REG_COEF)


def table(c):
    return c.zn if c.kind == "ftrl" else c.W


def forward(c):
    """(oracle, fp32 reference) of a sparse forward, each a dict of s, err
    [B, K] and loss [B]. Computed once per case."""
    if "_fwd" not in c.__dict__:
        c._fwd = tuple(_forward_on(c, table(c), lib32)
                       for lib32 in (False, True))
    return c._fwd


def oracle_err32(c):
    """The oracle's err rounded to fp32: the scatter tests' input, so that
    the scatter kernel is judged apart from the forward one."""
    return forward(c)[0]["err"].astype(np.float32)


def scatter(c, reg_type=0):
    """(oracle, fp32 reference) of the buffer after a scatter of
    oracle_err32(c). Computed once per case and reg_type."""
    cache = c.__dict__.setdefault("_scat", {})
    if reg_type not in cache:
        err = oracle_err32(c)
        cache[reg_type] = tuple(
            _scatter_on(c, table(c), err, LR, reg_type, lib32)
            for lib32 in (False, True))
    return cache[reg_type]


def chained(batches, table0, lrs, reg_type=0):
    """(oracle, fp32 reference) of forward-then-scatter over `batches` in
    turn, each on the table the one before left and with its own rate:
    (final table, [loss [B] per batch]). Nothing is rounded in between."""
    out = []
    for lib32 in (False, True):
        t, losses = table0, []
        for c, lr in zip(batches, lrs):
            f = _forward_on(c, t, lib32)
            losses.append(f["loss"])
            t = _scatter_on(c, t, f["err"], lr, reg_type, lib32)
        out.append((t, losses))
    return tuple(out)


# ---- the model-level cases -------------------------------------------------------

MODEL_LR0, MODEL_MB = 0.2, 16


def model_lrs(n):
    """The rates WorkerSGDSchedule hands out at learning_rate MODEL_LR0,
    learning_rate_coef 1 and minibatch_size MODEL_MB."""
    return [max(1e-3, MODEL_LR0 - t / MODEL_MB) for t in range(n)]


@functools.lru_cache(maxsize=None)
def model(kind, K):
    """Two minibatches of 16 samples over one table of 400 + 2 rows; keys
    are unique within a minibatch and shared between the two. Returns
    (batches, table0)."""
    rng = np.random.RandomState([9, K, len(kind)])
    rows, batches = 400, []
    for _ in range(2):
        lens = [0, 1, 65] + [int(n) for n in rng.randint(0, 13, MODEL_MB - 3)]
        c = _batch(rng, lens, rows, K, False, True)
        c.kind = kind
        batches.append(c)
    assert set(batches[0].keys) & set(batches[1].keys)
    if kind == "ftrl":
        t0 = _ftrl_state(rng, rows + 2, K)
        assert_ftrl_margins(SimpleNamespace(K=K, zn=t0))
    else:
        t0 = _weights(rng, rows + 2, K)
    return batches, t0
