"""GPU tests of k_w2v / k_w2v_ns against the fp64 oracle (w2v_oracle.py) on
the inputs of w2v_cases.py: every register bucket and all four variants of
the ragged kernel, a launch larger than the grid, the in-kernel negative
sampler, several groups of negative sampling, the rate the model hands to
the kernels, and the bindings' refusal of tensors the kernels cannot read.

Each comparison covers the whole of all four buffers. Per buffer the kernel
must be within max(8 * err_ref, 4 * eps * max|oracle|) of the oracle, where
err_ref is the distance of the sequential fp32 reference _w2v_train_torch
from the oracle (w2v_cases.bound); rows no group names must come back
bit-identical, and so must the accumulators when adagrad is off. The
measured figures are in profiles/w2v_oracle.md."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2v_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["in_buf", "out_buf", "in_gsq", "out_gsq"]
VARIANTS = [(False, False), (False, True), (True, False), (True, True)]
VARIANT_IDS = ["plain-hogwild", "plain-atomic", "adagrad-hogwild",
               "adagrad-atomic"]


def _hip():
    from multiverso_amd import ops
    return ops.module(required=True)


def _t(x, dtype):
    return torch.tensor(x, dtype=dtype, device="cuda")


def _reference(c, adagrad):
    """(oracle buffers, fp32 torch reference buffers) of a case; without
    adagrad the accumulators are expected unchanged. Computed once per
    case and variant and left unchanged."""
    cache = c.__dict__.setdefault("_refs", {})
    if adagrad not in cache:
        from multiverso_amd.apps.wordembedding.model import _w2v_train_torch
        want = list(cases.run_oracle(c, adagrad))
        if adagrad:
            # every element is compared, so none may sit on the threshold
            assert want[4] > 1e-3, want[4]
        else:
            want[2] = c.in_gsq.astype(np.float64)
            want[3] = c.out_gsq.astype(np.float64)
        ref = [torch.from_numpy(x.copy())
               for x in (c.in_buf, c.out_buf, c.in_gsq, c.out_gsq)]
        _w2v_train_torch(ref[0], ref[1], ref[2] if adagrad else None,
                         ref[3] if adagrad else None,
                         torch.tensor(c.in_idx, dtype=torch.int64),
                         torch.tensor(c.in_off, dtype=torch.int32),
                         torch.tensor(c.out_idx, dtype=torch.int64),
                         torch.tensor(c.out_label, dtype=torch.float32),
                         torch.tensor(c.out_off, dtype=torch.int32),
                         c.lr, adagrad, c.lr)
        cache[adagrad] = (want[:4], [r.numpy() for r in ref])
    return cache[adagrad]


def _device_buffers(c):
    return [torch.from_numpy(x.copy()).cuda()
            for x in (c.in_buf, c.out_buf, c.in_gsq, c.out_gsq)]


def _check(c, got, adagrad, label):
    """Whole-buffer comparison of the kernel's four buffers."""
    want, ref = _reference(c, adagrad)
    before = (c.in_buf, c.out_buf, c.in_gsq, c.out_gsq)
    unnamed = (c.unnamed_in, c.unnamed_out, c.unnamed_in, c.unnamed_out)
    failures = []
    for k, name in enumerate(NAMES):
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape
        if k >= 2 and not adagrad:
            assert np.array_equal(g.view(np.int32), before[k].view(np.int32)), \
                f"{label}: {name} changed without adagrad"
            continue
        err_ref, tol = cases.bound(ref[k], want[k])
        err = float(np.max(np.abs(g.astype(np.float64) - want[k])))
        print(f"W2V_ORACLE {label} {name} err={err:.3e} err_ref={err_ref:.3e} "
              f"tol={tol:.3e}")
        if not err <= tol:      # also catches NaN
            failures.append((name, err, err_ref, tol))
        assert np.array_equal(g[unnamed[k]].view(np.int32),
                              before[k][unnamed[k]].view(np.int32)), \
            f"{label}: an unnamed row of {name} changed"
    assert not failures, (label, failures)


def _run_ragged(c, adagrad, atomic):
    cases.assert_row_disjoint(c)
    got = _device_buffers(c)
    _hip().w2v_train(got[0], got[1], got[2], got[3],
                     _t(c.in_idx, torch.int64), _t(c.in_off, torch.int32),
                     _t(c.out_idx, torch.int64),
                     _t(c.out_label, torch.float32),
                     _t(c.out_off, torch.int32), c.lr, adagrad, atomic)
    torch.cuda.synchronize()
    return got


def _run_ns(c, adagrad, atomic, with_off=True):
    cases.assert_row_disjoint(c)
    if not with_off:
        assert c.in_off == list(range(len(c.centers) + 1))
    got = _device_buffers(c)
    _hip().w2v_train_ns(got[0], got[1], got[2], got[3],
                        _t(c.in_idx, torch.int64),
                        _t(c.in_off, torch.int32) if with_off else None,
                        _t(c.centers, torch.int64), _t(c.pool, torch.int64),
                        c.neg, c.seed, c.lr, adagrad, atomic)
    torch.cuda.synchronize()
    return got


# ---- ragged k_w2v: every bucket, all four variants --------------------------

_ragged = functools.lru_cache(maxsize=None)(cases.ragged)


@pytest.mark.parametrize("adagrad,atomic", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("dim", cases.RAGGED_DIMS)
def test_ragged_all_buckets(dim, adagrad, atomic):
    c = _ragged(dim)
    got = _run_ragged(c, adagrad, atomic)
    _check(c, got, adagrad, f"ragged dim={dim} ada={adagrad} atom={atomic}")
    if adagrad and cases.zero_columns(dim):
        # 0 * rsqrt(0) must not reach the weights
        zc = cases.zero_columns(dim)
        named = sorted(set(c.out_idx))
        assert torch.all(got[3][named][:, zc] == 0)
        assert torch.equal(got[1][named][:, zc].cpu(),
                           torch.from_numpy(c.out_buf[named][:, zc]))


# ---- more groups than the grid has waves ------------------------------------

_grid = functools.lru_cache(maxsize=None)(cases.grid_stride)


@pytest.mark.parametrize("adagrad,atomic", [(False, False), (True, True)],
                         ids=["plain-hogwild", "adagrad-atomic"])
def test_grid_stride_ragged(adagrad, atomic):
    c = _grid(False)
    assert len(c.in_off) - 1 == cases.GRID_G > 8192
    got = _run_ragged(c, adagrad, atomic)
    _check(c, got, adagrad, f"grid k_w2v ada={adagrad} atom={atomic}")


@pytest.mark.parametrize("with_off", [True, False], ids=["in_off", "no_off"])
def test_grid_stride_ns(with_off):
    """neg = 0: only the centre is scored, so the groups stay disjoint."""
    c = _grid(not with_off)
    assert len(c.centers) == cases.GRID_G > 8192 and c.neg == 0
    got = _run_ns(c, False, False, with_off)
    _check(c, got, False, f"grid k_w2v_ns in_off={with_off}")


# ---- the in-kernel sampler --------------------------------------------------

_sampler = functools.lru_cache(maxsize=None)(cases.sampler)


@pytest.mark.parametrize("adagrad,atomic", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("seed", cases.SAMPLER_SEEDS, ids=["seed1", "seed2p62"])
def test_ns_sampler_mapping(seed, adagrad, atomic):
    """One group, three pool rows, eight draws: stream start, recurrence,
    shift and modulus decide which row is hit how often. The draws repeat
    rows, so in the atomic variants a row is reloaded after atomicAdd."""
    c = _sampler(seed)
    import w2v_oracle as oracle
    draws = oracle.ns_draws(seed, 0, c.neg, len(c.pool))
    assert draws == cases.SAMPLER_DRAWS[seed]
    assert c.out_idx == [0] + [c.pool[p] for p in draws]
    for with_off in (True, False):
        got = _run_ns(c, adagrad, atomic, with_off)
        _check(c, got, adagrad, f"sampler seed={seed} ada={adagrad} "
                                f"atom={atomic} in_off={with_off}")


# ---- negative sampling over several groups ----------------------------------

# the variants of one case run back to back, so two cases are enough to keep
_ns_multi = functools.lru_cache(maxsize=2)(cases.ns_multi)


@pytest.mark.parametrize("adagrad,atomic", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("start_seed", cases.SAMPLER_SEEDS,
                         ids=["small", "large"])
@pytest.mark.parametrize("cbow", [False, True], ids=["skipgram", "cbow"])
@pytest.mark.parametrize("dim", cases.NS_DIMS)
def test_ns_multi_group(dim, cbow, start_seed, adagrad, atomic):
    """24 groups with their own streams; three of them draw their own
    centre, which is skipped but consumes the draw."""
    c = _ns_multi(dim, cbow, start_seed)
    lens = np.diff(c.out_off)
    for g in cases.NS_SKIP_GROUPS:
        assert lens[g] < 1 + c.neg
    got = _run_ns(c, adagrad, atomic, with_off=cbow)
    _check(c, got, adagrad, f"ns_multi dim={dim} cbow={cbow} seed={c.seed} "
                            f"ada={adagrad} atom={atomic}")


# ---- the rate the model passes ----------------------------------------------

def _model(adagrad, **kw):
    import multiverso_amd as mv
    from multiverso_amd.apps.wordembedding.model import (WordEmbedding,
                                                         WordEmbeddingOption)
    mv.init()
    opt = WordEmbeddingOption(embedding_size=64, negative_num=8,
                              init_learning_rate=cases.LR,
                              use_adagrad=adagrad, unigram_table_size=1000,
                              total_words=1000, **kw)
    model = WordEmbedding(opt, [10] * 8)
    model.learning_rate = 0.25 * opt.init_learning_rate
    return mv, model


def _with_rate(c, lr):
    d = cases.SimpleNamespace(**{k: v for k, v in c.__dict__.items()
                                 if k != "_refs"})
    d.lr = lr
    return d


@pytest.mark.parametrize("adagrad", [False, True], ids=["plain", "adagrad"])
def test_model_rate_ragged(adagrad):
    """_train_kernel with a decayed model.learning_rate: adagrad steps by
    init_learning_rate, the plain step by the decayed rate."""
    mv, model = _model(adagrad)
    try:
        lr = model.opt.init_learning_rate if adagrad else model.learning_rate
        c = _with_rate(_ragged(200), lr)
        got = _device_buffers(c)
        model._train_kernel(got[0], got[1],
                            got[2] if adagrad else None,
                            got[3] if adagrad else None,
                            _t(c.in_idx, torch.int64),
                            _t(c.in_off, torch.int64),
                            _t(c.out_idx, torch.int64),
                            _t(c.out_label, torch.float32),
                            _t(c.out_off, torch.int64))
        torch.cuda.synchronize()
        _check(c, got, adagrad, f"model ragged ada={adagrad}")
    finally:
        mv.shutdown()


@pytest.mark.parametrize("adagrad", [False, True], ids=["plain", "adagrad"])
def test_model_rate_ns(adagrad):
    mv, model = _model(adagrad)
    try:
        lr = model.opt.init_learning_rate if adagrad else model.learning_rate
        state = model._seed_state
        seed = model._next_seed()       # the seed the launch will use
        model._seed_state = state
        c = _with_rate(cases.sampler(seed), lr)
        got = _device_buffers(c)
        model._train_kernel_ns(got[0], got[1],
                               got[2] if adagrad else None,
                               got[3] if adagrad else None,
                               _t(c.in_idx, torch.int64), None,
                               _t(c.centers, torch.int64),
                               _t(c.pool, torch.int64))
        torch.cuda.synchronize()
        _check(c, got, adagrad, f"model ns ada={adagrad}")
    finally:
        mv.shutdown()


# ---- tensors the kernels cannot read are refused before any launch ----------

def _refusal_args(c):
    return dict(in_idx=_t(c.in_idx, torch.int64),
                in_off=_t(c.in_off, torch.int32),
                out_idx=_t(c.out_idx, torch.int64),
                out_label=_t(c.out_label, torch.float32),
                out_off=_t(c.out_off, torch.int32))


def _strided(t):
    """A non-contiguous GPU view holding exactly t's values."""
    wide = torch.zeros(t.numel(), 2, dtype=t.dtype, device=t.device)
    wide[:, 0] = t
    v = wide[:, 0]
    assert not v.is_contiguous() or t.numel() <= 1
    return v


def _assert_unchanged(c, got):
    torch.cuda.synchronize()
    for k, x in enumerate((c.in_buf, c.out_buf, c.in_gsq, c.out_gsq)):
        assert np.array_equal(got[k].cpu().numpy().view(np.int32),
                              x.view(np.int32)), NAMES[k]


@pytest.mark.parametrize("how", ["strided", "cpu"])
@pytest.mark.parametrize("which", ["in_idx", "in_off", "out_idx",
                                   "out_label", "out_off"])
def test_w2v_train_refuses(which, how):
    c = _ragged(64)
    a = _refusal_args(c)
    a[which] = _strided(a[which]) if how == "strided" else a[which].cpu()
    got = _device_buffers(c)
    with pytest.raises(RuntimeError):
        _hip().w2v_train(got[0], got[1], got[2], got[3], a["in_idx"],
                         a["in_off"], a["out_idx"], a["out_label"],
                         a["out_off"], c.lr, True, False)
    _assert_unchanged(c, got)


@pytest.mark.parametrize("how", ["strided", "cpu"])
@pytest.mark.parametrize("which", ["in_idx", "in_off", "centers", "pool"])
def test_w2v_train_ns_refuses(which, how):
    c = _sampler(1)
    a = dict(in_idx=_t(c.in_idx * 2, torch.int64),
             in_off=_t([0, 1, 2], torch.int32),
             centers=_t(c.centers * 2, torch.int64),
             pool=_t(c.pool, torch.int64))
    a[which] = _strided(a[which]) if how == "strided" else a[which].cpu()
    got = _device_buffers(c)
    with pytest.raises(RuntimeError):
        _hip().w2v_train_ns(got[0], got[1], got[2], got[3], a["in_idx"],
                            a["in_off"], a["centers"], a["pool"], c.neg,
                            c.seed, c.lr, True, False)
    _assert_unchanged(c, got)


def test_w2v_train_ns_refuses_bad_counts():
    c = _sampler(1)
    got = _device_buffers(c)
    args = (_t(c.in_idx, torch.int64), _t(c.in_off, torch.int32),
            _t(c.centers, torch.int64), _t(c.pool, torch.int64))
    with pytest.raises(RuntimeError):           # neg < 0
        _hip().w2v_train_ns(got[0], got[1], got[2], got[3], *args, -1,
                            c.seed, c.lr, False, False)
    with pytest.raises(RuntimeError):           # empty in_off
        _hip().w2v_train_ns(got[0], got[1], got[2], got[3], args[0],
                            _t([], torch.int32),
                            _t([], torch.int64), args[3], c.neg, c.seed,
                            c.lr, False, False)
    with pytest.raises(RuntimeError):
        _hip().w2v_train(got[0], got[1], got[2], got[3], args[0],
                         _t([], torch.int32), _t(c.out_idx, torch.int64),
                         _t(c.out_label, torch.float32),
                         _t([], torch.int32), c.lr, False, False)
    _assert_unchanged(c, got)
