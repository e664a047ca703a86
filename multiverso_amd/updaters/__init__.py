"""Server-side updaters — each a single fused CDNA4 HIP kernel on GPU.

Capability parity with the reference updater family (selected by the
``updater_type`` flag, src/updater/updater.cpp:46-57):

- default: ``data += delta``            (updater.cpp:22-29, K1)
- sgd:     ``data -= delta``            (sgd_updater.h:14-19, K2 — the
           worker pre-scales delta by lr)
- momentum:``m = mu*m + (1-mu)*delta; data -= m``
           (momentum_updater.h:17-25, K3)
- adagrad: ``g = delta/lr; G += g*g; data -= rho * g / sqrt(G + eps)``
           (adagrad_updater.h:23-41, K4). The reference decrements G and
           copies the accumulator row by value so the state update is lost
           (SURVEY.md §2.3 flags this as a bug to fix) — we keep the
           intended accumulate semantics. In the collective data plane the
           reduce-scattered delta is the sum over workers, so there is one
           accumulator per shard rather than one per (worker, shard).
- dcasgd / dcasgda: delay-compensated ASGD (selected at updater.cpp:51-54
           from a submodule absent in the snapshot; math from Zheng et
           al., ICML 2017) with per-worker backup rows.

One updater goes beyond the reference's set:

- adam:    Adam / AdamW as in ``torch.optim`` (``SparseAdam`` for keyed
           Adds): first and second moment per element, ONE update count
           per shard on the host, bias corrections passed to the kernel as
           scalars (``AdamUpdater``). float32 and float64 tables.

``AddOption`` keeps the reference's 20-byte wire envelope
(include/multiverso/updater/updater.h:10-70) for C-API parity; adam's
hyperparameters ride in the same five fields (``AddOption.adam``).

Updater state (momentum, accumulators, backups, Adam's moments and count)
lives with the updater and is NOT written by a table's ``store`` or by
``checkpoint``: a restored table resumes with fresh state.

Each updater's ``update`` is ONE pass over the shard: on GPU it dispatches
to the in-tree HIP extension (multiverso_amd.ops) — fused read-modify-write
kernels, float4-vectorized, grid-stride (memory-bound per the CDNA4 guide:
the bound is HBM3E bytes, so fusing m/G state updates into the same pass
halves traffic vs. composing torch ops). CPU fallback uses torch ops and
is numerically identical in fp32. Each whole-shard GPU pass runs in the
opposite direction to the one before it (``Updater._sweep``), which lets the
Infinity Cache serve the turning end of the shard and its state.

bf16 wire format (tables built with ``wire_dtype=torch.bfloat16``): on a
float32 shard every updater also takes a bfloat16 ``delta``, and
``update_and_copy`` a bfloat16 ``out``. The shard and all state stay fp32.
The HIP kernels widen the delta and narrow the Get buffer (round to nearest
even, bit for bit torch's cast) in registers, so no fp32 copy of the delta
exists on the GPU path; the CPU fallback runs the same torch ops on
``delta.float()``.
"""

from __future__ import annotations

import struct
from typing import Dict, Optional, Type

import torch


class AddOption:
    """20-byte (5 x 4B) add-option envelope; field order matches the
    reference union layout: worker_id(i), momentum(f), lr(f), rho(f),
    lambda(f)."""

    __slots__ = ("worker_id", "momentum", "learning_rate", "rho", "lambda_")

    def __init__(self, worker_id: int = 0, momentum: float = 0.0,
                 learning_rate: float = 0.01, rho: float = 0.1,
                 lambda_: float = 0.1) -> None:
        self.worker_id = worker_id
        self.momentum = momentum
        self.learning_rate = learning_rate
        self.rho = rho
        self.lambda_ = lambda_

    def to_bytes(self) -> bytes:
        return struct.pack("<iffff", self.worker_id, self.momentum,
                           self.learning_rate, self.rho, self.lambda_)

    @classmethod
    def from_bytes(cls, b: bytes) -> "AddOption":
        w, m, lr, rho, lam = struct.unpack("<iffff", b[:20])
        return cls(w, m, lr, rho, lam)

    @classmethod
    def adam(cls, lr: float = 1e-3, beta1: float = 0.9,
             beta2: float = 0.999, weight_decay: float = 0.0,
             worker_id: int = 0) -> "AddOption":
        """The option of an "adam" table. The envelope stays at five fields:
        lr rides in ``learning_rate``, beta1 in ``momentum``, beta2 in
        ``rho`` and the decoupled weight decay in ``lambda_``."""
        return cls(worker_id, beta1, lr, beta2, weight_decay)


def _widened(delta: torch.Tensor) -> torch.Tensor:
    """CPU fallback of the bf16 wire: the delta as fp32 (exact)."""
    return delta.float() if delta.dtype == torch.bfloat16 else delta


def _hip_ops():
    """In-tree HIP extension, or None on CPU-only hosts. On a GPU host a
    missing extension is a hard error (no silent eager fallback)."""
    from .. import ops
    return ops.module(required=torch.cuda.is_available())


_F32, _F64 = torch.float32, torch.float64


class Updater:
    """One rule, three forms: ``update`` (whole shard), ``update_and_copy``
    (whole shard, fused with the Get copy-out) and ``update_rows`` (the rows
    a keyed Add names). A subclass supplies

    - ``_resolve(option)``: its state tensors and its scalars for one update,
      in the order the kernels take them (the defaulting of ``option=None``
      lives there);
    - ``torch_step(w, *state, g, scalars)``: its formula in torch ops, in
      place — the fallback of all three forms;
    - the shard dtypes its HIP kernels cover, per form. Every other GPU
      shard, and every CPU shard, takes ``torch_step``.

    The extension's entry points are regular — ``X_update(data, *state,
    delta, *scalars, reverse=)``, ``X_copy_update(data, *state, delta, out,
    *scalars, reverse=)``, ``row_X_update(shard, *state, rows, vals,
    *scalars, perm)`` — so ``_hip_update`` and ``_hip_rows`` dispatch by
    ``name``; the updaters whose entry points differ override them."""

    name: str
    whole_dtypes = (_F32, _F64)
    fused_dtypes = (_F32,)
    keyed_dtypes = (_F32,)

    def __init__(self, shard: torch.Tensor) -> None:
        self.shard = shard
        # sweep direction of the next whole-shard GPU pass (see _sweep)
        self.reverse = False

    def _sweep(self) -> bool:
        """Direction for one whole-shard GPU launch; flips the parity.

        Consecutive passes over the shard (and its state) run in opposite
        directions, so the lines a pass touched last are the first the next
        pass touches, while the Infinity Cache still holds them. A hint
        only: the kernels compute the same bits either way. Row-keyed ops,
        store/load and the Get copy-out neither read nor flip it; the CPU
        fallbacks ignore it."""
        rev = self.reverse
        self.reverse = not rev
        return rev

    def _resolve(self, option: Optional[AddOption]):
        """(state tensors, scalars) of one update under ``option``."""
        raise NotImplementedError

    def _hip_update(self, state, delta: torch.Tensor,
                    out: Optional[torch.Tensor], scalars) -> None:
        """One whole-shard launch; with ``out`` the fused Add+Get kernel."""
        hip, rev = _hip_ops(), self._sweep()
        if out is None:
            getattr(hip, self.name + "_update")(
                self.shard, *state, delta, *scalars, reverse=rev)
        else:
            getattr(hip, self.name + "_copy_update")(
                self.shard, *state, delta, out, *scalars, reverse=rev)

    def _hip_rows(self, w, state, ids, vals, scalars,
                  assume_unique: bool) -> None:
        """k_row_update: value rows with the same id are summed in batch
        order, then one step per distinct row."""
        perm = None
        if not assume_unique:
            # equal ids adjacent, batch order kept inside each run; the
            # kernel reads the payload through perm, so vals stay put
            ids, perm = torch.sort(ids, stable=True)
        getattr(_hip_ops(), f"row_{self.name}_update")(
            w, *state, ids, vals, *scalars, perm)

    def _torch_rows(self, w, state, ids, vals, scalars) -> None:
        """The keyed semantics in torch ops: pre-sum duplicate rows, step
        the gathered rows of the distinct ids, write them back."""
        urows, inv = torch.unique(ids, return_inverse=True)
        g = torch.zeros(urows.numel(), vals.size(1), dtype=w.dtype,
                        device=w.device)
        g.index_add_(0, inv, vals)
        tensors = (w, *state)
        picked = [t[urows] for t in tensors]
        self.torch_step(*picked, g, scalars)
        for t, p in zip(tensors, picked):
            t[urows] = p

    def update(self, delta: torch.Tensor, option: Optional[AddOption]) -> None:
        state, scalars = self._resolve(option)
        if self.shard.is_cuda and self.shard.dtype in self.whole_dtypes:
            self._hip_update(state, delta, None, scalars)
        else:
            self.torch_step(self.shard, *state, _widened(delta), scalars)

    def update_and_copy(self, delta: torch.Tensor,
                        option: Optional[AddOption],
                        out: torch.Tensor) -> None:
        """Fused Add+Get (single-rank fast path): apply the update AND
        stream the updated shard into ``out`` in the same pass — saves
        the Get's shard re-read. Every updater has a fused HIP kernel;
        the fallback composes update + copy."""
        if self.shard.is_cuda and self.shard.dtype in self.fused_dtypes:
            state, scalars = self._resolve(option)
            self._hip_update(state, delta, out, scalars)
        else:
            self.update(delta, option)
            out.copy_(self.shard)

    def update_rows(self, local_ids: torch.Tensor, vals2d: torch.Tensor,
                    option: Optional[AddOption],
                    assume_unique: bool = False) -> None:
        """Row-keyed Add on the rows ``local_ids`` of the shard, seen as
        [rows, vals2d.size(1)] (the per-row updater dispatch of
        matrix_table.cpp:406-412). Duplicate ids of one batch are summed,
        then the rule steps once per distinct row; weights and state of
        other rows stay as they are. ``option`` defaults as in ``update``.
        A batch that brings this shard no rows is no update."""
        if not local_ids.numel():
            return
        from ..configure import get_flag
        if get_flag("deterministic") and not assume_unique:
            # fixed reduction order: pre-sum duplicate rows (sorted
            # segments) and update without atomics
            order = torch.argsort(local_ids, stable=True)
            v = vals2d[order]
            local_ids, counts = torch.unique_consecutive(
                local_ids[order], return_counts=True)
            # fp64 cumsum-diff segmented sum: fixed order, no atomics
            cs = torch.zeros(v.size(0) + 1, v.size(1), dtype=torch.float64,
                             device=v.device)
            torch.cumsum(v.to(torch.float64), 0, out=cs[1:])
            ends = counts.cumsum(0)
            # the shard's dtype, not v's: a bf16-wire sum stays fp32
            vals2d = (cs[ends] - cs[ends - counts]).to(self.shard.dtype)
            assume_unique = True
        cols = vals2d.size(1)
        state, scalars = self._resolve(option)
        w, state = self.shard.view(-1, cols), [s.view(-1, cols) for s in state]
        if self.shard.is_cuda and self.shard.dtype in self.keyed_dtypes:
            # a bf16-wire payload reaches the kernel as it is
            self._hip_rows(w, state, local_ids, vals2d.contiguous(), scalars,
                           assume_unique)
        else:
            self._torch_rows(w, state, local_ids, vals2d.to(w.dtype), scalars)

    def access(self, out: torch.Tensor) -> None:
        """K7: shard copy-out (updater.cpp:32-36)."""
        out.copy_(self.shard)


class DefaultUpdater(Updater):
    """``data += sign * delta``: no state, no scalars, and entry points of
    its own (K1/K2 whole, one signed fused kernel, the K5 scatter-add)."""

    name = "default"
    sign = 1.0
    whole_dtypes = (_F32, _F64, torch.int32, torch.int64)
    fused_dtypes = (_F32, _F64)

    def _resolve(self, option):
        return (), ()

    @staticmethod
    def torch_step(w: torch.Tensor, g: torch.Tensor, scalars) -> None:
        w.add_(g)

    def _hip_update(self, state, delta, out, scalars) -> None:
        hip, rev = _hip_ops(), self._sweep()
        if out is not None:
            hip.sgd_copy_update(self.shard, delta, out, self.sign,
                                reverse=rev)
        elif self.sign > 0:
            hip.add_inplace(self.shard, delta, reverse=rev)
        else:
            hip.sgd_update(self.shard, delta, reverse=rev)

    def _hip_rows(self, w, state, ids, vals, scalars, assume_unique) -> None:
        # atomic scatter-add: duplicates need no pre-sum
        _hip_ops().row_scatter_add(w, ids, vals, self.sign, assume_unique)

    def _torch_rows(self, w, state, ids, vals, scalars) -> None:
        w.index_add_(0, ids, vals * self.sign)


class SGDUpdater(DefaultUpdater):
    name = "sgd"
    sign = -1.0
    whole_dtypes = (_F32, _F64)

    @staticmethod
    def torch_step(w: torch.Tensor, g: torch.Tensor, scalars) -> None:
        w.sub_(g)


class MomentumUpdater(Updater):
    name = "momentum"

    def __init__(self, shard: torch.Tensor) -> None:
        super().__init__(shard)
        self.smooth_gradient = torch.zeros_like(shard)

    def _resolve(self, option):
        opt = option or AddOption()   # momentum defaults to 0.0
        return (self.smooth_gradient,), (float(opt.momentum),)

    @staticmethod
    def torch_step(w, m, g, scalars) -> None:
        mu, = scalars
        m.mul_(mu).add_(g, alpha=1.0 - mu)
        w.sub_(m)


class AdaGradUpdater(Updater):
    name = "adagrad"
    EPS = 1e-6

    def __init__(self, shard: torch.Tensor) -> None:
        super().__init__(shard)
        self.g_sqr = torch.zeros_like(shard)

    def _resolve(self, option):
        opt = option or AddOption()
        return (self.g_sqr,), (float(opt.learning_rate), float(opt.rho),
                               self.EPS)

    @staticmethod
    def torch_step(w, gsq, g, scalars) -> None:
        lr, rho, eps = scalars
        g = g / lr
        gsq.add_(g * g)
        w.sub_(rho * g / torch.sqrt(gsq + eps))

    def _hip_rows(self, w, state, ids, vals, scalars, assume_unique) -> None:
        # the keyed K15 kernel: duplicate rows race benignly via atomics
        # and keep the G accumulate, so no sort and no perm
        _hip_ops().row_scatter_adagrad(w, *state, ids, vals, *scalars,
                                       assume_unique)


class DCASGDUpdater(Updater):
    """DC-ASGD ("dcasgd", reference updater.cpp:51 — the updater itself
    lives in a submodule absent from the snapshot; math from Zheng et al.,
    "Asynchronous SGD with Delay Compensation", ICML 2017):

        w   -= lr * (g + lambda * g*g * (w - bak_k))
        bak_k = w

    ``bak_k`` is the per-worker backup of the weights worker k last
    synchronized (AddOption.worker_id selects the slot; worker_id < 0 —
    the collective merged-delta lane — uses one shared slot). Backups are
    lazily initialized to the shard's current values."""

    name = "dcasgd"
    whole_dtypes = (_F32,)

    def __init__(self, shard: torch.Tensor) -> None:
        super().__init__(shard)
        self._bak: Dict[int, torch.Tensor] = {}

    def _backup(self, worker_id: int) -> torch.Tensor:
        b = self._bak.get(worker_id)
        if b is None:
            b = self.shard.detach().clone()
            self._bak[worker_id] = b
        return b

    def _resolve(self, option):
        opt = option or AddOption()
        return ((self._backup(opt.worker_id),),
                (float(opt.learning_rate), float(opt.lambda_)))

    @staticmethod
    def torch_step(w, bak, g, scalars) -> None:
        lr, lam = scalars
        w.sub_(lr * (g + lam * g * g * (w - bak)))
        bak.copy_(w)


class DCASGDAUpdater(DCASGDUpdater):
    """DC-ASGD-a ("dcasgda", updater.cpp:52): adaptive lambda — a running
    mean-square of the gradient m = rho*m + (1-rho)*g*g scales the
    compensation coefficient to lambda / sqrt(m + eps)."""

    name = "dcasgda"
    EPS = 1e-7

    def __init__(self, shard: torch.Tensor) -> None:
        super().__init__(shard)
        self.mean_sqr = torch.zeros_like(shard)

    def _resolve(self, option):
        opt = option or AddOption()
        return ((self._backup(opt.worker_id), self.mean_sqr),
                (float(opt.learning_rate), float(opt.lambda_),
                 float(opt.rho), self.EPS))

    @staticmethod
    def torch_step(w, bak, msq, g, scalars) -> None:
        lr, lam, rho, eps = scalars
        msq.mul_(rho).add_((1.0 - rho) * g * g)
        lam_t = lam / torch.sqrt(msq + eps)
        w.sub_(lr * (g + lam_t * g * g * (w - bak)))
        bak.copy_(w)


class AdamUpdater(Updater):
    """Adam / AdamW ("adam"), the first updater beyond the reference's set:

        w  = w * (1 - lr*wd)              # decoupled decay; wd = 0: plain Adam
        m  = b1*m + (1-b1)*g
        v  = b2*v + (1-b2)*g*g
        w -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

    i.e. ``torch.optim.Adam`` / ``AdamW`` with ``amsgrad=False``, and
    ``SparseAdam`` for keyed batches. ``g`` is the delta as it reaches the
    shard, unscaled (in the collective plane: the sum over workers).
    ``step`` is ONE host-side count per shard of the updates applied so far,
    whole-table and keyed alike; ``t`` is its value after the update, and
    the bias corrections and the decay factor are computed from it on the
    host in double and handed to the kernel as scalars. There is no per-row
    count: a row that a keyed Add names rarely is corrected with the shard's
    ``t``, as in ``SparseAdam``.

    The 20-byte envelope carries the hyperparameters as ``learning_rate``
    -> lr, ``momentum`` -> b1, ``rho`` -> b2, ``lambda_`` -> wd (see
    ``AddOption.adam``); ``option=None`` means ``AddOption.adam()``, not the
    ``AddOption()`` field defaults. float32 and float64 shards only."""

    name = "adam"
    EPS = 1e-8

    def __init__(self, shard: torch.Tensor) -> None:
        if shard.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"updater_type 'adam' needs a float32 or float64 "
                            f"table, got {shard.dtype} (integer tables are "
                            f"add-only: use 'default')")
        super().__init__(shard)
        self.exp_avg = torch.zeros_like(shard)
        self.exp_avg_sq = torch.zeros_like(shard)
        self.step = 0

    def next_scalars(self, option: Optional[AddOption]):
        """Count one update and return the kernel's scalars for it, all in
        double: (b1, b2, lr/(1-b1^t), 1/sqrt(1-b2^t), 1-lr*wd, eps)."""
        opt = option if option is not None else AddOption.adam()
        lr, b1 = float(opt.learning_rate), float(opt.momentum)
        b2, wd = float(opt.rho), float(opt.lambda_)
        self.step += 1
        t = self.step
        return (b1, b2, lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** -0.5,
                1.0 - lr * wd, self.EPS)

    @staticmethod
    def torch_step(w: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                   g: torch.Tensor, scalars) -> None:
        """The same formula in torch ops, in place on w, m and v (CPU, and
        the keyed path of tables the row kernel does not cover)."""
        b1, b2, step, rbc2, decay, eps = scalars
        w.mul_(decay)
        m.mul_(b1).add_(g, alpha=1.0 - b1)
        v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
        w.addcdiv_(m, v.sqrt().mul_(rbc2).add_(eps), value=-step)

    def _resolve(self, option):
        return (self.exp_avg, self.exp_avg_sq), self.next_scalars(option)


_REGISTRY: Dict[str, Type[Updater]] = {
    "default": DefaultUpdater,
    "sgd": SGDUpdater,
    "momentum": MomentumUpdater,
    "adagrad": AdaGradUpdater,
    "dcasgd": DCASGDUpdater,
    "dcasgda": DCASGDAUpdater,
    "adam": AdamUpdater,
}


def create_updater(name: str, shard: torch.Tensor) -> Updater:
    """Factory keyed by the ``updater_type`` flag (updater.cpp:46-57)."""
    try:
        cls = _REGISTRY[name]
    except KeyError:
        raise ValueError(f"unknown updater_type '{name}' "
                         f"(have {sorted(_REGISTRY)})") from None
    return cls(shard)
