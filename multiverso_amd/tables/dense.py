"""DenseTable — the whole-table Get/Add path of ArrayTable and MatrixTable.

Written once in terms of three things the subclass hands ``_init_dense``:
the flat element count, the ``cols`` stride the collectives take (1 for an
array, ``num_col`` for a matrix: shards split on row boundaries) and the
public shape of a Get buffer.

MI355X mapping: Get = all-gather of shards into the caller's buffer; Add =
reduce-scatter of the delta followed by one fused updater kernel on the
owned shard. Both can be issued async and overlap with compute.

Single-rank Add deferral: an Add immediately followed by a whole-table Get
fuses into one updater kernel (updater.update_and_copy) that writes both the
shard and the Get buffer, saving the Get's shard re-read (0.5 GB/step on the
headline config). Any other table op materializes the Add first (flush).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..comm import (Handle, allgather_shards, onebit_exchange_delta,
                    reduce_scatter_delta)
from ..dashboard import monitor
from ..log import CHECK
from ..updaters import AddOption
from .base import Table


class DenseTable(Table):
    def _init_dense(self, numel: int, cols: int,
                    get_shape: Tuple[int, ...]) -> None:
        """Last step of a subclass constructor (shard and updater exist)."""
        self._numel = numel
        self._cols = cols
        self._get_shape = get_shape
        self._deferred = None  # (delta, option, delta._version)
        # subclasses with extra server state (SparseMatrixTable's
        # bitmap) publish readiness themselves after that state exists
        if not getattr(type(self), "_defer_ready", False):
            self._ready.set()

    def _apply_deferred(self, out: Optional[torch.Tensor] = None) -> None:
        """Apply the pending Add, if any; with ``out`` through the fused
        update+copy kernel."""
        d = self._deferred
        if d is None:
            return
        self._deferred = None
        self._check_deferred(d)
        with monitor("server.update"):
            if out is None:
                self.updater.update(d[0], d[1])
            else:
                self.updater.update_and_copy(d[0], d[1], out.view(-1))

    def _check_deferred(self, d) -> None:
        CHECK(d[0]._version == d[2],
              "the delta tensor passed to Add was mutated in place before "
              "the Add was applied (single-GPU deferred-Add fast path "
              "snapshots at the next table op; pass a fresh tensor)")

    def flush(self) -> None:
        self._apply_deferred()
        super().flush()

    def _get_buffer(self, out: Optional[torch.Tensor]) -> torch.Tensor:
        """``out`` size-checked, or a fresh buffer of the wire dtype."""
        if out is None:
            return torch.empty(self._get_shape, dtype=self.wire,
                               device=self.device)
        CHECK(out.numel() == self._numel, "Get buffer size mismatch")
        return out

    def _engine_get(self, eng, out, async_op):
        """Async-mode whole-table Get: request each server's shard; served
        on arrival (worker.cpp:30-51 -> server.cpp:36-46)."""
        CHECK(self.zoo.is_worker, "ps_role=server ranks issue no Gets")
        self.flush()
        user_out = out
        out = self._get_buffer(out)
        if not out.is_contiguous() or self._stage_get(out):
            out = self._get_buffer(None)
        with monitor("worker.get"):
            pr = eng.whole_get(self, out.view(-1), self._cols)

        def _finish() -> None:
            if user_out is not None and user_out is not out:
                user_out.copy_(out.view_as(user_out))
        h = Handle(pr, _finish)
        ret = user_out if user_out is not None else out
        if async_op:
            self._track(h)
            return ret, h
        h.wait()
        return ret

    def get(self, out: Optional[torch.Tensor] = None, async_op: bool = False):
        """Whole-table Get (array_table.cpp:24-66, matrix_table.cpp:66-75)."""
        eng = self.engine
        if eng is not None:
            return self._engine_get(eng, out, async_op)
        user_out = out
        out = self._get_buffer(out)
        # fused update+copy kernel needs a GPU contiguous target of the
        # wire dtype (fp32, or bf16 on a bf16-wire table; the deferral
        # itself only happens on GPU shards); any other out materializes
        # the Add and falls through to the copy path
        if (self._deferred is not None and not async_op
                and out.is_contiguous() and out.is_cuda
                and out.dtype == self.wire):
            self._apply_deferred(out)
            return out
        self.flush()
        if not out.is_contiguous() or self._stage_get(out):
            # gather needs a flat view (and, on a bf16-wire table, a bf16
            # one); stage and copy into the user's buffer afterwards
            out = self._get_buffer(None)
        with monitor("worker.get"):
            h = allgather_shards(out.view(-1), self.shard.view(-1), self.spec,
                                 self._cols, async_op=async_op)
        if out is not user_out and user_out is not None:
            if async_op:
                h.wait()
            user_out.copy_(out.view_as(user_out))
            out = user_out
        if async_op:
            self._track(h)
            return out, h
        return out

    def add(self, delta: torch.Tensor, option: Optional[AddOption] = None,
            async_op: bool = False) -> Handle:
        """Whole-table Add: reduce-scatter + updater (server.cpp:48 ->
        array_table.cpp:116-127); in async mode, per-server slices applied
        on arrival. Single-rank GPU adds DEFER until the next table op
        (fusing with an immediately following Get); every public read
        applies the pending add first, and in-place mutation of ``delta``
        before then is a loud error. Use ``flush()`` to force
        materialization (e.g. before timing the update itself)."""
        CHECK(delta.numel() == self._numel, "Add delta size mismatch")
        delta = delta.to(self.device, self.wire).contiguous().view(-1)
        eng = self.engine
        if eng is not None:
            CHECK(self.zoo.is_worker, "ps_role=server ranks issue no Adds")
            self.flush()
            with monitor("worker.add"):
                h = Handle(eng.whole_add(self, delta, self._cols, option,
                                         want_ack=not async_op))
            if async_op:
                return self._track(h)
            h.wait()
            return h
        if self.add_filter and self.zoo.size == 1:
            # the decoded tensor is the table's own: the caller may mutate
            # its delta at once
            delta = self._filter_local(delta)
        if self.zoo.size == 1 and self.shard.is_cuda:
            self.flush()                 # at most one deferred Add
            self._deferred = (delta, option, delta._version)
            return Handle()
        with monitor("worker.add"):
            if self.add_filter and self.zoo.size > 1:
                chunk, h = onebit_exchange_delta(
                    delta, self._filter_residual(delta.numel()), self.spec,
                    self._cols, async_op=async_op)
            else:
                chunk, h = reduce_scatter_delta(delta, self.spec, self._cols,
                                                async_op=async_op)
            if async_op:
                upd, opt = self.updater, option

                def epilogue() -> None:
                    with monitor("server.update"):
                        upd.update(chunk, opt)

                # inner Handle resolves the collective; epilogue applies the
                # updater exactly once (Handle latches on _done).
                return self._track(Handle(h, epilogue))
            with monitor("server.update"):
                self.updater.update(chunk, option)
            return Handle()
