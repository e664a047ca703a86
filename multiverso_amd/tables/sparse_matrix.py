"""SparseMatrixTable — MatrixTable with stale-aware (freshness-filtered)
whole-table Get.

Capability parity with the reference SparseMatrixTable
(src/table/sparse_matrix_table.cpp) / unified Matrix with is_sparse
(src/table/matrix.cpp): the server keeps a per-(worker, row) up-to-date
bitmap; a worker's Get returns only the rows that are stale FOR THAT
WORKER (UpdateGetState, :226-258), and an Add invalidates the touched rows
for every OTHER worker (UpdateAddState, :200-223). Workers therefore keep
a local cache of the whole table and only stale rows travel.

MI355X mapping: the bitmap lives with the owning shard as a bool tensor in
HBM; ``get_into(cache)`` is a collective where each owner builds each
requester's stale row list (a masked select), serves those rows (K6
gather) and marks them fresh; the rows travel in one all-to-all. Keyed
adds travel through the base class and invalidate per source rank."""

from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from ..comm import all_to_all_values
from ..dashboard import monitor
from ..log import CHECK
from ..updaters import AddOption
from .matrix_table import MatrixTable


class SparseMatrixTable(MatrixTable):
    _defer_ready = True   # bitmap must exist before async requests serve

    def __init__(self, num_row: int, num_col: int,
                 dtype: torch.dtype = torch.float32,
                 updater_type: Optional[str] = None,
                 random_init=None) -> None:
        super().__init__(num_row, num_col, dtype, updater_type, random_init)
        # SparseFilter on the stale-row reply payloads (the reference
        # filters every outgoing sparse-table bundle,
        # sparse_matrix_table.cpp:148-153): per-destination segments are
        # compressed when >50% zero; byte accounting on the Dashboard.
        from ..configure import get_flag
        # the filter's wire format is float32; non-f32 tables go dense
        # (silent precision loss otherwise — ADVICE r1)
        self.use_sparse_filter = (bool(get_flag("sparse_filter"))
                                  and dtype == torch.float32)
        nw = self.zoo.num_workers
        # up_to_date[w, r] == True -> worker w has the current row r
        self.up_to_date = torch.zeros(nw, self.local_rows, dtype=torch.bool,
                                      device=self.device)
        self._ready.set()

    # ---- invalidation hooks ----
    def _invalidate_all_but(self, local_ids: torch.Tensor,
                            worker: Optional[int]) -> None:
        self.up_to_date[:, local_ids] = False
        if worker is not None:
            self.up_to_date[worker, local_ids] = True

    def add(self, delta, option=None, async_op: bool = False):
        h = super().add(delta, option, async_op=async_op)
        # whole-table add touches every row; a dense add comes from every
        # worker at once (reduce-scatter), so everyone is stale.
        self.up_to_date.zero_()
        return h

    # ---- async-mode server hooks (the reference's sparse table served
    # its bitmap under the async server identically, matrix.cpp:461-478) --
    def _server_apply_chunk(self, chunk, option) -> None:
        super()._server_apply_chunk(chunk, option)
        with self._shard_lock:
            self.up_to_date.zero_()   # whole-shard add: everyone stale

    def _server_stale_for(self, worker: int):
        """Rows of MY shard stale for ``worker``: gather them, mark them
        fresh, return (global_ids, values). UpdateGetState semantics
        (sparse_matrix_table.cpp:226-258) served on arrival."""
        with self._shard_lock:
            stale = (~self.up_to_date[worker]).nonzero().reshape(-1)
            if stale.numel():
                served = self._gather_local(stale)
                self.up_to_date[worker, stale] = True
            else:
                served = torch.empty(0, self.num_col, dtype=self.dtype,
                                     device=self.device)
            return stale + self.row_offset, served

    def _server_add_rows(self, local_ids, vals2d, option) -> None:
        super()._server_add_rows(local_ids, vals2d, option)
        with self._shard_lock:
            self.up_to_date[:, local_ids.to(self.up_to_date.device)] = False

    def add_rows(self, row_ids, values, option: Optional[AddOption] = None,
                 source_worker: Optional[int] = None) -> None:
        # on the async plane the server-side hook above invalidates the
        # touched rows; on the sync plane _rows_added does
        super().add_rows(row_ids, values, option)

    def _rows_added(self, local_ids: torch.Tensor) -> None:
        # UpdateAddState: conservatively invalidate the touched rows for
        # EVERY worker (the reference spares the adding worker, whose cache
        # is pre-add anyway; invalidating all is never-stale-safe and costs
        # one extra row re-pull)
        self.up_to_date[:, local_ids] = False

    def _filtered_value_exchange(self, served: torch.Tensor,
                                 send_rows, recv_rows) -> torch.Tensor:
        """Value half of the stale-row exchange with SparseFilter applied
        per destination segment (FilterIn on send, FilterOut on receive —
        quantization_util.h:95-154 semantics over the collective). The
        per-segment payload sizes AND compressed flags travel in ONE
        control-lane message, so the receiver never reads per-segment
        device headers (no .item() syncs — ADVICE r1)."""
        from .. import sparse_filter as sf
        from ..comm import exchange_size_rows
        device = self.device
        packed_parts, packed_sizes, flags = [], [], []
        off = 0
        for n in send_rows:
            seg = served[off:off + n].reshape(-1)
            off += n
            payload, compressed = sf.filter_in(seg)
            packed_parts.append(payload)
            packed_sizes.append(payload.numel())
            flags.append(1 if compressed else 0)
        send_buf = (torch.cat(packed_parts) if packed_parts else
                    torch.empty(0, dtype=torch.float32, device=device))
        rsizes, rflags = exchange_size_rows([packed_sizes, flags])
        recv_buf = torch.empty(sum(rsizes), dtype=torch.float32,
                               device=device)
        dist.all_to_all_single(recv_buf, send_buf, rsizes, packed_sizes)
        outs, off = [], 0
        for n, sz, fl in zip(recv_rows, rsizes, rflags):
            payload = recv_buf[off:off + sz]
            off += sz
            outs.append(sf.filter_out(payload, bool(fl),
                                      n * self.num_col))
        return (torch.cat(outs) if outs else
                torch.empty(0, dtype=self.dtype, device=device))

    # ---- pipelined (double-buffered) stale get ----
    def prefetch_into(self, cache: torch.Tensor) -> "Handle":
        """The unified Matrix's ``is_pipeline`` capability
        (matrix.cpp:384-420: doubled up_to_date bitmap so the next
        block's Get proceeds while the current block computes): issue
        the stale-row exchange NOW, overlap with compute, apply to
        ``cache`` on ``wait()``. Rows are marked fresh at issue time —
        adds landing between issue and wait re-invalidate them, so the
        next get re-pulls (the doubled-bitmap semantics). Collective:
        every rank must call. The value exchange is dense (the
        SparseFilter's per-segment packing is synchronous by nature);
        ``handle.rows`` carries the incoming row count after wait()."""
        from ..comm import Handle, exchange_sizes
        CHECK(cache.shape == (self.num_row, self.num_col),
              "cache must be the full table shape")
        self.flush()
        if self.engine is not None:
            n = self.get_into(cache)   # async lane: served on arrival
            h = Handle()
            h.rows = n
            return h
        if self.zoo.size == 1:
            n = self.get_into(cache)
            h = Handle()
            h.rows = n
            return h
        nw = self.zoo.num_workers
        with monitor("worker.sparse_prefetch"):
            stale_lists = [(~self.up_to_date[w]).nonzero().reshape(-1)
                           for w in range(nw)]
            send_rows = [int(s.numel()) for s in stale_lists]
            recv_rows = exchange_sizes(send_rows)
            all_ids = (torch.cat(stale_lists) + self.row_offset
                       if sum(send_rows) else
                       torch.empty(0, dtype=torch.int64, device=self.device))
            got_ids = torch.empty(sum(recv_rows), dtype=torch.int64,
                                  device=self.device)
            w1 = dist.all_to_all_single(got_ids, all_ids, recv_rows,
                                        send_rows, async_op=True)
            served = (self._gather_local(torch.cat(stale_lists))
                      if sum(send_rows) else
                      torch.empty(0, self.num_col, dtype=self.dtype,
                                  device=self.device))
            got_vals = torch.empty(sum(recv_rows) * self.num_col,
                                   dtype=self.dtype, device=self.device)
            w2 = dist.all_to_all_single(
                got_vals, served.reshape(-1),
                [r * self.num_col for r in recv_rows],
                [s * self.num_col for s in send_rows], async_op=True)
            for w in range(nw):
                if send_rows[w]:
                    self.up_to_date[w, stale_lists[w]] = True

        def finish() -> None:
            w1.wait()
            w2.wait()
            if got_ids.numel():
                cache[got_ids] = got_vals.view(-1, self.num_col)
        h = Handle(None, finish)
        h.rows = sum(recv_rows)
        return self._track(h)

    # ---- stale-filtered whole-table get ----
    def get_into(self, cache: torch.Tensor) -> int:
        """Overwrite only the rows of ``cache`` that are stale for this
        worker; marks them fresh. Returns the number of rows received.
        Collective: every rank must call."""
        CHECK(cache.shape == (self.num_row, self.num_col),
              "cache must be the full table shape")
        self.flush()
        eng = self.engine
        if eng is not None:
            CHECK(self.zoo.is_worker, "ps_role=server ranks issue no Gets")
            with monitor("worker.sparse_get"):
                return eng.sparse_get_stale(self, cache)
        me = self.zoo.worker_id
        nw = self.zoo.num_workers
        with monitor("worker.sparse_get"):
            if self.zoo.size == 1:
                stale = (~self.up_to_date[0]).nonzero().reshape(-1)
                if stale.numel():
                    cache[stale] = self._gather_local(stale)
                    self.up_to_date[0, stale] = True
                return int(stale.numel())
            # 1) each owner builds per-requester stale lists
            stale_lists = [(~self.up_to_date[w]).nonzero().reshape(-1)
                           for w in range(nw)]
            send_rows = [int(s.numel()) for s in stale_lists]
            # 2) counts ride the control lane; then ids+values
            from ..comm import exchange_sizes
            recv_rows = exchange_sizes(send_rows)
            all_ids = torch.cat(stale_lists) + self.row_offset
            got_ids = torch.empty(sum(recv_rows), dtype=torch.int64,
                                  device=self.device)
            dist.all_to_all_single(got_ids, all_ids, recv_rows, send_rows)
            served = (self._gather_local(torch.cat(stale_lists))
                      if all_ids.numel() else
                      torch.empty(0, self.num_col, dtype=self.dtype,
                                  device=self.device))
            if self.use_sparse_filter:
                got_vals = self._filtered_value_exchange(
                    served, send_rows, recv_rows)
            else:
                got_vals = all_to_all_values(served.view(-1), send_rows,
                                             recv_rows, self.num_col)
            # 3) write into cache; mark fresh on the server side
            if got_ids.numel():
                cache[got_ids] = got_vals.view(-1, self.num_col)
            for w in range(nw):
                if send_rows[w]:
                    self.up_to_date[w, stale_lists[w]] = True
            return int(got_ids.numel())
