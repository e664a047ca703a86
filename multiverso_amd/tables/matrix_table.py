"""MatrixTable — 2-D dense table, row-sharded, whole-table or row-keyed ops.

Capability parity with the reference MatrixTable / unified Matrix table
(src/table/matrix_table.cpp, src/table/matrix.cpp): row sharding with
``num_row/num_servers`` rows per server and the remainder on the last
(matrix_table.cpp:24-45), whole-table Get/Add (:66-75, :387-417), row-set
Get/Add by ids (:59-147), optional uniform random init (float, :372-384),
raw-bytes Store/Load (:457-464).

MI355X mapping:
- whole-table Get = all-gather; whole-table Add = reduce-scatter + one
  fused updater kernel (K1-K4) on the owned rows. That path, with the
  single-rank Add deferral, is DenseTable's (dense.py), shared with
  ArrayTable.
- row-keyed ops = all-to-all exchange of (ids, values); the owner runs the
  K5/K6 gather/scatter kernels on its HBM shard. This replaces the
  per-server Request_Get/Add message fan-out (matrix_table.cpp:235-314)
  with per-destination bucketed traffic matched to xGMI's 7 p2p links.
- row-keyed Add runs the table's own updater on the touched rows only
  (matrix_table.cpp:403-412; the rule is the updater's, see
  updaters.Updater.update_rows): default/sgd scatter-add, adagrad the keyed
  K15 kernel, momentum/dcasgd/dcasgda/adam the k_row_update kernel —
  duplicate ids of one batch are summed in batch order, then one updater
  step per distinct row; weights and updater state of other rows stay as
  they are.

- ``wire_dtype=torch.bfloat16`` (float32 tables): every payload above is
  bf16 — whole-table deltas and Get results, keyed values in both directions
  of the all-to-all — while the shard and updater state stay fp32. The
  kernels widen and narrow in registers; duplicate rows of a keyed Add are
  summed in fp32 after widening.

- ``add_filter="onebit"`` (float32 tables): every whole-table Add goes
  through onebit_filter — signs plus two scales per 1024 elements, the
  quantisation error kept in ``self.residual`` (fp32, the full table size,
  per worker) and added to the next delta. Row-keyed ops, Get, Store and
  Load are unfiltered and leave the residual alone.

Sparse/stale-aware Get (SparseMatrixTable's per-(worker,row) freshness
bitmap) is implemented in sparse_matrix.py on top of this class; it takes no
``wire_dtype``.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..comm import Handle, ShardSpec, all_to_all_rows, all_to_all_values
from ..dashboard import monitor
from ..log import CHECK
from ..updaters import AddOption
from .dense import DenseTable


class MatrixTable(DenseTable):
    def __init__(self, num_row: int, num_col: int,
                 dtype: torch.dtype = torch.float32,
                 updater_type: Optional[str] = None,
                 random_init: Optional[Tuple[float, float]] = None,
                 wire_dtype: Optional[torch.dtype] = None,
                 add_filter: Optional[str] = None) -> None:
        super().__init__(updater_type)
        self._set_wire(wire_dtype, dtype)
        self._set_add_filter(add_filter, dtype, wire_dtype)
        CHECK(num_row >= self.zoo.num_servers,
              f"num_row {num_row} must be >= num_servers")
        self.num_row = num_row
        self.num_col = num_col
        self.dtype = dtype
        self.spec = ShardSpec(num_row, self.zoo.num_servers)
        if self.zoo.is_server:
            self.row_offset, self.local_rows = self.spec.range_of(
                self.zoo.server_id)
        else:
            self.row_offset, self.local_rows = 0, 0  # ps_role=worker
        self.shard = torch.zeros(self.local_rows, num_col, dtype=dtype,
                                 device=self.device)
        if random_init is not None:
            # reference matrix_table.cpp:372-384: uniform [min, max), float,
            # identical content on every rank's view of its own rows.
            lo, hi = random_init
            g = torch.Generator(device="cpu").manual_seed(0x5EED + self.table_id)
            full = torch.rand(num_row, num_col, generator=g) * (hi - lo) + lo
            self.shard.copy_(full[self.row_offset:
                                  self.row_offset + self.local_rows])
        self._make_updater(self.shard.view(-1))
        self._init_dense(num_row * num_col, num_col, (num_row, num_col))

    # ---- row-keyed ops (matrix_table.cpp:59-147, K5/K6) ----
    def _local_rows_of(self, ids: torch.Tensor) -> torch.Tensor:
        return ids - self.row_offset

    def _gather_local(self, local_ids: torch.Tensor) -> torch.Tensor:
        """K6 on the owned shard (HIP kernel for the f32 hot path;
        other dtypes use torch indexing — parity, not headline)."""
        if self.shard.is_cuda and self.dtype == torch.float32:
            from .. import ops
            hip = ops.module(required=True)
            if self.wire != self.dtype:   # bf16 wire: narrow while gathering
                return hip.row_gather(self.shard, local_ids, self.wire)
            return hip.row_gather(self.shard, local_ids)
        return self.shard[local_ids].to(self.wire)

    def get_rows(self, row_ids) -> torch.Tensor:
        """Row-subset Get: returns [len(row_ids), num_col] in caller order.

        ``row_ids`` is planned on the host (CPU ids are sync-free; device
        ids cost one D2H) and the split sizes ride the gloo control lane —
        no device sync between launch and the value all-to-all."""
        self.flush()
        eng = self.engine
        if eng is not None:
            CHECK(self.zoo.is_worker, "ps_role=server ranks issue no Gets")
            ids = torch.as_tensor(row_ids, dtype=torch.int64).cpu()
            with monitor("worker.get_rows"):
                return eng.keyed_get(self, ids, self.num_col)
        ids = torch.as_tensor(row_ids, dtype=torch.int64)
        with monitor("worker.get_rows"):
            in_ids, _, recv_sizes, order, send_sizes = all_to_all_rows(
                ids, None, self.spec, self.num_col, device=self.device)
            # serve: gather requested rows from my shard
            local = self._local_rows_of(in_ids)
            served = self._gather_local(local)
            # reply: route rows back to the requesters (what I received I
            # serve back — sizes swap roles, nothing recomputed)
            if self.zoo.size > 1:
                flat = all_to_all_values(served.view(-1), recv_sizes,
                                         send_sizes, self.num_col)
                got = flat.view(-1, self.num_col)
            else:
                # single rank: ids were never owner-sorted (order is the
                # identity), so the gather IS caller order — the
                # permutation write below would be a pure 31 us/chunk
                # identity index_put (measured, profiles r2 smaxprof2)
                return served.view(-1, self.num_col)
            # got is in owner-grouped order == order of sorted ids; undo sort
            out = torch.empty(ids.numel(), self.num_col, dtype=self.wire,
                              device=self.device)
            out[order] = got
        return out

    def add_rows(self, row_ids, values: torch.Tensor,
                 option: Optional[AddOption] = None,
                 assume_unique: bool = False) -> None:
        """Row-subset Add (matrix_table.cpp:265-309 partition path).
        ``assume_unique=True`` asserts the caller's row_ids have no
        duplicates (e.g. a sorted-unique union) — at world size 1 the
        scatter then skips atomics; with multiple ranks incoming ids can
        still collide across ranks, so atomics stay."""
        self.flush()   # a deferred whole-table Add must land first
        ids = torch.as_tensor(row_ids, dtype=torch.int64)
        vals = values.to(self.device, self.wire).contiguous()
        CHECK(vals.numel() == ids.numel() * self.num_col,
              "add_rows values size mismatch")
        eng = self.engine
        if eng is not None:
            CHECK(self.zoo.is_worker, "ps_role=server ranks issue no Adds")
            with monitor("worker.add_rows"):
                self._track(Handle(eng.keyed_add(
                    self, ids.cpu(), vals, self.num_col, option)))
            return
        with monitor("worker.add_rows"):
            in_ids, in_vals, _, _, _ = all_to_all_rows(
                ids, vals.view(-1), self.spec, self.num_col,
                device=self.device)
            if in_ids.numel():
                local = self._local_rows_of(in_ids)
                with monitor("server.update_rows"):
                    self.updater.update_rows(
                        local, in_vals.view(-1, self.num_col), option,
                        assume_unique=assume_unique and self.zoo.size == 1)
                self._rows_added(local)

    def _rows_added(self, local_ids: torch.Tensor) -> None:
        """Sync-plane hook: a keyed Add just updated these local rows."""

    # ---- server-side keyed entry points (async engine + local path) ----
    def _server_add_rows(self, local_ids: torch.Tensor,
                         vals2d: torch.Tensor, option) -> None:
        with self._shard_lock:
            with monitor("server.update_rows"):
                self.updater.update_rows(
                    local_ids, vals2d.reshape(-1, self.num_col), option)

    def _server_get_rows(self, local_ids: torch.Tensor) -> torch.Tensor:
        with self._shard_lock:
            return self._gather_local(local_ids)

    # ---- checkpoint (matrix_table.cpp:457-464) ----
    def store(self, path: str) -> None:
        """Raw whole-table bytes (row-major), streamed: each rank pwrites
        its own row range at its byte offset — no rank-0 staging."""
        self.flush()
        self._store_shard_stream(path, self.shard.view(-1),
                                 self.row_offset * self.num_col,
                                 self.num_row * self.num_col)

    def load(self, path: str) -> None:
        self.flush()
        self._load_shard_stream(path, self.shard.view(-1),
                                self.row_offset * self.num_col,
                                self.num_row * self.num_col)
