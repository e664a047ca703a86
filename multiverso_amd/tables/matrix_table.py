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

- ``nearest_rows`` = top-k row search where the shard lives: each owner scans
  its rows once (k_row_topk + k_topk_merge) and only ``k`` (score, id) pairs
  per query per shard cross the wire; ``merge_topk`` holds the one ordering
  rule. float32 tables, ``k <= 64``, dot or cosine.

Sparse/stale-aware Get (SparseMatrixTable's per-(worker,row) freshness
bitmap) is implemented in sparse_matrix.py on top of this class; it takes no
``wire_dtype``.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..comm import (Handle, ShardSpec, all_to_all_rows, all_to_all_values,
                    exchange_sizes)
from ..dashboard import monitor
from ..log import CHECK
from ..updaters import AddOption
from .dense import DenseTable

# nearest_rows: the largest k (one list slot per lane of a 64-lane wave) and
# the id of an empty slot, above every real row
MAX_NEAREST = 64
EMPTY_ID = torch.iinfo(torch.int64).max


def merge_topk(scores: torch.Tensor, ids: torch.Tensor, k: int
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The first ``k`` of ``[Q, m]`` candidates per query under the ordering
    rule of nearest_rows, defined here and in kernels.hip (topk_before) and
    nowhere else: a comes before b when ``a.score > b.score``, or the scores
    are equal and ``a.id < b.id``. A NaN score counts as ``-inf``. An empty
    slot is ``(-inf, EMPTY_ID)``; it sorts behind every real candidate, so it
    is dropped whenever ``k`` real ones exist, and fills the tail (``m < k``
    included) when they do not."""
    scores = torch.where(scores.isnan(),
                         torch.full_like(scores, float("-inf")), scores)
    if scores.shape[1] < k:
        pad = (scores.shape[0], k - scores.shape[1])
        scores = torch.cat([scores, scores.new_full(pad, float("-inf"))], 1)
        ids = torch.cat([ids, ids.new_full(pad, EMPTY_ID)], 1)
    ids, by_id = torch.sort(ids, dim=1, stable=True)
    scores = scores.gather(1, by_id)
    scores, by_score = torch.sort(scores, dim=1, descending=True, stable=True)
    return (scores[:, :k].contiguous(),
            ids.gather(1, by_score)[:, :k].contiguous())


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

    # ---- nearest rows: top-k row search where the shard lives ----
    def nearest_rows(self, queries, k: int, metric: str = "cosine"
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ``k`` rows of the table closest to each query: returns
        ``(scores, ids)``, float32 ``[Q, k]`` and int64 ``[Q, k]`` (global row
        ids), on the table's device, best first in merge_topk's order.

        ``queries`` is ``[Q, num_col]`` or ``[num_col]`` (one query, the
        result is ``[1, k]``), any device and float dtype; ``Q == 0`` returns
        two ``[0, k]`` tensors. ``1 <= k <= min(64, num_row)``: 64 is one
        list slot per lane of a wave, the same limit on CPU and GPU.
        ``metric="dot"`` scores row r as ``sum_e r[e]*q[e]``; ``"cosine"``
        normalises the queries here (``q / ||q||``, a zero query stays zero)
        and scores ``dot(r, q_hat) / ||r||``, a zero-norm row exactly 0.0.
        What the owner computes is what comes back; nothing is rescaled
        after selection. Float32 tables only. Queries and results travel as
        fp32 and int64 whatever the table's wire format.

        Every owner scans its own rows once and keeps its k best per query;
        only ``k`` pairs per query per shard cross the wire. On the sync
        plane this is a collective like ``get_rows``: every rank calls it,
        with its own queries and its own ``Q`` (0 included), and the same
        ``k`` and ``metric`` (not checked). Updater state and the sparse
        table's freshness bitmap are not touched."""
        self.flush()   # a deferred whole-table Add must land first
        CHECK(self.dtype == torch.float32,
              f"nearest_rows needs a float32 table, not {self.dtype}")
        CHECK(metric in ("dot", "cosine"),
              f"nearest_rows metric {metric!r} is not known "
              f"('dot' or 'cosine')")
        CHECK(isinstance(k, int) and 1 <= k <= min(MAX_NEAREST, self.num_row),
              f"nearest_rows k={k} must be in 1..min({MAX_NEAREST}, num_row="
              f"{self.num_row})")
        q = torch.as_tensor(queries)
        CHECK(q.is_floating_point(), "nearest_rows queries must be float")
        q = q.to(self.device, torch.float32)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        CHECK(q.dim() == 2 and q.shape[1] == self.num_col,
              f"nearest_rows queries must be [Q, {self.num_col}], got "
              f"{tuple(q.shape)}")
        # contiguous first: the norm of a strided view may round differently
        q = q.contiguous()
        if metric == "cosine":
            n = torch.linalg.vector_norm(q, dim=1, keepdim=True)
            q = torch.where(n > 0, q / n, q)
        eng = self.engine
        with monitor("worker.nearest_rows"):
            if eng is not None:
                CHECK(self.zoo.is_worker,
                      "ps_role=server ranks issue no searches")
                s, i = eng.nearest(self, q, k, metric)
            elif self.zoo.size > 1:
                s, i = self._nearest_exchange(q, k, metric)
            else:
                # one owner holds every row (k <= num_row: no empty slot)
                # and its selection already is the ordering rule's
                return self._server_nearest(q, k, metric)
            return merge_topk(s, i, k)

    def _nearest_exchange(self, q: torch.Tensor, k: int, metric: str):
        """Sync plane: my queries to every server, ``k`` candidates per query
        back from each; returns them as ``[Q, n*k]``. The counts ride the
        control lane."""
        n, nq = self.zoo.size, q.shape[0]
        theirs = exchange_sizes([nq] * n)
        mine = [nq] * n
        in_q = all_to_all_values(q.reshape(-1).repeat(n), mine, theirs,
                                 self.num_col)
        s, i = self._server_nearest(in_q.view(-1, self.num_col), k, metric)
        s = all_to_all_values(s.reshape(-1), theirs, mine, k)
        i = all_to_all_values(i.reshape(-1), theirs, mine, k)
        return (s.view(n, nq, k).transpose(0, 1).reshape(nq, n * k),
                i.view(n, nq, k).transpose(0, 1).reshape(nq, n * k))

    def _server_nearest(self, queries: torch.Tensor, k: int, metric: str
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The owned shard's ``k`` best rows for each query (fp32 ``[Q,
        num_col]`` on the table's device, already normalised under cosine):
        ``(scores [Q,k], global ids [Q,k])``, padded with empty slots where
        the shard has fewer than ``k`` rows. k_row_topk + k_topk_merge on GPU;
        torch ops on CPU and where the launcher refuses (one query larger
        than its LDS budget)."""
        with self._shard_lock, monitor("server.nearest_rows"):
            if self.shard.is_cuda:
                from .. import ops
                got = ops.module(required=True).row_topk(
                    self.shard, queries, k, metric == "cosine",
                    self.row_offset)
                if got is not None:
                    return got
            s = queries @ self.shard.t()
            if metric == "cosine":
                norm = torch.linalg.vector_norm(self.shard, dim=1)
                s = torch.where(norm == 0, torch.zeros_like(s), s / norm)
            ids = torch.arange(self.row_offset,
                               self.row_offset + self.local_rows,
                               device=s.device).expand(s.shape[0], -1)
            return merge_topk(s, ids, k)

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
