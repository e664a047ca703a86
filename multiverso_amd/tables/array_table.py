"""ArrayTable — 1-D dense table, contiguous-sharded across ranks.

Capability parity with the reference ArrayTable
(src/table/array_table.cpp, include/multiverso/table/array_table.h):
whole-table Get/Add only (the reference always sends key −1), contiguous
partition ``size/num_servers`` with the remainder on the last server
(array_table.cpp:11-21), server-side updater on Add (:116-127), Access
copy-out on Get (:130-141), raw-bytes Store/Load (:144-151).

The whole-table path itself (Get, Add, the single-rank Add deferral) is
DenseTable's (dense.py), shared with MatrixTable; this class is the 1-D
sharding, Store and Load.

``wire_dtype=torch.bfloat16`` (float32 tables) halves the bytes of both: the
delta is rounded to bf16 once and travels so, the owner's updater kernel
widens it in registers, and Get returns the fp32 shard rounded to bf16. The
shard, updater state and Store/Load stay fp32.

``add_filter="onebit"`` (float32 tables) sends every whole-table Add through
onebit_filter: signs plus two scales per 1024 elements, the quantisation
error kept in ``self.residual`` (fp32, the full table size, per worker) and
added to the next delta. Get, Store and Load are unfiltered.
"""

from __future__ import annotations

from typing import Optional

import torch

from ..comm import ShardSpec
from ..log import CHECK
from .dense import DenseTable


class ArrayTable(DenseTable):
    def __init__(self, size: int, dtype: torch.dtype = torch.float32,
                 updater_type: Optional[str] = None,
                 wire_dtype: Optional[torch.dtype] = None,
                 add_filter: Optional[str] = None) -> None:
        super().__init__(updater_type)
        self._set_wire(wire_dtype, dtype)
        self._set_add_filter(add_filter, dtype, wire_dtype)
        CHECK(size >= self.zoo.num_servers,
              f"table size {size} must be >= num_servers "
              f"{self.zoo.num_servers} (reference array_table.cpp:14)")
        self.size = size
        self.dtype = dtype
        self.spec = ShardSpec(size, self.zoo.num_servers)
        if self.zoo.is_server:
            off, cnt = self.spec.range_of(self.zoo.server_id)
        else:
            cnt = 0   # ps_role=worker: no shard hosted here
        self.shard = torch.zeros(cnt, dtype=dtype, device=self.device)
        self.row_offset = 0   # keyed-op base (arrays have no keyed ops)
        self._make_updater(self.shard)
        self._init_dense(size, 1, (size,))

    # ---- checkpoint (Store/Load, array_table.cpp:144-151) ----
    def store(self, path: str) -> None:
        """Write whole-table raw bytes, byte-identical to the reference's
        concatenated per-shard Store layout. Streaming: each rank pwrites
        its own shard at its offset — no rank-0 full-table gather."""
        self.flush()
        off, _ = self.spec.range_of(self.zoo.server_id)
        self._store_shard_stream(path, self.shard, off, self.size)

    def load(self, path: str) -> None:
        """Each rank reads only its own shard slice (streamed)."""
        self.flush()
        off, _ = self.spec.range_of(self.zoo.server_id)
        self._load_shard_stream(path, self.shard, off, self.size)
