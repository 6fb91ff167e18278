"""Snapshot -- environments copied out of a BatchedAuvEnv (auv_snapshot), to be put back (auv_restore) into the same handle or
into any handle with the same layout and the same world bank.

A row is opaque packed device memory (include/auv_hip.h documents it); this module holds the container and the host-side checks of
`BatchedAuvEnv.restore(validate=True)`, which need no device."""
from typing import Optional

import numpy as np
import torch


class Snapshot:
    """`rows` [m, row_bytes] uint8: one packed row per environment; `layout`: the fingerprint of the handle's row layout
    (auv_snapshot_layout); `envs` [m] int32: the environments the rows were taken from.  `cpu()` / `to(device)` move the tensors,
    so a snapshot can be kept on the host, saved with torch.save(snap.state_dict()) and loaded again."""

    def __init__(self, rows: torch.Tensor, layout: int, envs: torch.Tensor):
        if rows.dim() != 2 or rows.dtype != torch.uint8:
            raise ValueError("rows must be a [m, row_bytes] uint8 tensor")
        if envs.dim() != 1 or envs.numel() != rows.shape[0]:
            raise ValueError("envs must have one entry per row (%d), got %s" % (rows.shape[0], tuple(envs.shape)))
        self.rows = rows.contiguous()
        self.layout = int(layout)
        self.envs = envs.to(torch.int32).contiguous()

    @property
    def n_rows(self) -> int:
        return int(self.rows.shape[0])

    @property
    def row_bytes(self) -> int:
        return int(self.rows.shape[1])

    @property
    def device(self) -> torch.device:
        return self.rows.device

    def to(self, device) -> "Snapshot":
        return Snapshot(self.rows.to(device), self.layout, self.envs.to(device))

    def cpu(self) -> "Snapshot":
        return self.to("cpu")

    def state_dict(self):
        return dict(rows=self.rows.cpu(), layout=self.layout, envs=self.envs.cpu())

    @classmethod
    def from_state_dict(cls, sd) -> "Snapshot":
        return cls(sd["rows"], sd["layout"], sd["envs"])

    def __repr__(self):
        return "Snapshot(%d rows x %d bytes, layout %016x, %s)" % (self.n_rows, self.row_bytes, self.layout, self.device)


def _host_indices(x, name: str) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError("%s must be one-dimensional, got shape %s" % (name, a.shape))
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must hold integers, got %s" % (name, a.dtype))
    return a.astype(np.int64)


def check_restore(snap_layout: int, own_layout: int, n_rows: int, n_envs: int, rows, envs) -> None:
    """What restore(validate=True) refuses (ValueError): a snapshot of another layout, a row index outside [0, n_rows), an
    environment outside [0, n_envs), index arrays of different lengths, an environment written twice.  `rows` / `envs`: index
    arrays (any integer array-like; device tensors are read back -- this is the path that may synchronise)."""
    if int(snap_layout) != int(own_layout):
        raise ValueError("the snapshot's layout %016x is not this environment batch's (%016x): it was taken from a batch of another "
                         "shape (sensors, obstacles / movers per world, pooling, channels, worlds)" % (int(snap_layout), int(own_layout)))
    r, e = _host_indices(rows, "rows"), _host_indices(envs, "envs")
    if r.size != e.size:
        raise ValueError("rows and envs must have the same length, got %d and %d" % (r.size, e.size))
    if r.size and (r.min() < 0 or r.max() >= n_rows):
        raise ValueError("row index out of range [0, %d)" % n_rows)
    if e.size and (e.min() < 0 or e.max() >= n_envs):
        raise ValueError("environment index out of range [0, %d)" % n_envs)
    if np.unique(e).size != e.size:
        raise ValueError("an environment is written twice (one row may feed many environments, not the other way round)")


def resolve_pairs(snap_envs, n_rows: int, rows: Optional[object], envs: Optional[object]):
    """The (rows, envs) index pair of a restore with defaults filled in: rows=None is 0 .. m - 1 (m = len(envs), or every row);
    envs=None puts every row back where it was taken from (snap.envs[rows])."""
    if rows is None and envs is None:
        return torch.arange(n_rows, dtype=torch.int32, device=snap_envs.device), snap_envs
    if rows is None:
        envs = torch.as_tensor(envs)
        return torch.arange(envs.numel(), dtype=torch.int32, device=envs.device), envs
    rows = torch.as_tensor(rows)
    if envs is None:
        return rows, snap_envs.to(rows.device)[rows.long()]
    return rows, torch.as_tensor(envs)
