"""The rules of bn_index_append_rows / bn_index_append_subset (include/birdnet_hip.h, "Copying rows between indexes") restated in numpy.

An index is a State: the stored rows as bn_index_read returns them ([size, dim] float32, compared as bytes), one valid flag per row, the
tag plane (uint32 [size]) or None where the index never tagged, the size and the capacity.  append() gives the state of dst after a call
and the id of the first new row, or raises Refused with the word the library's message carries; append_loop() is the same contract one
row at a time, for the reference's own check."""
from dataclasses import dataclass
from typing import Optional

import numpy as np


class Refused(Exception):
    """BN_ERR_INVALID_ARG: nothing appended, both states as before"""


@dataclass
class State:
    rows: np.ndarray            # [size, dim] float32: the stored bits
    valid: np.ndarray           # [size] bool: False for a row stored as zeros
    tags: Optional[np.ndarray]  # [size] uint32, or None: no tag plane
    size: int
    capacity: int

    @property
    def dim(self) -> int:
        return self.rows.shape[1]

    def read_tags(self) -> np.ndarray:
        """what bn_index_read_tags returns: an absent plane reads as zeros"""
        return np.zeros(self.size, dtype=np.uint32) if self.tags is None else self.tags.astype(np.uint32)

    def check(self):
        assert self.rows.dtype == np.float32 and self.rows.shape[0] == self.size == len(self.valid) <= self.capacity
        assert self.tags is None or len(self.tags) == self.size
        return self


def state(rows, tags=None, capacity=None) -> State:
    """the state of an index that holds the STORED rows `rows`; valid: any element nonzero (the index's rule on stored bits)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    valid = (rows.view(np.uint32) & 0x7FFFFFFF != 0).any(axis=1) if rows.shape[1] else np.zeros(len(rows), dtype=bool)
    t = None if tags is None else np.asarray(tags, dtype=np.uint32).copy()
    return State(rows.copy(), valid, t, len(rows), len(rows) if capacity is None else capacity).check()


def empty(dim: int, capacity: int, tagged: bool = False) -> State:
    return State(np.zeros((0, dim), dtype=np.float32), np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint32) if tagged else None, 0, capacity)


def source_ids(src: State, first_id: int = 0, n_ids: int = 0, ids=None) -> np.ndarray:
    """the old id of every new row, in order: the range [first_id, first_id + n_ids) (n_ids 0: to the end), or a subset's list"""
    if ids is not None:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        assert (np.diff(ids) > 0).all() and (len(ids) == 0 or (ids[0] >= 0 and ids[-1] < src.size)), "not a subset of the source"
        return ids
    if first_id > src.size or n_ids > src.size - first_id:
        raise Refused("range")
    return np.arange(first_id, first_id + n_ids if n_ids else src.size, dtype=np.int64)


def _refusals(dst: State, src: State, same: bool, borrowed: bool):
    if same:
        raise Refused("borrows" if borrowed else "same index")
    if dst.dim != src.dim:
        raise Refused("dim")


def append(dst: State, src: State, first_id: int = 0, n_ids: int = 0, ids=None, same: bool = False):
    """(state of dst after the call, first_new_id).  same: dst and src are one index"""
    _refusals(dst, src, same, ids is not None)
    old = source_ids(src, first_id, n_ids, ids)
    n = len(old)
    if n > dst.capacity - dst.size:
        raise Refused("capacity")
    if n == 0:
        return dst, dst.size
    if src.tags is not None:
        tags = np.concatenate([dst.read_tags(), src.tags[old]])
    elif dst.tags is not None:
        tags = np.concatenate([dst.tags, np.zeros(n, dtype=np.uint32)])
    else:
        tags = None
    out = State(np.concatenate([dst.rows, src.rows[old]]), np.concatenate([dst.valid, src.valid[old]]), tags, dst.size + n, dst.capacity)
    return out.check(), dst.size


def append_loop(dst: State, src: State, first_id: int = 0, n_ids: int = 0, ids=None, same: bool = False):
    """the header's sentences one row at a time"""
    if same:
        raise Refused("borrows" if ids is not None else "same index")
    if dst.rows.shape[1] != src.rows.shape[1]:
        raise Refused("dim")
    if ids is None:
        if not (0 <= first_id <= src.size and n_ids <= src.size - first_id):
            raise Refused("range")
        end = first_id + n_ids if n_ids else src.size
        old = list(range(first_id, end))
    else:
        old = [int(i) for i in ids]
    if dst.size + len(old) > dst.capacity:
        raise Refused("capacity")
    rows = [dst.rows[i].tobytes() for i in range(dst.size)]
    valid = [bool(v) for v in dst.valid]
    has_plane = dst.tags is not None or (src.tags is not None and len(old) > 0)
    tags = [int(t) for t in dst.tags] if dst.tags is not None else [0] * dst.size
    first_new = dst.size
    for j, i in enumerate(old):                               # new row first_new + j is old row i
        assert len(rows) == first_new + j
        rows.append(src.rows[i].tobytes())
        valid.append(bool(src.valid[i]))
        tags.append(int(src.tags[i]) if src.tags is not None else 0)
    return rows, valid, (tags if has_plane else None), len(rows), first_new


def same_state(a: State, loop) -> bool:
    rows, valid, tags, size, _ = loop
    return (a.size == size and [a.rows[i].tobytes() for i in range(a.size)] == rows and a.valid.tolist() == valid and
            ((a.tags is None) == (tags is None)) and (tags is None or a.tags.tolist() == tags))
