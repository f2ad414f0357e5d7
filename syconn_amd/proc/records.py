"""Device-side record arrays of the dataset mergers (``proc.sd_proc.ChunkMerger``, ``extraction.cs_extraction_steps
.ContactSiteMerger``) and the download of the segment offsets their merges return."""
import numpy as np

# one record per (chunk, id) of an object table: id, representative coordinate, bounding box, voxels
OBJECT_FIELDS = [('ids', 'int64', 1), ('rc', 'int32', 3), ('bb', 'int32', 6), ('sizes', 'int64', 1)]


class Records:
    """Growable device arrays appended to at a device-side cursor.  ``fields`` = [(name, torch dtype name, inner width)]; `cursor`: a
    1-element view into the merger's counter tensor."""

    def __init__(self, device, fields, capacity: int, cursor):
        import torch
        self.device, self.cursor = device, cursor
        self.fields = [(n, getattr(torch, dt), w) for n, dt, w in fields]
        self.capacity = int(capacity)
        self.arrays = {n: self._new(dt, w, self.capacity) for n, dt, w in self.fields}

    def _new(self, dtype, width, n):
        from .. import _dev as D
        return D.empty((n, width) if width > 1 else n, dtype, self.device)

    def ptrs(self):
        return [self.arrays[n] for n, _, _ in self.fields]

    def room_for(self, stored: int, n_more: int):
        """`stored` records are known to be in the arrays; make sure `n_more` further ones fit."""
        need = int(stored) + int(n_more)
        if need <= self.capacity:
            return
        cap = max(need, 2 * self.capacity)
        for n, dt, w in self.fields:
            grown = self._new(dt, w, cap)
            keep = min(int(stored) + int(n_more), self.capacity)      # (everything that may have been written so far)
            grown[:keep] = self.arrays[n][:keep]
            self.arrays[n] = grown
        self.capacity = cap


def segment_offsets(begin, n_segments: int, end: int) -> np.ndarray:
    """int64 offsets (n_segments + 1) of the segments of a merge: the uint32 starts the device wrote into the int32 tensor `begin`,
    closed by `end`."""
    return np.concatenate((begin[:n_segments].cpu().numpy().view(np.uint32).astype(np.int64), [end]))
