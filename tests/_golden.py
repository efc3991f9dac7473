"""Golden fixtures larger than a committed file may be (1 MiB) are stored in parts: NAME.part0.npz, NAME.part1.npz, ...
each holding a run of the arrays, an array too large for one part split along its first axis into ``KEY#i`` pieces.
``load`` gives the same mapping ``np.load("NAME.npz")`` gave for the whole file (``.files``, ``[key]``); the fixture
generators under tools/ write through ``save``."""
import glob
import os
import re

import numpy as np

PART_BYTES = 768 << 10          # raw bytes per part: compressed, a part stays below 1 MiB even for incompressible data


class Golden:
    def __init__(self, arrays):
        self._arrays = arrays
        self.files = list(arrays)

    def __getitem__(self, key):
        return self._arrays[key]

    def __contains__(self, key):
        return key in self._arrays


def save(directory, name, arrays, part_bytes=PART_BYTES):
    """Write ``arrays`` (a dict) as NAME.npz when it fits in one part, else as NAME.part<i>.npz."""
    for stale in glob.glob(os.path.join(directory, f"{name}.part*.npz")) + glob.glob(os.path.join(directory, f"{name}.npz")):
        os.remove(stale)
    if sum(np.asarray(v).nbytes for v in arrays.values()) <= part_bytes:
        np.savez_compressed(os.path.join(directory, f"{name}.npz"), **arrays)
        return
    pieces = []                                           # (key, array) in order, large arrays cut along axis 0
    for key, v in arrays.items():
        v = np.asarray(v)
        if v.nbytes <= part_bytes or v.ndim == 0:
            pieces.append((key, v))
            continue
        rows = max(1, part_bytes // max(1, v.nbytes // v.shape[0]))
        for i, start in enumerate(range(0, v.shape[0], rows)):
            pieces.append((f"{key}#{i}", v[start:start + rows]))
    parts, cur, size = [], {}, 0
    for key, v in pieces:
        if cur and size + v.nbytes > part_bytes:
            parts.append(cur)
            cur, size = {}, 0
        cur[key] = v
        size += v.nbytes
    parts.append(cur)
    for i, part in enumerate(parts):
        np.savez_compressed(os.path.join(directory, f"{name}.part{i}.npz"), **part)


def load(directory, name):
    """-> the arrays of NAME.npz, or of its parts put back together, as a ``Golden`` mapping."""
    whole = os.path.join(directory, f"{name}.npz")
    if os.path.exists(whole):
        with np.load(whole) as z:
            return Golden({k: z[k] for k in z.files})
    paths = sorted(glob.glob(os.path.join(directory, f"{name}.part*.npz")),
                   key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))
    if not paths:
        raise FileNotFoundError(whole)
    pieces = {}
    for p in paths:
        with np.load(p) as z:
            for k in z.files:
                pieces[k] = z[k]
    arrays = {}
    for key, v in pieces.items():
        base, _, idx = key.rpartition("#")
        if base and idx.isdigit():
            arrays.setdefault(base, []).append((int(idx), v))
        else:
            arrays[key] = v
    return Golden({k: np.concatenate([x for _, x in sorted(v, key=lambda t: t[0])]) if isinstance(v, list) else v
                   for k, v in arrays.items()})
