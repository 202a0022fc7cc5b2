"""Golden fixtures on disk.  A fixture is one compressed ``<name>.npz``; one whose archive would pass the 1 MiB limit
for a committed file is stored as ``<name>.part0.npz``, ``<name>.part1.npz``, ... instead, every array whole and
unchanged in exactly one part.  ``load_npz`` returns the same ``{key: array}`` either way."""
import glob
import os

import numpy as np

MAX_BYTES = 1000 * 1024  # per file, below the 1 MiB limit


def _parts(path):
    return sorted(glob.glob(path[:-len(".npz")] + ".part[0-9].npz"))


def load_npz(path):
    files = [path] if os.path.exists(path) else _parts(path)
    if not files:
        raise FileNotFoundError(path)
    rec = {}
    for fn in files:
        with np.load(fn) as z:
            for k in z.files:
                assert k not in rec, (fn, k)
                rec[k] = z[k]
    return rec


def save_npz(path, rec, max_bytes=MAX_BYTES):
    """Write ``rec`` as ``path`` if that fits in ``max_bytes``, else as the fewest parts that each do (keys in
    order, split by array size)."""
    for old in [path] + _parts(path):
        if os.path.exists(old):
            os.remove(old)
    np.savez_compressed(path, **rec)
    if os.path.getsize(path) <= max_bytes:
        return [path]
    os.remove(path)
    keys, total = list(rec), sum(np.asarray(v).nbytes for v in rec.values())
    for n in range(2, 10):
        groups, acc = [[] for _ in range(n)], 0
        for k in keys:
            groups[min(n - 1, acc * n // max(1, total))].append(k)
            acc += np.asarray(rec[k]).nbytes
        files = []
        for i, g in enumerate(groups):
            files.append(f"{path[:-len('.npz')]}.part{i}.npz")
            np.savez_compressed(files[-1], **{k: rec[k] for k in g})
        if all(os.path.getsize(f) <= max_bytes for f in files):
            return files
        for f in files:
            os.remove(f)
    raise ValueError(f"{path}: does not fit in 9 parts of {max_bytes} bytes")
