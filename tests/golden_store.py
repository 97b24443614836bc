"""Golden vectors bigger than a committed file may be (1 MiB) are stored in parts: tests/golden/<name>.partNN.npz. An array of up to
CHUNK_BYTES is stored under its own key; a larger one is flattened and cut into chunks <key>@0, <key>@1, ... beside <key>@shape.
load() gives back the arrays bit for bit, whether the vectors are stored in one <name>.npz or in parts."""
import glob
import os

import numpy as np

CHUNK_BYTES = 448 << 10   # raw bytes of one stored piece
PART_BYTES = 896 << 10    # raw bytes of one part file (compression only makes it smaller; the zip overhead is a few hundred bytes)


def save(stem, **arrays):
    """write `arrays` as stem.partNN.npz (compressed), no part above PART_BYTES of raw array data"""
    pieces = []
    for k, v in arrays.items():
        v = np.asarray(v)
        if v.nbytes <= CHUNK_BYTES:
            pieces.append((k, v))
            continue
        pieces.append((k + "@shape", np.asarray(v.shape, dtype=np.int64)))
        flat = v.reshape(-1)
        step = max(1, CHUNK_BYTES // v.itemsize)
        pieces += [("%s@%d" % (k, i), flat[o:o + step]) for i, o in enumerate(range(0, flat.size, step))]
    for old in glob.glob(stem + ".part*.npz"):
        os.remove(old)
    parts, cur, size = [], {}, 0
    for k, v in pieces:
        if cur and size + v.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    parts.append(cur)
    for i, p in enumerate(parts):
        np.savez_compressed("%s.part%02d.npz" % (stem, i), **p)


def load(stem):
    """{key: array} of stem.npz, or of the parts stem.partNN.npz written by save()"""
    if os.path.exists(stem + ".npz"):
        with np.load(stem + ".npz", allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    files = sorted(glob.glob(stem + ".part*.npz"))
    if not files:
        raise FileNotFoundError(stem + ".npz")
    raw = {}
    for f in files:
        with np.load(f, allow_pickle=False) as z:
            raw.update({k: z[k] for k in z.files})
    out = {}   # (in the order the arrays were saved)
    for k, v in raw.items():
        if "@" not in k:
            out[k] = v
        elif k.endswith("@shape"):
            k = k[:-len("@shape")]
            n = sum(1 for c in raw if c.startswith(k + "@") and c != k + "@shape")
            out[k] = np.concatenate([raw["%s@%d" % (k, i)] for i in range(n)]).reshape(tuple(v))
    return out
