"""Golden fixtures under tests/golden/: ``load(name)`` reads <name>.npz, or -- for a fixture stored in parts so that no committed file
exceeds 1 MiB -- every <name>.part<K>.npz, K = 0, 1, ...  A key "<array>@<i>" of a part is row block i of <array> (blocks are joined
along axis 0 in i order); every other key is an array as is.  ``save_parts(name, arrays)`` writes that form."""
import glob
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
PART_LIMIT = 900 << 10          # compressed bytes per part file (below 1 MiB with the zip overhead)


def exists(name, root=GOLDEN):
    return os.path.exists(os.path.join(root, name + ".npz")) or os.path.exists(os.path.join(root, name + ".part0.npz"))


def load(name, root=GOLDEN):
    whole = os.path.join(root, name + ".npz")
    if os.path.exists(whole):
        return np.load(whole)
    parts = sorted(glob.glob(os.path.join(root, glob.escape(name) + ".part*.npz")), key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))
    if not parts:
        raise FileNotFoundError(whole)
    out, blocks = {}, {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                if "@" in k:
                    a, i = k.rsplit("@", 1)
                    blocks.setdefault(a, {})[int(i)] = z[k]
                else:
                    out[k] = z[k]
    for a, bl in blocks.items():
        out[a] = np.concatenate([bl[i] for i in range(len(bl))], axis=0)
    return out


def _packed_size(arrays):
    import io
    b = io.BytesIO()
    np.savez_compressed(b, **arrays)
    return b.tell()


def save_parts(name, arrays, root=GOLDEN):
    """Greedy packing in key order: an array too large for one part is cut into row blocks that each fit."""
    pieces = []
    for k, v in arrays.items():
        v = np.asarray(v)
        if _packed_size({k: v}) <= PART_LIMIT:
            pieces.append((k, v))
            continue
        n = 2
        while _packed_size({"x": np.array_split(v, n, axis=0)[0]}) > PART_LIMIT:
            n += 1
        pieces += [(f"{k}@{i}", b) for i, b in enumerate(np.array_split(v, n, axis=0))]
    parts, cur = [], {}
    for k, v in pieces:
        if cur and _packed_size({**cur, k: v}) > PART_LIMIT:
            parts.append(cur)
            cur = {}
        cur[k] = v
    parts.append(cur)
    for i, p in enumerate(parts):
        np.savez_compressed(os.path.join(root, f"{name}.part{i}.npz"), **p)
    return len(parts)
