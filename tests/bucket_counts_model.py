"""The contracts of labsort_bucket_counts_device and labsort_bincount_device (include/labsort.h) as
numpy models.  A bucket count is np.bincount over the ranks of tests/searchsorted_model.py, so the two
entries cannot drift apart: counts[r][b] = the number of values of row r that searchsorted ranks b.
Arrays are uint16, uint32 or uint64 words; kind is one of searchsorted_model.KINDS.  Nothing here
calls the library."""
import numpy as np

import searchsorted_model as SM

BIN_KINDS = ("u32", "i32", "u64", "i64")
SIGNED = {"u32": np.uint32, "i32": np.int32, "u64": np.uint64, "i64": np.int64}


def counts_of_ranks(ranks, nedges):
    """np.bincount(minlength=nedges + 1) per row of a 1-D or 2-D array of ranks, uint32."""
    ranks = np.asarray(ranks)
    if ranks.ndim == 1:
        return np.bincount(ranks.astype(np.int64), minlength=nedges + 1).astype(np.uint32)
    return np.stack([np.bincount(r.astype(np.int64), minlength=nedges + 1) for r in ranks]).astype(np.uint32) if ranks.shape[0] \
        else np.zeros((0, nedges + 1), dtype=np.uint32)


def expected(edges, values, right, kind):
    """The counts, uint32 of shape (nedges + 1,) for 1-D values, (rows, nedges + 1) for 2-D values.
    edges: 1-D (every row is counted on it) or rows x nedges."""
    edges, values = np.asarray(edges, dtype=SM.word_dtype(kind)), np.asarray(values, dtype=SM.word_dtype(kind))
    nedges = edges.shape[-1]
    return counts_of_ranks(SM.expected(edges, values, right, kind), nedges)


def loop_counts(edges, values, right, kind):
    """The definition, one comparison at a time (for the model's own test; 1-D, small): a value's bin is
    the number of edges below it (right: not above it)."""
    u, v = [int(t) for t in SM.image(edges, kind)], [int(t) for t in SM.image(values, kind)]
    out = np.zeros(len(u) + 1, dtype=np.uint32)
    for t in v:
        out[sum(1 for e in u if (e <= t if right else e < t))] += 1
    return out


def bincount_expected(values, nbins, kind):
    """counts[r][b] = the values of row r equal to b, b < nbins; counts[r][nbins] = those outside
    [0, nbins).  values: 1-D or 2-D words of a kind of BIN_KINDS."""
    assert kind in BIN_KINDS
    x = np.asarray(values, dtype=SM.word_dtype(kind)).view(SIGNED[kind])
    rows = x.reshape(1, -1) if x.ndim == 1 else x
    out = np.zeros((rows.shape[0], nbins + 1), dtype=np.uint32)
    for r, row in enumerate(rows):
        inside = (row >= 0) & (row < nbins) if nbins else np.zeros(row.shape, dtype=bool)
        out[r, :nbins] = np.bincount(row[inside].astype(np.int64), minlength=nbins)[:nbins]
        out[r, nbins] = row.size - int(inside.sum())
    return out[0] if x.ndim == 1 else out


def bincount_loop(values, nbins, kind):
    x = [int(t) for t in np.asarray(values, dtype=SM.word_dtype(kind)).view(SIGNED[kind])]
    out = np.zeros(nbins + 1, dtype=np.uint32)
    for t in x:
        out[t if 0 <= t < nbins else nbins] += 1
    return out


def bincount_words(n, nbins, seed, kind):
    """n words around [0, nbins): most inside, some at the ends, some negative or far outside."""
    rng = np.random.default_rng([seed, n, nbins])
    dt = SIGNED[kind]
    x = rng.integers(0, max(nbins, 1), size=n, dtype=np.int64)
    far = np.array([-1, -2, nbins, nbins + 1, 0, nbins - 1, np.iinfo(np.int32).max, np.iinfo(np.int32).min,
                    (1 << 40) + 3, -(1 << 40), 1 << 32], dtype=np.int64)
    at = rng.random(n) < 0.2
    x[at] = far[rng.integers(0, far.size, size=int(at.sum()))]
    if kind in ("u32", "i32"):
        x = x.astype(np.int32)  # (wraps: 2^32 becomes 0, 2^40 + 3 becomes 3)
    return x.astype(dt).view(SM.word_dtype(kind))
