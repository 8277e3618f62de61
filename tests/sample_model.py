"""The contract of labsort_sample_device (include/labsort.h) as a numpy model with Python integers,
shared by test_sample_model.py and test_gpu_sample.py.  An element weighs top_p_model.weight; a row's
total is W; a random word U in [0, 2^32) gives the target s = floor(U W / 2^32), and the draw is the
smallest position whose inclusive prefix of weights exceeds s; a row with W == 0 draws SENTINEL and
flags the status.  Arrays are words (uint16 for "bf16" / "f16", uint32 for "f32").  Nothing here calls
the library."""
import numpy as np

import top_p_model as P

SENTINEL = 0xFFFFFFFF


def draw(x, U, kind):
    """(positions, flagged): uint32 positions of shape U.shape for the words x (rows x cols) and the
    random words U (rows x ndraw), and whether the status call reports ERR_ARG."""
    return draw_weights(P.weight(np.asarray(x), kind), U)


def draw_weights(w, U):
    """draw() on the uint64 weights w (rows x cols) themselves."""
    w, U = np.asarray(w), np.asarray(U)
    rows, ndraw = U.shape
    assert w.shape[0] == rows
    out = np.full((rows, ndraw), SENTINEL, dtype=np.uint32)
    flagged = False
    for r in range(rows):
        cum = np.cumsum(w[r], dtype=np.uint64)  # (< 2^63 for cols <= 2^23)
        W = int(cum[-1])
        if W == 0:
            flagged = True
            continue
        s = np.array([(int(u) * W) >> 32 for u in U[r]], dtype=np.uint64)
        out[r] = np.searchsorted(cum, s, side="right")
    return out, flagged


def boundaries(x_row, kind):
    """For every cumulative mass c of the row with 0 < c < W, ascending: the word U_b = ceil(c 2^32 / W),
    the first U that leaves the element ending at c.  Returns (U_b as Python integers, c likewise)."""
    cum = np.cumsum(P.weight(np.asarray(x_row), kind), dtype=np.uint64)
    W = int(cum[-1])
    cs = [int(c) for c in np.unique(cum) if 0 < int(c) < W]
    return [-((-c << 32) // W) for c in cs], cs
