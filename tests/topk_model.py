"""The radix select of labsort_topk_device (csrc/topk.hip) as a host model, shared by
test_topk_model.py and test_gpu_topk_select.py: the expected outputs in O(cols) per row, the level at
which the device must narrow a row, the select's shape constants read from csrc/topk.h, and
deterministic generators of rows that narrow at a chosen level or whose bucket has a chosen size.
Arrays are uint32 or uint16 words; kind is "u32", "i32", "f32", "bf16" or "f16".  The generators work
on the order image u (plain unsigned order is the order asked for, the direction included); raw_of
maps an image back to the words of a kind.  Nothing here calls the library."""
import glob
import os
import re

import numpy as np

import f16_model as M16
import f32_model as M32

KINDS32 = ("u32", "i32", "f32")
KINDS16 = M16.KINDS
KINDS = KINDS32 + KINDS16
NEVER = None  # narrow_level's answer for a row that is read from the input at every level


def bits_of(kind):
    return 16 if kind in KINDS16 else 32


def levels_of(kind):
    """Digit levels of a call: 8 bits each."""
    return bits_of(kind) // 8


def word_dtype(kind):
    return np.uint16 if kind in KINDS16 else np.uint32


# ---- the select's constants, from the header the kernels are compiled with ----

def _topk_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    found = [h for h in glob.glob(os.path.join(repo, "*", "csrc", "topk.h"))
             if os.path.exists(os.path.join(os.path.dirname(os.path.dirname(h)), "__init__.py"))]
    assert len(found) == 1, f"csrc/topk.h next to the package's __init__.py: {found}"
    return found[0]


def constants():
    """TK_CHUNK, TK_BLOCK, TK_CAND_DIV and TK_MAX_HIST_WG of csrc/topk.h.  Each must be found: a
    renamed constant fails here and does not move a test off its edge."""
    with open(_topk_header()) as f:
        text = f.read()
    out = {}
    for name in ("TK_CHUNK", "TK_BLOCK", "TK_CAND_DIV", "TK_MAX_HIST_WG"):
        m = re.findall(r"constexpr\s+(?:int|uint32_t|unsigned)\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert len(m) == 1, f"{name}: {len(m)} definitions found in csrc/topk.h"
        out[name] = int(m[0])
    return out


def cap_of(cols, consts):
    """Pairs a row's candidate buffer holds."""
    return cols // consts["TK_CAND_DIV"]


# ---- order images ----

def _dir_mask(kind, largest):
    return word_dtype(kind)((1 << bits_of(kind)) - 1 if largest else 0)


def u_of(x, kind, largest=False):
    """The order image of the words x under the direction."""
    if kind == "f32":
        return M32.u_of(x, largest)
    if kind in KINDS16:
        return M16.u_of(x, kind, largest)
    return np.asarray(x, dtype=np.uint32) ^ np.uint32(0x80000000 if kind == "i32" else 0) ^ _dir_mask(kind, largest)


def raw_of(u, kind, largest=False):
    """The words whose image is u.  (Float kinds: u must avoid the images no word has, which the
    generators below do; the tests assert u_of(raw_of(u)) == u.)"""
    o = np.asarray(u, dtype=word_dtype(kind)) ^ _dir_mask(kind, largest)
    if kind == "f32":
        return M32.unord_bits(o)
    if kind in KINDS16:
        return M16.unord16(o)
    return o ^ np.uint32(0x80000000 if kind == "i32" else 0)


# ---- expected outputs ----

def select_expected(u, k):
    """u: (rows, cols) order images.  Per row the positions of the first k elements of the stable
    sort of u: only the elements up to the k-th smallest value are sorted."""
    u = np.asarray(u)
    assert u.ndim == 2 and u.dtype in (np.uint32, np.uint16) and 1 <= k <= u.shape[1]
    out = np.empty((u.shape[0], k), dtype=np.int64)
    for r, row in enumerate(u):
        t = np.partition(row, k - 1)[k - 1]
        at = np.flatnonzero(row <= t)
        out[r] = at[np.argsort(row[at], kind="stable")[:k]]
    return out


def expected(x, k, kind, largest):
    """x: (rows, cols) words of the kind.  The keys and positions labsort_topk_device must write."""
    idx = select_expected(u_of(x, kind, largest), k)
    return np.take_along_axis(x, idx, axis=1), idx.astype(np.uint32)


def assert_keys(got, want, kind, msg=""):
    """Float kinds: NaN-ness equal everywhere, everything else bit-exact.  Integers: bit-exact."""
    if kind == "f32":
        M32.assert_keys(got, want, msg)
    elif kind in KINDS16:
        M16.assert_keys(got, want, kind, msg)
    else:
        np.testing.assert_array_equal(got, want, err_msg=f"keys: {msg}")


# ---- where the device narrows ----

def narrow_level(u_row, k, cap, levels):
    """The level after which the device copies this row's bucket to the candidate buffer: the first
    level, the last one excluded, at which the keys sharing the k-th key's digits so far number at
    most cap.  NEVER when there is none."""
    u_row = np.asarray(u_row)
    assert u_row.ndim == 1 and levels == u_row.dtype.itemsize and 1 <= k <= u_row.size
    bits = 8 * levels
    kth = np.partition(u_row, k - 1)[k - 1]
    for level in range(levels - 1):
        shift = u_row.dtype.type(bits - 8 * (level + 1))
        if int(np.count_nonzero((u_row >> shift) == (kth >> shift))) <= cap:
            return level
    return NEVER


def select_runs(cols, k, sort_div):
    """The precondition of the select on a long row: k at most cols / sort_div."""
    return cols // k >= sort_div


# ---- generators (order images) ----
# Top bytes stay within 0x04 .. 0xFB: every image in that range is the image of one word for
# every kind and direction (the images of NaNs other than all-ones lie outside it).
TOP_LO, TOP_HI = 0x04, 0xFC


def _rand_bits(rng, n, width):
    if width == 0:
        return np.zeros(n, dtype=np.uint64)
    return rng.integers(0, 1 << width, size=n, dtype=np.uint64)


def _prefix(rng, share):
    """share (a multiple of 8) random top bits, the top byte within the range above."""
    if share == 0:
        return 0
    return (int(rng.integers(TOP_LO, TOP_HI)) << (share - 8)) | int(rng.integers(0, 1 << (share - 8)))


def row_narrowing_at(level, cols, seed, bits=32):
    """Random keys sharing their top 8 * level bits, so that the device narrows after `level`; for
    NEVER, keys sharing all but their low byte."""
    nlev = bits // 8
    assert level is NEVER or 0 <= level < nlev - 1
    rng = np.random.default_rng([seed, 0x70D0, bits, nlev if level is NEVER else level])
    share = bits - 8 if level is NEVER else 8 * level
    low = bits - share
    if share == 0:
        u = (rng.integers(TOP_LO, TOP_HI, size=cols, dtype=np.uint64) << np.uint64(bits - 8)) | _rand_bits(rng, cols, bits - 8)
    else:
        u = np.uint64(_prefix(rng, share) << low) | _rand_bits(rng, cols, low)
    return u.astype(np.uint32 if bits == 32 else np.uint16)


def row_bucket_of(size, level, cols, k_below, seed, bits=32):
    """A row whose keys share their top 8 * level bits; at `level`, k_below keys have a digit below
    the bucket's, exactly `size` keys lie in the bucket and the rest above it, in random places.  The
    bucket's keys take their remaining bits from 32 values, so every k in k_below + 1 ..
    k_below + size falls on a value with many ties."""
    nlev = bits // 8
    assert 0 <= level < nlev - 1 and 0 < size and 0 <= k_below and size + k_below <= cols
    rng = np.random.default_rng([seed, 0x70D1, bits, level, size, k_below])
    share, w = 8 * level, bits - 8 * (level + 1)
    D = 0x80
    lo, hi = (TOP_LO, TOP_HI) if level == 0 else (0, 256)
    n_above = cols - size - k_below
    digit = np.concatenate([rng.integers(lo, D, size=k_below, dtype=np.uint64),
                            np.full(size, D, dtype=np.uint64),
                            rng.integers(D + 1, hi, size=n_above, dtype=np.uint64)])
    pool = _rand_bits(rng, 32, w)
    rem = np.concatenate([_rand_bits(rng, k_below, w), pool[rng.integers(0, 32, size=size)], _rand_bits(rng, n_above, w)])
    u = np.uint64(_prefix(rng, share) << (bits - share)) | (digit << np.uint64(w)) | rem
    return u[rng.permutation(cols)].astype(np.uint32 if bits == 32 else np.uint16)


def k_below_of(k):
    """The keys the bucket rows put below their bucket for a call with this k: two thirds of it, so
    the k-th key lies inside the bucket and cuts a run of ties."""
    return (2 * k) // 3


# ---- the seeded sweep's cases ----
ROW_GENS = ("level0", "level1", "level2", "never", "cap@0", "cap+1@0", "cap@1", "cap+1@1", "ties", "random")


def sweep_row(gen, cols, k, kind, largest, cap, seed):
    """One row of words of the kind from the named generator."""
    bits = bits_of(kind)
    if gen in ("ties", "random"):  # float words with NaNs, both zeros and the planted specials
        if bits == 16:
            return (M16.tie_words if gen == "ties" else M16.random_words)((cols,), seed, kind)
        return (M32.tie_words if gen == "ties" else M32.random_words)((cols,), seed)
    if gen == "never":
        u = row_narrowing_at(NEVER, cols, seed, bits)
    elif gen.startswith("level"):
        u = row_narrowing_at(min(int(gen[5:]), bits // 8 - 2), cols, seed, bits)
    else:
        size = cap + (1 if "+1" in gen else 0)
        level = min(int(gen[-1]), bits // 8 - 2)
        u = row_bucket_of(size, level, cols, min(k_below_of(k), cols - size), seed, bits)
    return raw_of(u, kind, largest)


def sweep_case(rng, tile, consts, sort_div):
    """One case of the sweep: shape, k, kind, direction, the options and the input words, with the
    path the call takes ("select" or "sort": rows longer than the tile never take the short path)
    and, for the select, each row's narrowing level."""
    chunk = consts["TK_CHUNK"]
    if rng.integers(0, 3) == 0:
        ms = [m for m in range(1, (1 << 18) // chunk + 1) if m * chunk - 1 > tile]
        cols = int(rng.choice(ms)) * chunk + int(rng.integers(-1, 2))
        cols = min(cols, 1 << 18)
    else:
        cols = int(np.exp(rng.uniform(np.log(tile + 1), np.log(1 << 18))))
        cols = min(max(cols, tile + 1), 1 << 18)
    rows = int(rng.integers(1, min(6, (1 << 20) // cols) + 1))
    k = min(max(int(np.exp(rng.uniform(0.0, np.log(cols)))), 1), cols)
    kind = KINDS[int(rng.integers(0, len(KINDS)))]
    largest = bool(rng.integers(0, 2))
    with_idx = bool(rng.integers(0, 2))
    in_off = int(rng.integers(0, 2))
    cap = cap_of(cols, consts)
    gens = [ROW_GENS[int(rng.integers(0, len(ROW_GENS)))] for _ in range(rows)]
    x = np.stack([sweep_row(g, cols, k, kind, largest, cap, int(rng.integers(0, 1 << 31))) for g in gens])
    path = "select" if select_runs(cols, k, sort_div) else "sort"
    levels = None
    if path == "select":
        u = u_of(x, kind, largest)
        levels = [narrow_level(u[r], k, cap, levels_of(kind)) for r in range(rows)]
    tag = f"{kind} ({rows}, {cols}) k={k} largest={largest} idx={with_idx} in_off={in_off} {path} rows={gens} levels={levels}"
    return dict(rows=rows, cols=cols, k=k, kind=kind, largest=largest, with_idx=with_idx, in_off=in_off, x=x, path=path,
                levels=levels, tag=tag)


SWEEP_SEEDS = (71, 72, 73)
SWEEP_CASES = 40


def sweep_cases(seed, tile, consts, sort_div):
    rng = np.random.default_rng(seed)
    for _ in range(SWEEP_CASES):
        yield sweep_case(rng, tile, consts, sort_div)
