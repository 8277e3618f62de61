"""Inputs for the pass-skip logic of the LDS class kernels (the dense row sort, the 16-bit long rows
and the segmented sorts) and the seeded sweeps of those three entries, shared by
test_sort_sweep_model.py and the test_gpu_* files.

The class kernels form, per unit (row or segment), the bits in which the unit's order images differ
and skip each of the 8-bit passes whose digit is uniform.  digit_mask_rows builds rows whose images
differ in exactly a chosen set of digits, by as little as one bit or in one key only; mask_of reads
the set back.  A mask has one bit per digit, bit 0 for the low byte: four bits for "u32" / "i32" /
"f32", two for "bf16" / "f16" (the two bytes of the 16-bit image, digits 2 and 3 of the row sort's
packed word).  The generators work on the order image u (topk_model.u_of: plain unsigned order is
the order asked for, the direction included) and map it back with topk_model.raw_of.

Arrays are uint32 or uint16 words; kind is a key of rowsort_model.KINDS.  Nothing here calls the
library: the shapes of the kernels (class edges, tiles, chunk) are arguments."""
import numpy as np

import f16_model as M16
import f32_model as M32
import rowsort_model as R
import topk_model as T

VARIANTS = ("full", "onebit", "lone_first", "lone_last", "lone_mid")


def ndigits(kind):
    return T.levels_of(kind)


def masks_of(kind):
    """Every mask of the kind's width, 0 (an all-equal row) included."""
    return list(range(1 << ndigits(kind)))


def mask_of(u):
    """u: (rows, cols) order images.  Per row the set of digits in which the row's images differ."""
    u = np.asarray(u)
    assert u.ndim == 2 and u.dtype in (np.uint32, np.uint16)
    d = np.bitwise_or.reduce(u, axis=1) ^ np.bitwise_and.reduce(u, axis=1)
    out = np.zeros(u.shape[0], dtype=np.int64)
    for i in range(u.dtype.itemsize):
        out |= (((d >> u.dtype.type(8 * i)) & u.dtype.type(0xFF)) != 0).astype(np.int64) << i
    return out


def lone_position(variant, cols, seed, r):
    """Where row r of a lone_* matrix holds its lone key.  lone_mid: a random position, inside the
    row when it has an inside."""
    if variant == "lone_first":
        return 0
    if variant == "lone_last":
        return cols - 1
    assert variant == "lone_mid"
    rng = np.random.default_rng([seed, 0x10AE, r, cols])
    return int(rng.integers(1, cols - 1)) if cols >= 3 else int(rng.integers(0, cols))


def _digit_range(i, nd):
    """The values digit i may take: the top byte stays within TOP_LO .. TOP_HI (topk_model)."""
    return (T.TOP_LO, T.TOP_HI) if i == nd - 1 else (0, 256)


def _mask_row(rng, mask, cols, nd, variant, lone_at=None, lone_smaller=False):
    """One row of order images (uint64) whose digits differ exactly in `mask`."""
    assert 0 <= mask < (1 << nd) and variant in VARIANTS and cols >= 1
    u = np.zeros(cols, dtype=np.uint64)
    top = max((i for i in range(nd) if (mask >> i) & 1), default=-1)
    for i in range(nd):
        lo, hi = _digit_range(i, nd)
        sh = np.uint64(8 * i)
        if not (mask >> i) & 1 or cols == 1:
            u |= np.uint64(int(rng.integers(lo, hi))) << sh  # one value per row
            continue
        if variant == "full":
            d = rng.integers(lo, hi, size=cols, dtype=np.uint64)
            if bool((d == d[0]).all()):  # (lo .. hi is closed under ^ 1)
                d[int(rng.integers(0, cols))] ^= np.uint64(1)
        elif variant == "onebit":
            while True:
                v0, bit = int(rng.integers(lo, hi)), int(rng.integers(0, 8))
                if lo <= (v0 ^ (1 << bit)) < hi:
                    break
            pick = rng.integers(0, 2, size=cols, dtype=np.uint64)
            p, q = rng.choice(cols, size=2, replace=False)  # both values occur
            pick[p], pick[q] = 0, 1
            d = np.uint64(v0) ^ (pick << np.uint64(bit))
        else:
            base = int(rng.integers(lo + 1, hi - 1))
            if i == top:  # the highest differing digit orders the lone key against the rest
                lone = int(rng.integers(lo, base)) if lone_smaller else int(rng.integers(base + 1, hi))
            else:
                lone = int(rng.integers(lo, hi - 1))
                lone += lone >= base
            d = np.full(cols, base, dtype=np.uint64)
            d[lone_at] = lone
        u |= d << sh
    return u


def digit_mask_rows(masks, cols, seed, kind, descending=False, variant="full"):
    """(len(masks), cols) words of the kind.  Row r's order images (under the direction) differ in
    exactly the digits of masks[r]; its other digits hold one random value per row, the top byte within
    TOP_LO .. TOP_HI, so every image is the image of a word and none of a NaN.
      full        masked digits random per key
      onebit      each masked digit takes two values that differ in one randomly chosen bit
      lone_first, lone_last, lone_mid   every key equal but the one at lone_position(), which differs
                  in all masked digits and is smaller than the rest in even rows, larger in odd ones
    cols == 1 or a mask of 0 gives an all-equal row."""
    nd = ndigits(kind)
    out = np.empty((len(masks), cols), dtype=T.word_dtype(kind))
    for r, m in enumerate(masks):
        rng = np.random.default_rng([seed, 0xD161, r, cols, int(m), VARIANTS.index(variant)])
        at = lone_position(variant, cols, seed, r) if variant.startswith("lone") else None
        out[r] = _mask_row(rng, int(m), cols, nd, variant, at, r % 2 == 0).astype(out.dtype)
    return T.raw_of(out, kind, descending)


# ---- the layouts of the test_digit_masks tests ----

def mask_matrix(kind, cols, seed, descending=False):
    """Every mask x every variant as the rows of one matrix (80 rows for the 32-bit kinds, 20 for
    the 16-bit ones), and each row's (mask, variant)."""
    masks = masks_of(kind)
    x = np.concatenate([digit_mask_rows(masks, cols, seed + i, kind, descending, v) for i, v in enumerate(VARIANTS)])
    return np.ascontiguousarray(x), [(m, v) for v in VARIANTS for m in masks]


MASK_SEGMENT_LENGTHS = (1, 2, 33, 64, 65, 200, 400, 900, 3000, 9000)
TILE_VARIANTS = ("full", "onebit", "lone_last")  # of a segment as long as the tile


def mask_segments(kind, T_len, seed):
    """The segmented sorts' digit-mask input: for each length of MASK_SEGMENT_LENGTHS and for T_len
    (the tile) a segment per mask x variant (at T_len: TILE_VARIANTS only), lengths ascending, so the
    segments start at odd offsets.  Returns (keys, offsets, [(length, mask, variant)])."""
    masks = masks_of(kind)
    parts, lengths, labels = [], [], []
    for length in MASK_SEGMENT_LENGTHS + (T_len,):
        for i, v in enumerate(VARIANTS if length != T_len else TILE_VARIANTS):
            parts.append(digit_mask_rows(masks, length, seed + 16 * i + length, kind, False, v).reshape(-1))
            lengths += [length] * len(masks)
            labels += [(length, m, v) for m in masks]
    offs = np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.uint32)
    return np.concatenate(parts), offs, labels


def assert_ties_in_position_order(x, gi, kind, descending, msg=""):
    """x: (rows, cols) input words, gi: the positions a sort returned.  The images read through gi
    ascend, and equal ones come in position order."""
    u = R.u_of(np.take_along_axis(x, gi.astype(np.int64), axis=1), kind, descending).astype(np.int64)
    du = np.diff(u, axis=1)
    assert bool((du >= 0).all()), f"not sorted: {msg}"
    assert bool((np.diff(gi.astype(np.int64), axis=1)[du == 0] > 0).all()), f"equal keys out of position order: {msg}"


# ---- row generators of the sweeps, by name ----
PLAIN_GENS = ("random", "ties", "planted", "normal", "sorted", "reversed", "all_equal", "all_nan")


def _nan_words(rng, cols, kind):
    """all_nan: NaNs of several payloads and both signs; the largest key for the integer kinds."""
    if kind == "f32":
        pool = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32)
    elif R.is16(kind):
        s = M16.specials(kind)
        pool = np.array([s["qnan"], s["-qnan1"], s["snan"], s["-snan"], 0x7FFF, 0xFFFF], dtype=np.uint16)
    else:
        pool = np.array([R.nan_word(kind)], dtype=np.uint32)
    return pool[rng.integers(0, pool.size, size=cols)]


def sweep_row(gen, cols, kind, descending, rng):
    """One row (or segment) of words of the kind from the named generator: one of PLAIN_GENS or
    "mask:<m>:<variant>"."""
    seed = int(rng.integers(0, 1 << 31))
    if gen.startswith("mask:"):
        _, m, variant = gen.split(":")
        at = lone_position(variant, cols, seed, 0) if variant.startswith("lone") else None
        u = _mask_row(rng, int(m), cols, ndigits(kind), variant, at, bool(seed & 1)).astype(T.word_dtype(kind))
        return T.raw_of(u, kind, descending)
    if gen == "ties":
        return R.tie_words((cols,), seed, kind)
    if gen == "planted":
        return R.planted_words((cols,), seed, kind)
    if gen == "normal":  # (integer kinds: the float32 words, whose top byte is concentrated)
        return M16.normal_words((cols,), seed, kind) if R.is16(kind) else M32.normal_words((cols,), seed)
    if gen == "all_nan":
        return _nan_words(rng, cols, kind)
    x = R.random_words((cols,), seed, kind)
    if gen == "all_equal":
        return np.full(cols, x[0], dtype=x.dtype)
    if gen in ("sorted", "reversed"):
        x = x[np.argsort(R.u_of(x, kind, descending), kind="stable")]
        return x[::-1].copy() if gen == "reversed" else x
    assert gen == "random", gen
    return x


def pick_gen(rng, kind):
    """Half of the rows from a mask generator (mask and variant random), half from a plain one."""
    if rng.integers(0, 2):
        return f"mask:{int(rng.integers(0, 1 << ndigits(kind)))}:{VARIANTS[int(rng.integers(0, len(VARIANTS)))]}"
    return PLAIN_GENS[int(rng.integers(0, len(PLAIN_GENS)))]


def _gens_tag(gens):
    return "[" + " ".join(gens[:12]) + (f" ... {len(gens)} in all" if len(gens) > 12 else "") + "]"


# ---- the row sort's sweep ----
ROWSORT_SEEDS = (83, 84, 85)
ROWSORT_CASES = 40
GRIDS = (None, "rows", "fixed")  # LABSORT_ROWSORT_GRID: unset, or one form forced


def rowsort_path(kind, cols, with_idx, edges, tile, pair_tile):
    """Where labsort_sort_rows_device sorts rows of this length: "short" (one key per lane, in the
    first wave class's kernel), "class0" .. "class4" (the LDS classes: edges are their upper bounds
    below the tile) or "long" (past the tile that holds the call)."""
    if cols > (tile if (R.is16(kind) or not with_idx) else pair_tile):
        return "long"
    if cols <= 64:
        return "short"
    return f"class{sum(cols > e for e in edges)}"


def rowsort_sweep_cases(seed, edges, tile, pair_tile):
    """ROWSORT_CASES cases: a kind, 1 .. 48 rows with rows * cols <= 2^19; cols in every third
    case on a class or tile edge +-1, in a tenth past the tile up to 40000 (the long path), else
    log-uniform in 1 .. tile; direction, positions, grid form and (16-bit kinds) the offsets of the
    matrices in their storages random; every row from its own generator.  edges: the class bounds
    below the tile (segment_class_edges(False)[:-1])."""
    marks = [64] + list(edges) + [pair_tile, tile]
    for i in range(ROWSORT_CASES):
        rng = np.random.default_rng([seed, 0x5EE9, i])
        kind = R.KINDS[int(rng.integers(0, len(R.KINDS)))]
        src = int(rng.integers(0, 20))
        if i % 3 == 0:
            cols = int(rng.choice(marks)) + int(rng.integers(-1, 2))
        elif src < 3:
            cols = int(rng.integers(tile + 1, 40001))
        else:
            cols = min(max(int(np.exp(rng.uniform(0.0, np.log(tile + 1)))), 1), tile)
        rows = int(rng.integers(1, min(48, (1 << 19) // cols) + 1))
        descending, with_idx = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        grid = GRIDS[int(rng.integers(0, len(GRIDS)))]
        in_off, out_off = (int(rng.integers(0, 2)), int(rng.integers(0, 2))) if R.is16(kind) else (0, 0)
        gens = [pick_gen(rng, kind) for _ in range(rows)]
        x = np.stack([sweep_row(g, cols, kind, descending, rng) for g in gens]).astype(R.wdtype(kind))
        path = rowsort_path(kind, cols, with_idx, edges, tile, pair_tile)
        tag = (f"rowsort seed={seed} case={i} {kind} ({rows}, {cols}) descending={descending} idx={with_idx} grid={grid} "
               f"in_off={in_off} out_off={out_off} {path} rows={_gens_tag(gens)}")
        yield dict(kind=kind, rows=rows, cols=cols, descending=descending, with_idx=with_idx, grid=grid, in_off=in_off,
                   out_off=out_off, gens=gens, x=x, path=path, tag=tag)


# ---- the 16-bit long rows' sweep ----
SORT16_SEEDS = (91, 92, 93)
SORT16_CASES = 16
ENTRIES = ("sort16", "rows")


def sort16_sweep_cases(seed, C, tile):
    """SORT16_CASES cases on the long path: both 16-bit kinds, 1 .. 4 rows, tile < cols <= 6 C, half of
    the widths from {m C - 1, m C, m C + 1}; direction, positions, offsets and the entry
    (labsort_sort16_device or labsort_sort_rows_device) random; every row from its own generator.  (A
    2-bit mask with a digit clear: that radix pass puts every chunk into one bin.)"""
    for i in range(SORT16_CASES):
        rng = np.random.default_rng([seed, 0x5167, i])
        kind = M16.KINDS[int(rng.integers(0, 2))]
        edge = None
        if i % 2:
            while True:
                m, d = int(rng.integers(2, 7)), int(rng.integers(-1, 2))
                cols = m * C + d
                if tile < cols <= 6 * C:
                    break
            edge = ("mC-1", "mC", "mC+1")[d + 1]
        else:
            cols = int(rng.integers(tile + 1, 6 * C + 1))
        rows = int(rng.integers(1, 5))
        descending, with_idx = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        in_off, out_off = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        entry = ENTRIES[int(rng.integers(0, 2))]
        gens = [pick_gen(rng, kind) for _ in range(rows)]
        x = np.stack([sweep_row(g, cols, kind, descending, rng) for g in gens]).astype(np.uint16)
        tag = (f"sort16 seed={seed} case={i} {kind} ({rows}, {cols}) descending={descending} idx={with_idx} in_off={in_off} "
               f"out_off={out_off} entry={entry} edge={edge} rows={_gens_tag(gens)}")
        yield dict(kind=kind, rows=rows, cols=cols, descending=descending, with_idx=with_idx, in_off=in_off, out_off=out_off,
                   entry=entry, edge=edge, gens=gens, x=x, tag=tag)


# ---- the float32 segmented sort's sweep ----
F32SEG_SEEDS = (101, 102, 103)
F32SEG_CASES = 60


def f32_segment_sweep_cases(seed, tile, pair_tile):
    """F32SEG_CASES cases shaped like test_gpu_segsort.py's seeded stress: n <= 2^17 keys cut at random
    places (empty segments among them), every third case into 1 .. 11 long segments, else into a
    log-uniform 1 .. 2000; max_segment_keys the true maximum or 0; keys or pairs with random
    payloads; in place or out of place; every segment from its own generator.  path: "lds" when the
    promise is at most the tile that holds the call, else "general"."""
    for i in range(F32SEG_CASES):
        rng = np.random.default_rng([seed, 0xF5E6, i])
        # (n >= 1: a call without keys returns before it clears the workspace header the status call reads)
        n = (1 << 17) if i == 1 else int(rng.integers(1, (1 << 17) + 1)) if i else 1
        nseg = int(rng.integers(1, 12)) if i % 3 == 0 else int(np.exp(rng.uniform(0.0, np.log(2000.0))))
        cuts = np.sort(rng.integers(0, n + 1, size=nseg - 1))
        offs = np.concatenate(([0], cuts, [n])).astype(np.uint32)
        pairs, inplace = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        true_max = int(np.diff(offs.astype(np.int64)).max())
        m = true_max if rng.integers(0, 2) else 0
        keys = np.empty(n, dtype=np.uint32)
        gens = []
        for a, b in zip(offs[:-1], offs[1:]):
            g = pick_gen(rng, "f32")
            gens.append(g)
            if b > a:
                keys[int(a):int(b)] = sweep_row(g, int(b) - int(a), "f32", False, rng)
        vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) if pairs else None
        path = "lds" if 0 < m <= (pair_tile if pairs else tile) else "general"
        tag = (f"f32 segments seed={seed} case={i} n={n} nseg={nseg} longest={true_max} m={m} pairs={pairs} inplace={inplace} "
               f"{path} segments={_gens_tag(gens)}")
        yield dict(n=n, nseg=nseg, offs=offs, m=m, pairs=pairs, inplace=inplace, keys=keys, vals=vals, gens=gens, path=path,
                   true_max=true_max, tag=tag)
