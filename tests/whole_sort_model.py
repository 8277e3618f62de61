"""The whole-array device sorts (labsort_sort_device, labsort_sort_pairs_device) as host models, shared
by test_whole_sort_model.py, test_gpu_whole_masks.py and test_gpu_pairs.py: the digit-mask arrays
of sort_sweep_model.py at whole-array sizes, the 8-bit radix plan (csrc/kernels.hip: k_plan8 and
plan_buffers) restated on the order images, the merge sort's pass shapes (csrc/api.hip: sort_merge,
csrc/merge4.hip: m4_geo), the key shapes of the run-edge tests and the seeded key/value sweep.

Arrays are uint32 words; kind is "u32", "i32" or "f32".  The expected result of every sort is
    u = topk_model.u_of(x, kind, False); perm = np.argsort(u, kind="stable"); x[perm], vals[perm].
Nothing here calls the library; the constants come from the headers the kernels are compiled with."""
import glob
import os
import re

import numpy as np

import f32_model as M32
import sort_sweep_model as S
import topk_model as T

KINDS = ("u32", "i32", "f32")
IN, OUT, TMP, SKIP = "IN", "OUT", "TMP", "SKIP"  # common.h: SEL_IN, SEL_OUT, SEL_TMP, SEL_SKIP


# ---- constants, from the headers ----

def _repo():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _common_header():
    found = [h for h in glob.glob(os.path.join(_repo(), "*", "csrc", "common.h"))
             if os.path.exists(os.path.join(os.path.dirname(os.path.dirname(h)), "__init__.py"))]
    assert len(found) == 1, f"csrc/common.h next to the package's __init__.py: {found}"
    return found[0]


def constants():
    """Shape constants of csrc/common.h and the key/value AUTO bound of include/labsort.h.  Each must
    be found: a renamed constant fails here and does not move a test off its edge."""
    with open(_common_header()) as f:
        text = f.read()
    out = {}
    for name in ("OSP_BLOCK", "OSP_KPT", "OSP_LBW", "NSEG", "TS_BLOCK", "TS_KPT", "TS_KPT_KV", "GS_BLOCK", "GS_KPT", "GS_GROUP",
                 "GS_SMALL_NG", "MG_BLOCK", "MG_KPT"):
        m = re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert len(m) == 1, f"{name}: {len(m)} definitions found in csrc/common.h"
        out[name] = int(m[0])
    m = re.findall(r"#define\s+LABSORT_M4_S\s+(\d+)", text)
    assert len(m) == 1, "LABSORT_M4_S"
    out["M4_S"] = int(m[0])
    with open(os.path.join(_repo(), "include", "labsort.h")) as f:
        m = re.findall(r"#define\s+LABSORT_AUTO_PAIRS_MERGE_MAX_KEYS\s+\(1u\s*<<\s*(\d+)\)", f.read())
    assert len(m) == 1, "LABSORT_AUTO_PAIRS_MERGE_MAX_KEYS"
    out["AUTO_PAIRS_MERGE_MAX_KEYS"] = 1 << int(m[0])
    out["OSP_TILE"] = out["OSP_BLOCK"] * out["OSP_KPT"]    # keys per onesweep tile
    out["TILE_KEYS"] = out["TS_BLOCK"] * out["TS_KPT"]     # labsort_tile_keys(): the keys-only small path
    out["PAIR_TILE"] = out["TS_BLOCK"] * out["TS_KPT_KV"]  # labsort_pair_tile_keys(): the one-tile key/value path
    out["GS_TILE"] = out["GS_BLOCK"] * out["GS_KPT"]
    out["MG_TILE"] = out["MG_BLOCK"] * out["MG_KPT"]
    return out


# ---- the sizes of test_gpu_whole_masks.py ----
ONESWEEP_SIZES = (40000, 300007)          # 3 tiles, every nibble segment shorter than a tile; 19 tiles
GATHER_FUSED_SIZE = 131077                # 17 gathered tiles, one scan group: the fused path
GATHER_SIZE = (1 << 20) + 8192 + 5        # 130 gathered tiles, 3 scan groups (more than GS_SMALL_NG): the non-fused form
GATHER_VARIANTS = ("full", "onebit", "lone_mid")  # at GATHER_SIZE
PAIR_TILE_SIZES = (16384, 5000)           # the one-tile key/value path
MASK_SEED = 0xA11


def mask_arrays(kind, n, seed, variants=S.VARIANTS):
    """[((mask, variant), words)]: the rows of digit_mask_rows(masks_of(kind), n, ..., variant) over the
    variants (all five: 80 arrays), ascending order asked for."""
    masks = S.masks_of(kind)
    out = []
    for v in variants:
        x = S.digit_mask_rows(masks, n, seed + S.VARIANTS.index(v), kind, False, v)
        out += [((m, v), x[r]) for r, m in enumerate(masks)]
    return out


def ff_arrays(kind, n, seed):
    """[((mask, "ff"), words)] for the integer kinds: the `full` rows with every digit outside the mask
    set to 0xFF in the order image, the digit of the onesweep passes' sentinel (~flip) in every pass,
    so a skipped digit is a constant that is not zero and the last partial tile's padding ranks among
    real keys of its digit."""
    assert kind in ("u32", "i32")
    out = []
    for (m, _), x in mask_arrays(kind, n, seed + 0xFF, ("full",)):
        u = T.u_of(x, kind, False)
        for i in range(4):
            if not (m >> i) & 1:
                u = u | np.uint32(0xFF << (8 * i))
        out.append(((m, "ff"), T.raw_of(u, kind, False)))
    return out


def expected(x, kind, vals=None):
    """The sorted words (and payloads) by the stable argsort of the order image."""
    perm = np.argsort(T.u_of(x, kind, False), kind="stable")
    return (x[perm], None) if vals is None else (x[perm], vals[perm])


# ---- the 8-bit radix plan ----

def sorts_in_place(kind, in_place):
    """Whether the radix / merge driver runs with IN == OUT: a float32 call maps the keys into the
    output and sorts there in place, whatever the caller passed (api.hip:538-544, labsort_sort_device,
    and api.hip:851-860, labsort_sort_pairs_device: the LABSORT_KEY_F32 branch)."""
    return in_place or kind == "f32"


def radix_plan_model(u, in_place):
    """k_plan8 (csrc/kernels.hip:455-580) and plan_buffers (kernels.hip:143-152) on the host, for the
    classic path (no hybrid: the host gate, api.hip:174-179 and :222, is closed below 2^28 - 2^24 keys
    and for key/value sorts).  The code is the specification; the quoted lines are its.  u: the order
    images.
      active     the digits whose pass runs: k_plan8 calls digit p trivial when one of its 256 counts
                 equals n (:496, "if (v[p] == n) triv[p] = 1")
      modes      per active pass its SegPlan::mode.  The first one: 0 (position segments) when it is
                 digit 0, else 2, one chain (:569-579, "hp = first == 0 ? hps : ... nullptr; if (seg_later < 0
                 || !hp) ... build_segplan(..., 2u, ...)").  A later pass q: 1 (segments by the previous
                 digit's top nibble) when the previous active digit is q - 1, else 2
                 (build_segplan_later, :426-443: "if (seg_later <= 0 || prev + 1u != (uint32_t)q)";
                 launch_plan8 passes seg_later = 1, :1815)
      route      per active pass (src, dst): plan_buffers, :143-152 -- "from_tmp = in_is_out && (k & 1)";
                 pass i writes OUT when "from_tmp ? (i & 1) : !((k - 1 - i) & 1)", else TMP, and
                 reads what the pass before wrote, the first one IN
      copy_from  "(k == 0 && in_is_out) || src == SEL_OUT ? SEL_SKIP : src": IN when nothing runs out
                 of place (pass 0's launch copies), TMP after an odd count of passes in place"""
    u = np.asarray(u, dtype=np.uint32)
    n = u.size
    active = [p for p in range(4) if int(np.bincount((u >> np.uint32(8 * p)) & np.uint32(0xFF), minlength=256).max()) != n]
    k = len(active)
    modes = []
    for i, q in enumerate(active):
        if i == 0:
            modes.append(0 if q == 0 else 2)
        else:
            modes.append(1 if active[i - 1] + 1 == q else 2)
    from_tmp = bool(in_place) and (k & 1) == 1
    src, route = IN, []
    for i in range(k):
        to_out = bool(i & 1) if from_tmp else not ((k - 1 - i) & 1)
        dst = OUT if to_out else TMP
        route.append((src, dst))
        src = dst
    copy_from = SKIP if (k == 0 and in_place) or src == OUT else src
    return dict(active=active, modes=modes, route=route, copy_from=copy_from)


def plan_tag(plan):
    return (f"active={plan['active']} modes={plan['modes']} route={'>'.join([r[0] for r in plan['route'][:1]] + [r[1] for r in plan['route']])}"
            f" copy_from={plan['copy_from']}")


def nibble_segments(u, q):
    """The 16 segment lengths of a mode-1 pass on digit q: the counts of the top nibble of digit q - 1
    (build_segplan_later: "exclusive prefix over nibble groups of hist[prev]")."""
    return np.bincount((np.asarray(u, dtype=np.uint32) >> np.uint32(8 * (q - 1) + 4)) & np.uint32(15), minlength=16)


# ---- the merge sort's passes ----

def merge_shape(n, pairs, consts=None):
    """sort_merge (csrc/api.hip:293-336) with every pointer 16-byte aligned (`four`, :303): the levels
    above the tile sort (merge_levels, :129-133: runs of 32768 keys or 16384 pairs doubled until one
    run), the passes ("pair" first when the level count is odd, then "four" per two levels:
    next_is_four, :309, "(m - lv) % 2 == 0") and per four-way pass over runs of r (m4_geo,
    csrc/merge4.hip:778-795) the runs of its last group and the last run's length."""
    c = consts or constants()
    tile = c["PAIR_TILE"] if pairs else c["TILE_KEYS"]
    m, run = 0, tile
    while run < n:
        m += 1
        run *= 2
    passes, fours, r = [], [], tile
    lv = 0
    while lv < m:
        if (m - lv) % 2 == 0:
            nruns = -(-n // r)
            fours.append(dict(r=r, last_group_runs=(nruns - 1) % 4 + 1, last_run=n - (nruns - 1) * r))
            passes.append("four")
            r *= 4
            lv += 2
        else:
            passes.append("pair")
            r *= 2
            lv += 1
    return dict(levels=m, passes=passes, fours=fours)


# ---- key shapes of test_gpu_pairs.py ----
TIE_VALUES = np.array([0, 0x55555555, 0x7FFFFFFF, 0xAAAAAAAA, 0xFFFFFFFF], dtype=np.uint32)
PAIR_SHAPES = ("ties", "const", "sorted_ties", "reversed_ties", "uniform")
RUN_EDGE_TAILS = (1, 127, 128, 129)


def shape_keys(shape, n, seed, kind="u32"):
    """ties: the five TIE_VALUES at random (0xFFFFFFFF and 0x7FFFFFFF are the sentinel words ~flip of
    u32 and i32); sorted_ties / reversed_ties: the sort of `ties` in the kind's order and its
    reverse; const; uniform."""
    rng = np.random.default_rng([seed, 0x5AFE, n])
    if shape == "uniform":
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if shape == "const":
        return np.full(n, TIE_VALUES[int(rng.integers(0, TIE_VALUES.size))], dtype=np.uint32)
    x = TIE_VALUES[rng.integers(0, TIE_VALUES.size, size=n)]
    if shape == "ties":
        return x
    x = x[np.argsort(T.u_of(x, kind, False), kind="stable")]
    if shape == "reversed_ties":
        return x[::-1].copy()
    assert shape == "sorted_ties", shape
    return x


def payloads(n, bijection=False):
    """Positions, or a bijection of them (an odd multiplier mod 2^32)."""
    v = np.arange(n, dtype=np.uint32)
    return v * np.uint32(2654435761) if bijection else v


# ---- the seeded key/value sweep ----
PAIRS_SEEDS = (111, 112, 113)
PAIRS_CASES = 64
ALGOS = ("radix", "merge", "auto")
OFFSETS = (0, 1, 3)
PLAIN_GENS = ("uniform", "ties", "sorted_ties", "reversed_ties", "extremes", "runs", "f32_random")
EXTREMES = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)


def sweep_edge_sizes(consts):
    t, a = consts["PAIR_TILE"], consts["AUTO_PAIRS_MERGE_MAX_KEYS"]
    e = [1, 2, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, a, a + 1, (1 << 20) - 1, (1 << 20) + 1]
    for k in range(3, 14):
        e += [k * t - 1, k * t, k * t + 1]
    return sorted(set(e))


def _sweep_keys(gen, n, kind, rng):
    seed = int(rng.integers(0, 1 << 31))
    if gen.startswith("mask:"):
        return S.sweep_row(gen, n, kind, False, rng)
    if gen in ("uniform", "ties", "sorted_ties", "reversed_ties"):
        return shape_keys(gen, n, seed, kind)
    if gen == "extremes":
        return EXTREMES[rng.integers(0, EXTREMES.size, size=n)]
    if gen == "f32_random":  # NaNs of both signs, denormals, both zeros and the infinities planted
        return M32.random_words((n,), seed)
    assert gen == "runs", gen
    a = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    i = 0
    while i < n:  # ascending and descending stretches (in plain word order) of random lengths
        L = int(rng.integers(1, 70000))
        seg = np.sort(a[i:i + L])
        a[i:i + L] = seg if rng.random() < 0.5 else seg[::-1]
        i += L
    return a


def pairs_sweep_cases(seed, consts=None):
    """PAIRS_CASES cases of labsort_sort_pairs_device.  Drawn per case: the key type, in place or not,
    the size (every second case from sweep_edge_sizes, else log-uniform in 1 .. 2^21), the four
    views' offsets in words (half of the cases all aligned, else each of keys in / payloads in / keys
    out / payloads out from OFFSETS; in place the outputs are the inputs) and whether the payloads
    are positions or a bijection of them.  Cycled, so that the three seeds meet every combination the
    model test lists: the algorithm (case % 3), and in every second case a mask generator whose mask
    walks through all sixteen (those cases take their size above the one-tile path); the other cases
    draw one of PLAIN_GENS (f32_random for float32 keys only)."""
    c = consts or constants()
    edges = sweep_edge_sizes(c)
    big = [e for e in edges if e > c["PAIR_TILE"]]
    for i in range(PAIRS_CASES):
        rng = np.random.default_rng([seed, 0x9A12, i])
        algo = ALGOS[i % 3]
        kind = KINDS[int(rng.integers(0, 3))]
        inplace = bool(rng.integers(0, 2))
        masked = i % 2 == 0
        if masked:
            m = (i // 2 + 5 * seed) % 16
            gen = f"mask:{m}:{S.VARIANTS[int(rng.integers(0, len(S.VARIANTS)))]}"
        else:
            while True:
                gen = PLAIN_GENS[int(rng.integers(0, len(PLAIN_GENS)))]
                if gen != "f32_random" or kind == "f32":
                    break
        if rng.integers(0, 2):
            n = int(rng.choice(big if masked else edges))
        else:
            lo = c["PAIR_TILE"] + 1 if masked else 1
            n = min(max(int(np.exp(rng.uniform(np.log(lo), np.log(1 << 21)))), lo), 1 << 21)
        if rng.integers(0, 2):
            offs = (0, 0, 0, 0)
        else:
            offs = tuple(int(rng.choice(OFFSETS)) for _ in range(4))
        if inplace:
            offs = (offs[0], offs[1], offs[0], offs[1])
        bijection = bool(rng.integers(0, 2))
        x = np.ascontiguousarray(_sweep_keys(gen, n, kind, rng), dtype=np.uint32)
        runs = "radix" if algo == "radix" or (algo == "auto" and n > c["AUTO_PAIRS_MERGE_MAX_KEYS"]) else "merge"
        if n <= c["PAIR_TILE"]:
            runs = "tile"
        tag = (f"pairs seed={seed} case={i} {kind} n={n} {algo}->{runs} inplace={inplace} offs={offs} bijection={bijection} {gen}")
        yield dict(i=i, n=n, kind=kind, algo=algo, runs=runs, inplace=inplace, offs=offs, bijection=bijection, gen=gen, x=x,
                   tag=tag)
