"""Every digit mask through every whole-array radix path: arrays whose order images differ in exactly
a chosen set of the four digits (tests/sort_sweep_model.py: 16 masks x 5 variants, by as little as
one bit or in one key only; for the integer kinds also with every other digit 0xFF, the sentinel's
digit) sorted by the onesweep passes and the gathered passes (LABSORT_RADIX_IMPL), keys only, and by
labsort_sort_pairs_device with the radix, the merge sort and the one-tile path.  The sixteen masks
are the sixteen sets of active passes of k_plan8: every segment mode as the first and as a later
pass, every ping-pong route and every copy_from (tests/whole_sort_model.py: radix_plan_model, which
names the plan in a failure).  Protocol and expected result: tests/whole_sort_run.py.

One test id per entry, key type, size and in place / out of place; each loops over the masks and the
variants and reports every array that failed."""
import functools

import numpy as np
import pytest

import sort_sweep_model as S
import topk_model as T
import whole_sort_model as W
import whole_sort_run as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def cases(kind, n):
    """[(mask, variant, words, perm)] of one kind and size: computed once, shared by the ids that
    differ in entry and in place, never written."""
    variants = W.GATHER_VARIANTS if n == W.GATHER_SIZE else S.VARIANTS
    arrays = W.mask_arrays(kind, n, W.MASK_SEED, variants)
    if kind != "f32":
        arrays = arrays + W.ff_arrays(kind, n, W.MASK_SEED)
    out = []
    for (m, v), x in arrays:
        perm = np.argsort(T.u_of(x, kind, False), kind="stable").astype(np.uint32)
        x.setflags(write=False)
        perm.setflags(write=False)
        out.append((m, v, x, perm))
    return out


def run_all(kind, n, inplace, one):
    """one(x, ek, perm) -> None or what went wrong, over every array; the failures with mask, variant
    and the radix plan of the call."""
    failures = []
    for m, v, x, perm in cases(kind, n):
        why = one(x, x[perm], perm)
        if why:
            plan = W.radix_plan_model(T.u_of(x, kind, False), W.sorts_in_place(kind, inplace))
            failures.append(f"mask {m:#x} {v}: {why} [{W.plan_tag(plan)}]")
    assert not failures, f"{len(failures)} of {len(cases(kind, n))} arrays: " + "; ".join(failures[:6])


# (implementation, size): both at the onesweep sizes, the gathered passes also at their own two
KEYS_CASES = [(impl, n) for n in W.ONESWEEP_SIZES for impl in ("onesweep", "gather")] + [
    ("gather", W.GATHER_FUSED_SIZE), ("gather", W.GATHER_SIZE)]


@pytest.mark.parametrize("kind", ["u32", "i32"])
@pytest.mark.parametrize("impl,n", KEYS_CASES)
@pytest.mark.parametrize("inplace", [False, True])
def test_keys_digit_masks(ls, torch_gpu, monkeypatch, inplace, impl, n, kind):
    """labsort_sort_device(LABSORT_ALGO_RADIX) with the implementation forced.  40000: three onesweep
    tiles, every nibble segment shorter than a tile, above the 32768-key small path; 300007: 19 tiles,
    a single chain looks back over three windows; 131077: the gathered passes' fused path, whose skip
    test reads the per-tile digit min / max pairs; 2^20 + 8192 + 5: their non-fused form (three of the
    variants there)."""
    monkeypatch.setenv("LABSORT_RADIX_IMPL", impl)
    assert ls.radix_impl(n) == impl
    run_all(kind, n, inplace, lambda x, ek, perm: R.check_keys(ls, torch_gpu, x, ek, kind, "radix", inplace))


# (algorithm, size): the merge sort at the smaller size only
PAIRS_CASES = [("radix", n) for n in W.ONESWEEP_SIZES] + [("merge", W.ONESWEEP_SIZES[0])]


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("algo,n", PAIRS_CASES)
@pytest.mark.parametrize("inplace", [False, True])
def test_pairs_digit_masks(ls, torch_gpu, inplace, algo, n, kind):
    """labsort_sort_pairs_device, payloads = positions.  radix: k_onesweep_p<true> under every plan
    (its payloads' route and final copy follow the keys'); merge at 40000: the pass-skip header of
    k_tile_sort<KV> with payloads (three tiles of 16384 pairs), then one four-way pass over the three runs."""
    vals = W.payloads(n)
    run_all(kind, n, inplace,
            lambda x, ek, perm: R.check_pairs(ls, torch_gpu, x, vals, ek, perm, kind, algo, inplace))


@pytest.mark.parametrize("kind", W.KINDS)
@pytest.mark.parametrize("n", W.PAIR_TILE_SIZES)
@pytest.mark.parametrize("inplace", [False, True])
def test_pairs_one_tile_digit_masks(ls, torch_gpu, inplace, n, kind):
    """The one-tile key/value path (n <= 16384: one launch of k_tile_sort<KV>), a full tile and a
    partial one, payloads = a bijection of the positions."""
    assert n <= ls.pair_tile_keys()
    vals = W.payloads(n, True)
    run_all(kind, n, inplace,
            lambda x, ek, perm: R.check_pairs(ls, torch_gpu, x, vals, ek, vals[perm], kind, "auto", inplace))
