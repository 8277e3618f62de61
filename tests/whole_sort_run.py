"""One call of labsort_sort_device / labsort_sort_pairs_device under the protocol of
tests/test_gpu_f32_sort.py, shared by test_gpu_whole_masks.py and test_gpu_pairs.py: the workspace
filled with 0xFF, the outputs with a pattern, the status call after the sort, the inputs of an
out-of-place call unchanged, keys and payloads compared exactly (float32: NaN-ness everywhere, every
other word bit-exact).  Every array is a view into a buffer of its own that starts GUARD + offset
words in, between canary words that must survive.  check_* return None or what went wrong."""
import numpy as np

import f32_model as M32

PATTERN = 0x5A5A5A5A
CANARY = 0x0C0FFEE5
GUARD = 4  # words before and after each view: the view is 16-byte aligned when its offset is 0


def same_keys(got, want, kind):
    if kind != "f32":
        return np.array_equal(got, want)
    gn, wn = M32.is_nan(got), M32.is_nan(want)
    return np.array_equal(gn, wn) and np.array_equal(np.where(gn, np.uint32(0), got), np.where(wn, np.uint32(0), want))


class View:
    """n words at GUARD + off words of a canary-filled buffer; x: the words to hold, None: the pattern."""

    def __init__(self, torch, n, off, x=None):
        self.n, self.at = n, GUARD + off
        self.buf = torch.full((self.at + n + GUARD,), CANARY, dtype=torch.int32, device="cuda")
        self.t = self.buf[self.at:self.at + n]
        assert self.t.data_ptr() % 16 == (4 * off) % 16
        if x is None:
            self.t.fill_(PATTERN)
        else:
            self.t.copy_(torch.from_numpy(np.array(x).view(np.int32)))

    def words(self):
        return self.t.cpu().numpy().view(np.uint32)

    def canaries_intact(self):
        edges = np.concatenate([self.buf[:self.at].cpu().numpy(), self.buf[self.at + self.n:].cpu().numpy()])
        return edges.size == self.at + GUARD and bool((edges == CANARY).all())


def _typed(torch, t, kind):
    return t.view(torch.float32) if kind == "f32" else t


def check_keys(ls, torch, x, ek, kind, algo, inplace, offs=(0, 0)):
    """sort_device of the words x; ek: the expected words.  offs: (input, output) view offsets in
    words (in place: the first one)."""
    n = x.size
    src = View(torch, n, offs[0], x)
    dst = src if inplace else View(torch, n, offs[1])
    ws = torch.full((max(ls.workspace_bytes(n, algo), 256),), 0xFF, dtype=torch.uint8, device="cuda")
    ls.sort_device(_typed(torch, src.t, kind), _typed(torch, dst.t, kind), n, key=kind, algo=algo, workspace=ws)
    ls.workspace_status(ws, n, algo)
    if not (src.canaries_intact() and dst.canaries_intact()):
        return "a word outside the views was written"
    if not inplace and not np.array_equal(src.words(), x):
        return "the input was written"
    if not same_keys(dst.words(), ek, kind):
        got = dst.words()
        bad = np.flatnonzero(got != ek)
        return f"keys differ at {bad.size} of {n} places, first at {int(bad[0]) if bad.size else -1}"
    return None


def check_pairs(ls, torch, x, vals, ek, ev, kind, algo, inplace, offs=(0, 0, 0, 0)):
    """sort_pairs_device of (x, vals); offs: the offsets of keys in, payloads in, keys out, payloads
    out (in place: the first two)."""
    n = x.size
    ki, vi = View(torch, n, offs[0], x), View(torch, n, offs[1], vals)
    ko, vo = (ki, vi) if inplace else (View(torch, n, offs[2]), View(torch, n, offs[3]))
    ws = torch.full((max(ls.pairs_workspace_bytes(n, algo), 256),), 0xFF, dtype=torch.uint8, device="cuda")
    ls.sort_pairs_device(_typed(torch, ki.t, kind), vi.t, _typed(torch, ko.t, kind), vo.t, n, key=kind, algo=algo, workspace=ws)
    ls.pairs_workspace_status(ws, n, algo)
    if not all(v.canaries_intact() for v in (ki, vi, ko, vo)):
        return "a word outside the views was written"
    if not inplace and not (np.array_equal(ki.words(), x) and np.array_equal(vi.words(), vals)):
        return "an input was written"
    gk, gv = ko.words(), vo.words()
    if not same_keys(gk, ek, kind):
        bad = np.flatnonzero(gk != ek)
        return f"keys differ at {bad.size} of {n} places, first at {int(bad[0]) if bad.size else -1}"
    if not np.array_equal(gv, ev):
        bad = np.flatnonzero(gv != ev)
        return f"payloads differ at {bad.size} of {n} places, first at {int(bad[0])}: got {int(gv[bad[0]])}, expected {int(ev[bad[0]])}"
    return None
