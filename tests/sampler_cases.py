"""Shared inputs of the sampler tests (test_sampler_api.py on the CPU, test_gpu_sampler.py on the
device): a scalar restatement of the draw in plain Python ints, the random small case and the
edge users. Everything is built once per process and never modified."""
import functools

import numpy as np

from gcn_recommendation_amd.evaluate import mask_csr

M32 = 0xFFFFFFFF

# (counter words, key words) -> output words: the known answers of Philox4x32-10
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32,) * 4, (M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_py(ctr, key):
    """Philox4x32-10 on Python ints."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def kth_missing_py(L, j):
    """The j-th (0-based) non-negative integer not in the sorted list L, by counting."""
    return j + sum(1 for t, x in enumerate(L) if x - t <= j)


def draw_py(idx, L, n_items, seed, epoch):
    """The negative of interaction idx for a user with sorted positives L; -1 without a free item."""
    n_free = n_items - len(L)
    if n_free <= 0:
        return -1
    o = philox_py((idx & M32, idx >> 32, epoch, 0), (seed & M32, seed >> 32))
    j = (((o[1] << 32) | o[0]) * n_free) >> 64
    return kth_missing_py(L, j)


class Case:
    """Low-level inputs of one draw: interactions, the positive CSR (which the edge cases build
    by hand: a user without positives has no interaction to derive them from), sizes."""

    def __init__(self, user, item, rowptr, pos_items, U, I):
        self.user = np.ascontiguousarray(user, dtype=np.int32)
        self.item = np.ascontiguousarray(item, dtype=np.int32)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.pos_items = np.ascontiguousarray(pos_items, dtype=np.int32)
        self.U, self.I = U, I
        for a in (self.user, self.item, self.rowptr, self.pos_items):
            a.setflags(write=False)

    def __len__(self):
        return len(self.user)

    def positives(self, u):
        return [int(x) for x in self.pos_items[self.rowptr[u]:self.rowptr[u + 1]]]


@functools.lru_cache(maxsize=None)
def random_case():
    """U = 50, I = 37, 600 interactions with duplicates; user 7 never appears."""
    rng = np.random.default_rng(20240611)
    U, I, n = 50, 37, 600
    user = rng.integers(0, U, n)
    user[user == 7] = 8
    item = rng.integers(0, I, n)
    user[500:] = user[:100]   # duplicates of whole interactions
    item[500:] = item[:100]
    rowptr, pos_items = mask_csr(user, item, U)
    return Case(user, item, rowptr, pos_items, U, I)


EDGE_I = 9
EDGE_LISTS = {
    "deg0": [],
    "free_first": list(range(1, EDGE_I)),
    "free_last": list(range(EDGE_I - 1)),
    "free_middle": [x for x in range(EDGE_I) if x != 4],
    "full": list(range(EDGE_I)),
    "run_at_start": [0, 1, 2, 3],
    "run_at_end": [5, 6, 7, 8],
    "alternating_even": [0, 2, 4, 6, 8],
    "alternating_odd": [1, 3, 5, 7],
}
EDGE_SAMPLES = 200  # of the edge user (user 1); user 0 (positives [3]) has 40 in between


@functools.lru_cache(maxsize=None)
def edge_case(name):
    L = EDGE_LISTS[name]
    user = np.array([1] * EDGE_SAMPLES + [0] * 40)
    user = user[np.random.default_rng(5).permutation(user.size)]
    item = np.where(user == 0, 3, L[0] if L else 0)
    return Case(user, item, [0, 1, 1 + len(L)], [3] + L, 2, EDGE_I)
