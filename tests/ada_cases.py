"""Adaptive strength of the discriminator augmentation (csrc/csg_augment.h: `aug_gate`, `ada_next_p`; csrc/augment.hip: the
gate, sign and update kernels): restatements in Python integers and numpy uint64, and fixed vectors worked out once with them.
tests/test_ada_cases.py holds the host half of the shared header to them; tests/test_gpu_ada.py holds the device to them.

THE GATE.  With h the sample's key (tests/augment_cases.py: `key_py`), policy j = 0, 1, 2 (colour, translation, cutout) is on
iff  step(h, 8 + j) >> 40 < p24,  p24 an integer in [0, 2^24]:  p = p24 * 2^-24.  A draw has 24 bits, so p24 = 2^24 turns
every policy on and p24 = 0 every policy off.  Draws 1..7 — the parameter rows — are untouched.

THE CONTROLLER.  Eight int64 words [p24, S, C, updates, S_last, C_last, 0, 0].  S = sum of sign(x), C = number of elements x;
sign(x) = +1 for x > 0, -1 for x < 0, 0 for +0, -0 and NaN.  One update:
    d = S * 2^24 - T24 * C         (Python integers here: no overflow to think about)
    p24' = clamp(p24 + sgn(d) * step24, 0, 2^24);   C = 0 or d = 0: p24' = p24
then S_last = S, C_last = C, S = C = 0, updates += 1.  d > 0 is r_t = S / C > T: the discriminator is too sure of the real
pictures and p goes up.
"""
import numpy as np

import augment_cases as ac

ONE = 1 << 24
MAX_COUNT = 1 << 38
WORDS = 8
P24_VALUES = [0, 1, 1 << 23, ONE - 1, ONE]
KEYS = [(0, 0, 0, 0), (0, 1, 2, 0), (12345, 7, 1, 1), ((1 << 64) - 1, (1 << 63) - 1, 5, 3), (7, 123456789, 2, (1 << 31) - 1)]
#        (seed, iteration, pass, rank)


# ------------------------------------------------------------------------------------------------ the gate
def gate_py(seed, iteration, pass_id, rank, n, p24):
    h = ac.key_py(seed, iteration, pass_id, rank, n)
    return sum(1 << j for j in range(3) if (ac.step_py(h, 8 + j) >> 40) < p24)


def gate_np(seed, iteration, pass_id, rank, rows, p24):
    """(rows,) int32: the masks the gate entries write."""
    n = np.arange(rows, dtype=np.uint64)
    h = ac.step_np(ac.step_np(ac.step_np(ac.step_np(np.uint64(0), np.uint64(seed)), np.uint64(iteration)), np.uint64(pass_id)),
                   (np.uint64(rank) << np.uint64(32)) | n)
    out = np.zeros(rows, np.int32)
    for j in range(3):
        u = (ac.step_np(h, np.uint64(8 + j)) >> np.uint64(40)).astype(np.int64)
        out |= ((u < p24).astype(np.int32) << j)
    return out


# (seed, iteration, pass, rank, n) -> the three 24-bit draws 8, 9, 10: worked out once with ac.key_py / ac.step_py
DRAW_VECTORS = [
    ((0, 0, 0, 0, 0), (426660, 15499297, 5947316)),
    ((0, 1, 2, 0, 1), (7131770, 1584343, 7437176)),
    ((12345, 7, 1, 1, 299), (3631552, 11891745, 7984934)),
    (((1 << 64) - 1, (1 << 63) - 1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1), (14190851, 576324, 7247855)),
]
# rows 0..7 of (seed, iteration, pass, rank) = GATE_VECTORS_KEY at p24 = 2^23
GATE_VECTORS_KEY = (12345, 7, 1, 1)
GATE_VECTORS = [0, 3, 2, 0, 3, 4, 3, 6]


# ------------------------------------------------------------------------------------------------ the controller
def next_p(p24, S, C, T24, step24):
    if C <= 0:
        return p24
    d = S * ONE - T24 * C
    if d == 0:
        return p24
    return min(max(p24 + (step24 if d > 0 else -step24), 0), ONE)


def update_words(words, T24, step24):
    p24, S, C, updates = (int(v) for v in words[:4])
    return [next_p(p24, S, C, T24, step24), 0, 0, updates + 1, S, C, int(words[6]), int(words[7])]


T06 = 10066330                       # round(0.6 * 2^24)
# (p24, S, C, T24, step24) -> p24': both clamps, C = 0, d = 0 exactly, negative S, step24 = 1, a step larger than the range,
# the largest count the entry takes.  Written by hand from the rule; next_p is held to it in tests/test_ada_cases.py.
NEXT_P_TABLE = [
    ((0, 0, 0, T06, 1000), 0),                           # C = 0: unchanged
    ((500, 0, 0, T06, 1000), 500),
    ((500, 7, 10, T06, 1000), 1500),                     # 0.7 > 0.6: up
    ((500, 6, 10, T06, 1000), 0),                        # 0.6 < T06 / 2^24 = 0.60000002...: down, clamped at 0
    ((5000, 5, 10, T06, 1000), 4000),                    # down
    ((ONE - 10, 10, 10, T06, 1000), ONE),                # clamped at 2^24
    ((ONE, 10, 10, T06, 1), ONE),
    ((ONE, -10, 10, T06, 1), ONE - 1),                   # negative S, step24 = 1
    ((0, -3, 10, T06, 1), 0),                            # clamped at 0
    ((1, -3, 10, T06, 1), 0),
    ((1 << 23, 1, 2, 1 << 23, 77), 1 << 23),             # d = 0 exactly: S / C = T = 0.5
    ((1 << 23, 3, 4, 3 << 22, 77), 1 << 23),             # d = 0 exactly: 0.75
    ((1 << 23, 2, 4, 3 << 22, 77), (1 << 23) - 77),
    ((1 << 23, 4, 4, 3 << 22, 77), (1 << 23) + 77),
    ((1 << 23, 0, 5, 1, 1), (1 << 23) - 1),              # S = 0, the smallest target above 0
    ((1 << 23, 1, ONE, 1, 1), 1 << 23),                  # d = 0 with T24 = 1: S / C = 2^-24
    ((123, 1, 1, ONE - 1, 1 << 40), ONE),                # a step far larger than the range
    ((ONE - 123, -1, 1, ONE - 1, 1 << 40), 0),
    ((1000, MAX_COUNT - 1, MAX_COUNT - 1, ONE, 5), 1000),            # d = 0 at the largest count
    ((1000, MAX_COUNT - 1, MAX_COUNT - 1, ONE - 1, 5), 1005),
    ((1000, -(MAX_COUNT - 1), MAX_COUNT - 1, ONE, 5), 995),
]


def step24(batch_size, world_size, interval, kimg):
    """max(1, round(batch_size world_size interval 2^24 / (1000 kimg))) with halves rounded up, in integers: kimg is given as a
    ratio (numerator, denominator) or an integer."""
    num, den = kimg if isinstance(kimg, tuple) else (kimg, 1)
    a, b = batch_size * world_size * interval * ONE * den, 1000 * num
    return max(1, (2 * a + b) // (2 * b))


# (batch_size, world_size, K, M) -> step24, by hand:  4 * 1 * 4 * 2^24 / 500000 = 536.87 -> 537;  32 * 8 * 4 * 2^24 / 500000
# = 34359.74 -> 34360;  2 * 1 * 2 * 2^24 / 8 = 8388608 (M = 0.008);  1 * 1 * 1 * 2^24 / 10^11 < 0.5 -> the floor of 1
STEP24_VECTORS = [((4, 1, 4, 500), 537), ((32, 8, 4, 500), 34360), ((2, 1, 2, (8, 1000)), 8388608), ((1, 1, 1, 100000000), 1)]


# ------------------------------------------------------------------------------------------------ signs
def sign_count(maps):
    """(S, C) over numpy float32 arrays: +1 for x > 0, -1 for x < 0, 0 for both zeros and NaN; every element counts."""
    S = sum(int((m > 0).sum()) - int((m < 0).sum()) for m in maps)
    return S, sum(int(m.size) for m in maps)


SPECIALS = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.0, -1.0,
                     3.4028235e38, -3.4028235e38, 2.5, -0.125], np.float32)
MAP_SIZES = [1, 63, 64, 65, 255, 256, 257]


def sign_map(n, seed):
    """A (1, 1, 1, n)-shaped float32 map holding the special values (as many as fit) among ordinary ones, about 60 % positive."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-0.8, 1.2, size=n)).astype(np.float32)
    k = min(n, len(SPECIALS))
    x[rng.choice(n, size=k, replace=False)] = rng.permutation(SPECIALS)[:k]
    return x.reshape(1, 1, 1, n)
