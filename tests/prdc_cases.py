"""The cases of the k-nearest-neighbour manifold metrics (csrc/manifold.hip, canonicalsg2im_amd/quality.py: precision / recall,
density / coverage) and a restatement of their rules in numpy fp64, written from include/csg_hip.h and DESIGN 4.19c and
not from the kernels.  Host only: tests/test_prdc_cases.py checks the restatement against hand-worked integers and a double
loop, tests/test_gpu_prdc.py checks the device against the restatement.

  the distance   `d2_ref`: sum over the columns in ascending order of t * t, t = (double)u_c - (double)v_c; NaN ranks as +inf
  the radii      `radii_ref`: the k-th smallest distance to the OTHER rows (self excluded by index, ties counted as they come)
  the counts     `counts_ref`: inside[j] = #{i : d2(q_j, f_i) finite and <= r2[i]}, holds[i] = #{j : the same}
  the metrics    `prdc_ref`: the four numbers from those integers, divided as quality.prdc_from_features divides them

Where the features are small integers every t * t and every partial sum is an exact integer, so neither the order of the
columns nor the fusing of the multiply-add can change a distance: the device's radii and counts must EQUAL the restatement's.
On random fp32 rows the two may differ by rounding; the bound below is for D + 1 roundings of at most 2^-53 each (D
sums, and the product when it is not fused), doubled.
"""
import numpy as np

K_MAX = 16
MAX_ROWS = 1 << 20


# ------------------------------------------------------------------------------------------------ the rules, restated
def d2_ref(a, b):
    """(len(a), len(b)) float64: the squared distances of the rows of a to the rows of b; NaN -> +inf."""
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    out = np.zeros((a64.shape[0], b64.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(a64.shape[1]):
            t = a64[:, c, None] - b64[None, :, c]
            out += t * t
    out[np.isnan(out)] = np.inf
    return out


def radii_ref(f, k, d=None):
    d = d2_ref(f, f) if d is None else d.copy()
    np.fill_diagonal(d, np.inf)                      # self by index: a twin at another index stays, at distance 0
    return np.sort(d, axis=1)[:, k - 1]


def counts_ref(q, f, r2, d=None):
    """-> (inside (m,) int64, holds (n,) int64)"""
    d = d2_ref(q, f) if d is None else d
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d <= np.asarray(r2, np.float64)[None, :])
    return ok.sum(axis=1), ok.sum(axis=0)


def prdc_ref(real, gen, k):
    inside, holds = counts_ref(gen, real, radii_ref(real, k))
    inside_r, _ = counts_ref(real, gen, radii_ref(gen, k))
    n_real, n_gen = len(real), len(gen)
    return {"precision": int((inside > 0).sum()) / n_gen, "recall": int((inside_r > 0).sum()) / n_real,
            "density": int(inside.sum()) / (k * n_gen), "coverage": int((holds > 0).sum()) / n_real,
            "k": k, "n": [n_real, n_gen]}


def radius_bound(D):
    """relative, device radius against the restatement's"""
    return (D + 2) * 2.0 ** -52


def undecided_pairs(d, r2, D):
    """The pairs (j, i) whose side of the sphere rounding could change: |d2 - r2_i| <= (D + 2) 2^-51 r2_i."""
    with np.errstate(invalid="ignore"):
        return np.argwhere(np.abs(d - r2[None, :]) <= (D + 2) * 2.0 ** -51 * r2[None, :])


def neighbour_margin(f, k):
    """The smallest relative gap between a row's k-th neighbour distance and its (k - 1)-th and (k + 1)-th (where they
    exist): above the rounding bound, the device picks the same neighbour as the restatement."""
    d = d2_ref(f, f)
    np.fill_diagonal(d, np.inf)
    s = np.sort(d, axis=1)
    gaps = []
    if k >= 2:
        gaps.append(((s[:, k - 1] - s[:, k - 2]) / s[:, k - 1]).min())
    if k <= s.shape[1] - 2:                          # the last column is the +inf of the diagonal
        gaps.append(((s[:, k] - s[:, k - 1]) / s[:, k - 1]).min())
    return min(gaps)


# ------------------------------------------------------------------------------------------------ the split rule
def chunks_rule(rows, cols):
    """include/csg_hip.h, csg_manifold_column_chunks, restated."""
    blocks, tiles = -(-rows // 64), -(-cols // 64)
    return max(1, min(64, -(-tiles // 2), -(-8192 // blocks)))


def chunk_boundaries(chunks, limit=1024):
    """[n < limit : chunks(n, n) != chunks(n + 1, n + 1)] for the host entry (or the restated rule) `chunks`."""
    return [n for n in range(1, limit) if chunks(n, n) != chunks(n + 1, n + 1)]


def row_groups_rule(m):
    """include/csg_hip.h, csg_ball_counts: the query tiles are cut into min(64, ceil(m / 64)) row groups.  Up to m = 4096 a
    block owns ONE query tile; above it a block walks several in turn, accumulating `holds` across them in the workspace
    and closing `inside` once per tile."""
    return min(64, -(-m // 64))


# (m queries, n centres), each also run the other way round.  4096: the last m with one tile per group; 4161: 66 tiles in
# 64 groups, so two groups walk two tiles and the last tile is partial; 8259: 130 tiles, every group walks two or three.
ROW_GROUP_CASES = [(4096, 130), (4161, 130), (8259, 130)]


def row_group_case(m, n, D=64, seed=11):
    """-> (q (m,D), f (n,D), r2 (n,)): integer-grid rows and INTEGER radii around the typical distance (mean 4 D), so that
    counts are neither 0 nor everything and pairs lie exactly on spheres.  The radii are given, not k-NN radii: the
    restatement of n = 8259 rows against themselves would cost more than the case is worth, and csg_ball_counts takes any."""
    q, f = grid(m, D, seed), grid(n, D, seed + 1000)
    r2 = np.random.RandomState(seed + 2000).randint(4 * D - 40, 4 * D + 10, size=n).astype(np.float64)
    return q, f, r2


# ------------------------------------------------------------------------------------------------ the hand-worked row
# Points on a line: the first feature column is the coordinate, the others are 0.  D = 64, k = 1.
#   real 0, 1, 2, 4: nearest others at 1, 1, 1, 2        -> r2_real = [1, 1, 1, 4]
#   gen  0.5, 3, 7:  0.5 is within 1 of 0 and of 1 (d2 0.25 each), 1.5 from 2 (2.25 > 1), 3.5 from 4 (12.25 > 4): inside 2
#                    3 is at d2 = 1 from 2, ON its sphere (<=: inside), and at d2 = 1 from 4 (<= 4): inside 2
#                    7 is at d2 = 9 from 4 (> 4): inside 0                      -> inside_gen = [2, 2, 0]
#   holds_real: 0 holds 0.5; 1 holds 0.5; 2 holds 3; 4 holds 3                  -> [1, 1, 1, 1]
#   precision 2/3, density (2 + 2 + 0) / (1 * 3) = 4/3, coverage 4/4 = 1
#   gen radii: 0.5 -> 3 at 2.5 (6.25); 3 -> 0.5 (6.25); 7 -> 3 at 4 (16)        -> r2_gen = [6.25, 6.25, 16]
#   real in gen balls: 0 is 0.25 from 0.5: inside; likewise 1, 2 (2.25), 4 (1 from 3): all inside -> recall 1
HAND_K, HAND_D = 1, 64
HAND_REAL_X, HAND_GEN_X = [0.0, 1.0, 2.0, 4.0], [0.5, 3.0, 7.0]
HAND = {"r2_real": [1.0, 1.0, 1.0, 4.0], "inside_gen": [2, 2, 0], "holds_real": [1, 1, 1, 1],
        "r2_gen": [6.25, 6.25, 16.0], "inside_real": [1, 2, 2, 2],
        "precision": 2 / 3, "density": 4 / 3, "coverage": 1.0, "recall": 1.0}
# inside_real, worked: 0 -> in the ball of 0.5 only (9 > 6.25 from 3, 49 > 16 from 7): 1; 1 -> 0.5 (0.25) and 3 (4): 2;
# 2 -> 0.5 (2.25) and 3 (1): 2 (25 > 16 from 7); 4 -> 3 (1) and 7 (9 <= 16), 12.25 > 6.25 from 0.5: 2


def line_points(xs, D=HAND_D):
    f = np.zeros((len(xs), D), np.float32)
    f[:, 0] = xs
    return f


# ------------------------------------------------------------------------------------------------ integer-grid rows
def grid(n, D, seed):
    """(n, D) fp32 with entries from {-2, ..., 2}: every distance an exact integer, exact ties between pairs."""
    return np.random.RandomState(seed).randint(-2, 3, size=(n, D)).astype(np.float32)


def grid_case(n, m, D, k, seed=7, ties=False):
    """-> (real (n,D), gen (m,D), k).  ties=True plants the degenerate rows: four identical real rows (radius 0 for k <= 3)
    with a generated row equal to them, one real row duplicated once, and three generated rows copied from real ones."""
    real, gen = grid(n, D, seed), grid(m, D, seed + 1000)
    if ties:
        assert n >= 16 and m >= 4
        real[1:4] = real[0]                  # rows 0..3 identical
        gen[0] = real[0]
        real[6] = real[5]                    # a twin: each excludes itself and counts the other
        gen[1:4] = real[10:13]
    return real, gen, k


# (name, n real rows, m generated rows, D, k, ties planted)
GRID_CASES = [
    ("ties", 70, 65, 64, 3, True),
    ("ties_k1", 70, 65, 64, 1, True),
    ("minimum_n", 4, 5, 64, 3, False),            # n = k + 1
    ("two_rows", 2, 1, 64, 1, False),             # the smallest call there is; m = 1
    ("k16_minimum", 17, 3, 64, 16, False),        # k = 16 = n - 1
    ("k_n_minus_1", 10, 12, 64, 9, False),
    ("n63", 63, 64, 64, 3, False),
    ("n64", 64, 63, 64, 1, False),
    ("n65_k16_d128", 65, 65, 128, 16, True),
    ("n130", 130, 70, 64, 3, True),               # three tiles, two chunks
    ("one_query", 65, 1, 64, 3, False),           # m = 1
    ("uneven", 200, 37, 128, 5, True),            # n != m, D = 128
]

MASK_CASE = (70, 65, 64, 3)                       # n, m, D, k: no multiple of the tile, so a read past the end finds rows


def masked_operands(n, m, D, k):
    """-> (f_big, q_big, n, m): f = f_big[:n] and q = q_big[:m] are leading views; behind each view lie copies of the OTHER
    operand's rows, so a kernel that reads past n or m meets distance-0 neighbours and the integers change."""
    real, gen, _ = grid_case(n, m, D, k)
    return np.concatenate([real, gen]), np.concatenate([gen, real]), n, m


# ------------------------------------------------------------------------------------------------ random fp32 rows
# (n, m, D, k, seed of np.random.RandomState): standard normal real rows, then 0.9 normal + 0.15 generated rows
RANDOM_CASES = [(150, 130, 64, 5, 0), (257, 129, 128, 1, 2), (200, 200, 64, 16, 3)]
INTERIOR_CASE = RANDOM_CASES[1]                   # precision, recall and coverage strictly inside (0, 1)


def random_case(n, m, D, k, seed):
    rng = np.random.RandomState(seed)
    real = rng.standard_normal((n, D)).astype(np.float32)
    gen = (0.9 * rng.standard_normal((m, D)) + 0.15).astype(np.float32)
    return real, gen, k


# ------------------------------------------------------------------------------------------------ the non-finite row
NONFINITE_ROWS, NONFINITE_COLUMN = (7, 9), 3      # two rows with +inf in one column: inf - inf = NaN between them


def nonfinite_case():
    """-> (real with the +inf rows, the same rows without them, gen, k)"""
    real, gen, k = grid_case(70, 65, 64, 3)
    bad = real.copy()
    bad[list(NONFINITE_ROWS), NONFINITE_COLUMN] = np.inf
    return bad, np.delete(real, NONFINITE_ROWS, axis=0), gen, k
