"""DiffAugment of the discriminators' inputs (csrc/augment.hip, csrc/csg_augment.h): the case table, and a restatement in
numpy uint64 (the hash and the parameter rows) and float64 (the transform and its adjoint).  tests/test_augment_cases.py holds
the restatement to fixed vectors and to the host half of the shared header; tests/test_gpu_augment.py holds the device to it.

THE PARAMETER ROW.  key h = step(step(step(step(0, seed), iteration), pass), rank << 32 | n), draw k = step(h, k) for
k = 1..7 in the order r1, r2, r3, tx, ty, cy, cx; a float is (g >> 40) * 2^-24, an integer in [0, n) is ((g >> 32) * n) >> 32.
b = r1 - 0.5 and s = 2 r2 are exact in fp32; c = r3 + 0.5 is float32(u3 + 2^23) * 2^-24, ONE rounding (of a 25-bit
integer).  t = int(H / 8 + 0.5), size = int(H / 2 + 0.5), the centres are uniform in [0, H - 1 + (1 - size % 2)] and
y0 = centre - size // 2.  A row is eight 32-bit words: the bits of b, s, c, then tx, ty, y0, x0, size.

THE BOUND OF THE COLOUR MAP.  The device's fp32 operation sequence is stated in the header comment of csrc/augment.hip:
    forward   x1_k = x_k + b (3);  t = (x1_0 + x1_1) + x1_2 (2);  mp = t / 3 (1);  d_k = x1_k - mp (1);
              x2_k = fmaf(d_k, s, mp) (1);  mu = float32(S / (3 H H) + b) (1);  e_k = x2_k - mu (1);  x3_k = fmaf(e_k, c, mu) (1)
    backward  gbar = float32(S' / (3 H H)) (1);  omc = 1 - c (1);  q = omc * gbar (1);  g2_k = fmaf(c, g3_k, q) (3);
              t = (g2_0 + g2_1) + g2_2 (2);  mg = t / 3 (1);  oms = 1 - s (1);  r = oms * mg (1);  gx_k = fmaf(s, g2_k, r) (1)
so 11 roundings feed a forward value and 12 a backward one (the sums S, S' are fp64 trees: their error, 2^-53 relative per
addition, is far below one fp32 rounding and is covered by the rounding counted for mu / gbar).  Every rounding perturbs its
own result by at most 2^-24 of its magnitude, and that magnitude is at most L, the largest magnitude among ALL the
intermediates of the sample — the inputs, x1, t, mp, d, d * s, x2, mu, e, e * c, x3 (backward: g3, gbar, q, c * g3, g2, t,
mg, r, s * g2, gx) — evaluated in float64.  The bound is
    |device - float64 restatement| <= ROUNDINGS * 2^-24 * L         per sample,
computed from the inputs, never tuned.  (To first order a perturbation made before the multiplications by s <= 2 and
c <= 1.5 is scaled by them; the products d * s and e * c are among the intermediates L is taken over.)  Where the map is a
copy or a zero — every channel outside [c0, c0 + 3), and every channel with colour off — the device must give the
restatement's BITS.

THE LAUNCH RULE OF THE REDUCTION (csrc/augment.hip): a sample's H * H pixels are cut into chunks of CHUNK = 256 pixels, one
fp64 partial per chunk whatever the grid; the first launch has min(N * chunks, MAX_GRID = 2048) blocks that stride over the
chunks; the second launch gives lane l of one block per sample the chunks l, l + 256, ...  The code takes another path at
    chunks 1 -> 2              H = 16 | 17     (one partial; several, the last chunk partly filled)
    lane 0 takes a 2nd chunk   H = 256 | 257   (chunks 256 -> 259 > STAGE2 = 256)
    the grid is capped         N * chunks = 2048 | > 2048: (N, H) = (8, 256) | (9, 256)
`SPLIT_SHAPES` lists the smallest shapes on either side of each; between those points only the number of chunks changes.
"""
import numpy as np

MASK = (1 << 64) - 1
COLOR, TRANSLATION, CUTOUT = 1, 2, 4
POLICY_NAMES = {"color": COLOR, "translation": TRANSLATION, "cutout": CUTOUT}
CHUNK, STAGE2, MAX_GRID = 256, 256, 2048
FWD_ROUNDINGS, BWD_ROUNDINGS = 11, 12
U = 2.0 ** -24
SENTINEL = np.int32(0x7fc0dead)          # a NaN with a payload: no kernel output can equal it by accident


# ------------------------------------------------------------------------------------------------ the hash, Python ints
def fin_py(z):
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & MASK
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def step_py(h, w):
    return fin_py(((h ^ w) + 0x9e3779b97f4a7c15) & MASK)


def key_py(seed, iteration, pass_id, rank, n):
    h = step_py(0, seed)
    h = step_py(h, iteration)
    h = step_py(h, pass_id)
    return step_py(h, (rank << 32) | n)


def extents(H):
    """(t, size, centres): the largest shift, the cutout's side and the number of values a centre takes."""
    size = int(H * 0.5 + 0.5)
    return int(H * 0.125 + 0.5), size, H + (1 - size % 2)


def row_py(seed, iteration, pass_id, rank, n, H):
    """The eight words of one row as Python ints (b, s, c as fp32 bit patterns; the integers as signed values)."""
    h = key_py(seed, iteration, pass_id, rank, n)
    g = [step_py(h, k) for k in range(1, 8)]
    t, size, centres = extents(H)
    u1, u2, u3 = (x >> 40 for x in g[:3])
    b = np.float32(u1 - (1 << 23)) * np.float32(2.0 ** -24)
    s = np.float32(u2) * np.float32(2.0 ** -23)
    c = np.float32(u3 + (1 << 23)) * np.float32(2.0 ** -24)
    ints = [(((g[3] >> 32) * (2 * t + 1)) >> 32) - t, (((g[4] >> 32) * (2 * t + 1)) >> 32) - t,
            (((g[5] >> 32) * centres) >> 32) - size // 2, (((g[6] >> 32) * centres) >> 32) - size // 2, size]
    return [int(np.float32(v).view(np.int32)) for v in (b, s, c)] + ints


# (seed, iteration, pass, rank, n) -> (key, first draw): worked out once with the functions above
HASH_VECTORS = [
    ((0, 0, 0, 0, 0), (0x2130748aaac80268, 0xa5d3758b95b92366)),
    ((0, 1, 0, 0, 0), (0xd1c0270687984b37, 0x00c3dedf8d7bb611)),
    ((1, 0, 0, 0, 0), (0xe28195ddd9ee4956, 0x12087fdb175ec8f9)),
    ((0, 0, 5, 0, 3), (0x0c1952e38a47c7a3, 0xc1496918dfa225bd)),
    ((7, 123456789, 2, 1, 15), (0xe1526d067235928b, 0x284d103f9bec1616)),
    (((1 << 64) - 1, (1 << 63) - 1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1), (0x80d36266f0e25f73, 0xc0c5c58ab00b3994)),
]
# rows 0..2 of the table of (seed, iteration, pass, rank, H) = ROW_VECTORS_KEY: words as int32
ROW_VECTORS_KEY = ((1 << 64) - 1, 5, 4, 3, 16)
ROW_VECTORS = [[1049394762, 1071322312, 1068430617, 1, 2, -4, 6, 8], [-1110645984, 1060446218, 1059473748, 2, -1, 8, -3, 8],
               [1056435962, 1058115514, 1057246367, -2, 0, 3, -3, 8]]


# ------------------------------------------------------------------------------------------------ the hash, numpy uint64
def _fin_np(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xbf58476d1ce4e5b9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def step_np(h, w):
    with np.errstate(over="ignore"):
        return _fin_np((np.asarray(h, np.uint64) ^ np.asarray(w, np.uint64)) + np.uint64(0x9e3779b97f4a7c15))


def table_np(seed, iteration, pass_id, rank, rows, H):
    """(rows, 8) int32: the table the device entry fills."""
    n = np.arange(rows, dtype=np.uint64)
    h = step_np(step_np(step_np(step_np(np.uint64(0), np.uint64(seed)), np.uint64(iteration)), np.uint64(pass_id)),
                (np.uint64(rank) << np.uint64(32)) | n)
    g = [step_np(h, np.uint64(k)) for k in range(1, 8)]
    t, size, centres = extents(H)
    u = [(x >> np.uint64(40)).astype(np.int64) for x in g[:3]]
    out = np.zeros((rows, 8), np.int32)
    out[:, 0] = ((u[0] - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -24)).view(np.int32)
    out[:, 1] = (u[1].astype(np.float32) * np.float32(2.0 ** -23)).view(np.int32)
    out[:, 2] = ((u[2] + (1 << 23)).astype(np.float32) * np.float32(2.0 ** -24)).view(np.int32)

    def integer(x, m):
        return (((x >> np.uint64(32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
    out[:, 3] = integer(g[3], 2 * t + 1) - t
    out[:, 4] = integer(g[4], 2 * t + 1) - t
    out[:, 5] = integer(g[5], centres) - size // 2
    out[:, 6] = integer(g[6], centres) - size // 2
    out[:, 7] = size
    return out


# ------------------------------------------------------------------------------------------------ rows written by hand
def make_row(b, s, c, tx, ty, y0, x0, size):
    row = np.zeros(8, np.int32)
    row[:3] = np.asarray([b, s, c], np.float32).view(np.int32)
    row[3:] = [tx, ty, y0, x0, size]
    return row


def row_params(row):
    b, s, c = (float(v) for v in np.asarray(row[:3], np.int32).view(np.float32))
    return (b, s, c) + tuple(int(v) for v in row[3:])


def policy_mask(names):
    return sum(POLICY_NAMES[n] for n in names)


ALL_POLICIES = [m for m in range(1, 8)]                       # the 7 non-empty sets


# ------------------------------------------------------------------------------------------------ the transform, float64
def _cut_box(H, y0, x0, size):
    return max(y0, 0), min(y0 + size, H), max(x0, 0), min(x0 + size, H)


def _shift(a, ty, tx):
    """out[y, x] = a[y - ty, x - tx], zero outside (a: (H, H, C))."""
    H = a.shape[0]
    out = np.zeros_like(a)
    ys0, ys1, xs0, xs1 = max(0, -ty), min(H, H - ty), max(0, -tx), min(H, H - tx)       # the source window
    if ys1 > ys0 and xs1 > xs0:
        out[ys0 + ty:ys1 + ty, xs0 + tx:xs1 + tx] = a[ys0:ys1, xs0:xs1]
    return out


def restate_fwd(x, table, c0, policy):
    """x (N, H, H, Ct) float32 -> (float64 result, exact (bool, same shape): the device must give float32(result)'s bits there,
    L (N,): the largest intermediate magnitude of each sample's colour map, 0 with colour off)."""
    N, H, _, Ct = x.shape
    out = np.zeros(x.shape, np.float64)
    exact = np.ones(x.shape, bool)
    L = np.zeros(N)
    for n in range(N):
        b, s, c, tx, ty, y0, x0, size = row_params(table[n])
        a = x[n].astype(np.float64)
        if policy & COLOR:
            col = a[..., c0:c0 + 3]
            x1 = col + b
            t1 = x1[..., 0] + x1[..., 1]
            t2 = t1 + x1[..., 2]
            mp = (t2 / 3.0)[..., None]
            d = x1 - mp
            x2 = d * s + mp
            mu = col.sum() / (3.0 * H * H) + b
            e = x2 - mu
            x3 = e * c + mu
            L[n] = max(np.abs(v).max() for v in (col, x1, t1, t2, mp, d, d * s, x2, e, e * c, x3, np.float64(mu)))
            a = a.copy()
            a[..., c0:c0 + 3] = x3
        if policy & TRANSLATION:
            a = _shift(a, ty, tx)
        live = np.ones((H, H), bool)
        if policy & TRANSLATION:
            live = _shift(np.ones((H, H, 1)), ty, tx)[..., 0] > 0
        if policy & CUTOUT:
            r0, r1, q0, q1 = _cut_box(H, y0, x0, size)
            if r1 > r0 and q1 > q0:
                a = a.copy()
                a[r0:r1, q0:q1] = 0.0
                live[r0:r1, q0:q1] = False
        out[n] = a
        if policy & COLOR:
            exact[n, :, :, c0:c0 + 3] = ~live[..., None]          # a zero fill is exact; a colour value is not
    return out, exact, L


def restate_bwd(g, table, c0, policy):
    """The adjoint: g (N, H, H, Ct) float32 at the transform's output -> (float64 gradient at its input, exact, L)."""
    N, H, _, Ct = g.shape
    out = np.zeros(g.shape, np.float64)
    exact = np.ones(g.shape, bool)
    L = np.zeros(N)
    for n in range(N):
        b, s, c, tx, ty, y0, x0, size = row_params(table[n])
        a = g[n].astype(np.float64).copy()
        if policy & CUTOUT:
            r0, r1, q0, q1 = _cut_box(H, y0, x0, size)
            if r1 > r0 and q1 > q0:
                a[r0:r1, q0:q1] = 0.0
        if policy & TRANSLATION:
            a = _shift(a, -ty, -tx)
        if policy & COLOR:
            g3 = a[..., c0:c0 + 3]
            gbar = g3.sum() / (3.0 * H * H)
            q = (1.0 - c) * gbar
            g2 = c * g3 + q
            t1 = g2[..., 0] + g2[..., 1]
            t2 = t1 + g2[..., 2]
            mg = (t2 / 3.0)[..., None]
            r = (1.0 - s) * mg
            gx = s * g2 + r
            L[n] = max(np.abs(v).max() for v in (g3, c * g3, g2, t1, t2, mg, r, s * g2, gx, np.float64(gbar), np.float64(q)))
            a[..., c0:c0 + 3] = gx
            exact[n, :, :, c0:c0 + 3] = False
        out[n] = a
    return out, exact, L


def check_against(got, ref, exact, L, roundings, what):
    """got (float32) against the restatement: bits where `exact`, the derived bound elsewhere.  Returns the worst
    |got - ref| / bound over the inexact elements (0 if there are none); asserts nothing about it."""
    want = ref.astype(np.float32)
    same = got.view(np.int32) == want.view(np.int32)
    bad = exact & ~same
    assert not bad.any(), "%s: %d elements that must be copies or zeros differ in their bits, first at %s" % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    worst = 0.0
    for n in range(got.shape[0]):
        m = ~exact[n]
        if m.any():
            assert L[n] > 0 and np.isfinite(L[n]), (what, n, L[n])
            err = np.abs(got[n][m].astype(np.float64) - ref[n][m]).max()
            worst = max(worst, float(err / (roundings * U * L[n])))
    return worst


# ------------------------------------------------------------------------------------------------ the case table
SHAPES = [(1, 2, 4, 0), (3, 4, 4, 0), (2, 8, 8, 4), (2, 8, 8, 5), (3, 16, 12, 8), (2, 32, 40, 32)]       # (N, H, Ct, c0)
SPLIT_SHAPES = [(2, 16, 4, 0), (2, 17, 4, 0), (1, 256, 4, 0), (1, 257, 4, 1), (8, 256, 4, 0), (9, 256, 4, 0)]


def chunks_of(H):
    return (H * H + CHUNK - 1) // CHUNK


def launch_rule(N, H):
    """(chunks per sample, blocks of the first launch, chunks lane 0 of the second launch takes)."""
    ch = chunks_of(H)
    return ch, min(N * ch, MAX_GRID), (ch + STAGE2 - 1) // STAGE2


def workspace_bytes(N, H):
    return (N * chunks_of(H) * 8 + N * 4 + 15) // 16 * 16


def boundary_rows(H):
    """Rows that hit every boundary on purpose: tx, ty in {-t, 0, t} in all combinations, each with a cutout centre out of
    {0, H - 1 + (1 - size % 2), the middle} in turn (all 9 centre pairs occur), and colour parameters that walk through
    s = 0, c = 0.5, b = -0.5 and ordinary values."""
    t, size, centres = extents(H)
    cs = [0, centres - 1, centres // 2]
    colour = [(-0.5, 0.0, 0.5), (0.25, 2.0 - 2.0 ** -23, 1.5), (0.0, 1.0, 1.0), (-0.5, 0.75, 1.25), (0.4375, 0.0, 0.5)]
    rows, k = [], 0
    for ty in (-t, 0, t):
        for tx in (-t, 0, t):
            cy, cx = cs[k % 3], cs[(k // 3) % 3]
            b, s, c = colour[k % len(colour)]
            rows.append(make_row(b, s, c, tx, ty, cy - size // 2, cx - size // 2, size))
            k += 1
    return np.stack(rows)


def data(shape, seed):
    """(N, H, H, Ct) float32 in about [-1, 1] with a few exact zeros, negative zeros and large values."""
    N, H, Ct, _ = shape
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(N, H, H, Ct)).astype(np.float32)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=max(3, flat.size // 50), replace=False)
    flat[idx[0::3]] = 0.0
    flat[idx[1::3]] = -0.0
    flat[idx[2::3]] *= 64.0
    return x
