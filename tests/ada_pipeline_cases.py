"""The ADA augmentation pipeline (csrc/csg_ada_pipeline.h, csrc/ada_pipeline.hip): the case table, and a restatement in numpy
uint64 / float64 (the draws, the polynomials, the composition: the parameter row, bit for bit) and numpy float32 (the
coordinates, taps and weights of the resampler, bit for bit) and float64 (the sums the device's values are held to).
tests/test_ada_pipeline_cases.py holds the host half of the shared header to the restatement; tests/test_gpu_ada_pipeline.py
holds the device to both.

THE ROW (32 words): M 0..5, G 6..11, margin 12, flags 13, ex ey 14 15, C 16..27, a b c d 28..31; the draws start at 16 and
are listed in the header.  Every fp64 operation of the header is one numpy float64 operation here, in the header's order
(numpy never fuses a multiplication into an addition); a transform that is off is skipped with np.where.

THE BOUNDS, from the operation sequences stated at the top of csrc/ada_pipeline.hip, u = 2^-24:
    interpolation   v = ((w00 a00 + w01 a01) + w10 a10) + w11 a11: 4 products and 3 additions = INTERP_ROUNDINGS = 7, each
                    of a magnitude <= max|x| * sum(w), and the four fp32 weights sum to at most 1 + 3 u (1 - fx is one
                    rounding, a product one more):      |device - fp64 sum over the device's weights| <= 7 u max|x| (1 + 2^-20)
    colour          r' = ((c00 r + c01 g) + c02 b) + c03: 3 products and 3 additions = COLOR_ROUNDINGS = 6, each of a
                    magnitude <= L, the largest intermediate of the sample in fp64:      <= 6 u L
    colour adjoint  t_j = (c0j g0 + c1j g1) + c2j g2: COLOR_ADJOINT_ROUNDINGS = 5:        <= 5 u L
    adjoint         acc = acc + w t over the `terms` output pixels that hold q among their taps: one product and one
                    addition per term, each of a magnitude <= S = sum |w t| (1 + terms u):
                                                                     <= (terms + TERM_ROUNDINGS = 1) u S (1 + 2^-20)
Where the map is a copy or a zero the device must give the restatement's BITS; the weights themselves are held as bits by
one-hot inputs (1 * w and w + 0 are exact).
"""
import numpy as np

import augment_cases as ac

BLIT, GEOM, COLOR = 8, 16, 32
POLICIES = [BLIT, GEOM, COLOR, BLIT | GEOM, BLIT | COLOR, GEOM | COLOR, BLIT | GEOM | COLOR]
ROW_WORDS, MAX_BOX, MAX_MARGIN = 32, 16, 4
GEOM_ID, GEOM_INT, COLOR_ID = 1, 2, 4
ONE = 1 << 24
P24_VALUES = [0, 1, 1 << 23, ONE - 1, ONE]
TABLE_H = [2, 5, 8, 16, 256]
KEYS = [(0, 1, 0, 0), (7, 123456789, 2, 1), ((1 << 64) - 1, (1 << 63) - 1, 5, (1 << 31) - 1)]      # (seed, iteration, pass, rank)
INTERP_ROUNDINGS, COLOR_ROUNDINGS, COLOR_ADJOINT_ROUNDINGS, TERM_ROUNDINGS = 7, 6, 5, 1
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
F32 = np.float32

_EXP_COEFFS = [1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0,
               1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0]
_SIN_COEFFS = [1.0 / 1307674368000.0, -1.0 / 6227020800.0, 1.0 / 39916800.0, -1.0 / 362880.0, 1.0 / 5040.0, -1.0 / 120.0, 1.0 / 6.0]
_COS_COEFFS = [1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0,
               1.0 / 24.0, -0.5]
TURN = 6.283185307179586476925 * 2.0 ** -24
THIRD = 1.0 / 3.0
INV_SQRT3 = 0.57735026918962576451


# ------------------------------------------------------------------------------------------------ the maths, float64
def exp2_np(e):
    e = np.asarray(e, np.float64)
    nf = np.floor(e + 0.5)
    f = e - nf
    t = f * 0.6931471805599453094
    p = np.full(e.shape, 1.0 / 87178291200.0)
    for c in _EXP_COEFFS:
        p = p * t + c
    return p * np.ldexp(1.0, nf.astype(np.int64))


def sincos_np(u):
    """(sin, cos) of u * 2^-24 turns, u an integer array in [0, 2^24)."""
    u = np.asarray(u, np.int64)
    h = ((u >> 21) + 1) >> 1
    phi = (u - (h << 22)).astype(np.float64) * TURN
    x = phi * phi
    ps = np.full(x.shape, -1.0 / 355687428096000.0)
    for c in _SIN_COEFFS:
        ps = ps * x + c
    ps = ps * x
    sp = phi - phi * ps
    pc = np.full(x.shape, -1.0 / 6402373705728000.0)
    for c in _COS_COEFFS:
        pc = pc * x + c
    cp = pc * x + 1.0
    q = h & 3
    s = np.where(q == 0, sp, np.where(q == 1, cp, np.where(q == 2, -sp, -cp)))
    c = np.where(q == 0, cp, np.where(q == 1, -sp, np.where(q == 2, -cp, sp)))
    return s, c


def prot24_of(p24):
    a = 1.0 - np.float64(p24) * 2.0 ** -24
    return int(np.floor((1.0 - np.sqrt(a)) * 16777216.0))


# ------------------------------------------------------------------------------------------------ the draws
def key_np(seed, iteration, pass_id, rank, rows):
    n = np.arange(rows, dtype=np.uint64)
    return ac.step_np(ac.step_np(ac.step_np(ac.step_np(np.uint64(0), np.uint64(seed)), np.uint64(iteration)), np.uint64(pass_id)),
                      (np.uint64(rank) << np.uint64(32)) | n)


def draw(h, k):
    return ac.step_np(h, np.uint64(k))


def u24(g):
    return (g >> np.uint64(40)).astype(np.int64)


def normal_np(h, first):
    s = np.zeros(h.shape, np.int64)
    for k in range(12):
        s = s + u24(draw(h, first + k))
    return (s - 6 * ONE).astype(np.float64) * 2.0 ** -24


def integer(g, m):
    return (((g >> np.uint64(32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def blit_draws(h, H, p24):
    """What the blit stage does to each sample: (flip, k, tx, ty, any), the values already 0 where the transform is off."""
    t = (H + 4) >> 3
    on_f, on_r, on_t = (u24(draw(h, k)) < p24 for k in (16, 18, 20))
    flip = on_f & ((draw(h, 17) >> np.uint64(63)) == 1)
    k = np.where(on_r, (draw(h, 19) >> np.uint64(62)).astype(np.int64), 0)
    tx = np.where(on_t, integer(draw(h, 21), 2 * t + 1) - t, 0)
    ty = np.where(on_t, integer(draw(h, 22), 2 * t + 1) - t, 0)
    return flip, k, tx, ty, on_f | on_r | on_t


# ------------------------------------------------------------------------------------------------ the composition
def _aff(l00, l01, t0, l10, l11, t1, like):
    return [np.broadcast_to(np.asarray(v, np.float64), like.shape).copy() for v in (l00, l01, t0, l10, l11, t1)]


def _aff_mul(A, B):
    a00, a01, at0, a10, a11, at1 = A
    b00, b01, bt0, b10, b11, bt1 = B
    return [a00 * b00 + a01 * b10, a00 * b01 + a01 * b11, (a00 * bt0 + a01 * bt1) + at0,
            a10 * b00 + a11 * b10, a10 * b01 + a11 * b11, (a10 * bt0 + a11 * bt1) + at1]


def _where(on, new, old):
    return [np.where(on, n, o) for n, o in zip(new, old)]


def _col(diag, off, t, like):
    z = np.zeros(like.shape)
    l = [[(z + diag) if i == j else (z + off) for j in range(3)] for i in range(3)]
    return l, [z + t for _ in range(3)]


def _col_mul(A, C):
    (al, at), (cl, ct) = A, C
    l = [[(al[i][0] * cl[0][j] + al[i][1] * cl[1][j]) + al[i][2] * cl[2][j] for j in range(3)] for i in range(3)]
    t = [((al[i][0] * ct[0] + al[i][1] * ct[1]) + al[i][2] * ct[2]) + at[i] for i in range(3)]
    return l, t


def _col_where(on, new, old):
    return ([[np.where(on, new[0][i][j], old[0][i][j]) for j in range(3)] for i in range(3)],
            [np.where(on, new[1][i], old[1][i]) for i in range(3)])


def table_np(seed, iteration, pass_id, rank, rows, H, policy, p24):
    """(rows, 32) int32: the table the entries fill."""
    h = key_np(seed, iteration, pass_id, rank, rows)
    like = np.zeros(rows)
    prot24 = prot24_of(p24)
    blit, geom, colour = bool(policy & BLIT), bool(policy & GEOM), bool(policy & COLOR)
    off = np.zeros(rows, bool)

    def gate(k, thr, group):
        return (u24(draw(h, k)) < thr) if group else off
    M = _aff(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, like)
    G = _aff(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, like)

    def compose(on, inv, fwd):
        nonlocal M, G
        M = _where(on, _aff_mul(M, inv), M)
        G = _where(on, _aff_mul(fwd, G), G)
    # ---- pixel blitting
    g16, g18, g20 = gate(16, p24, blit), gate(18, p24, blit), gate(20, p24, blit)
    any_blit = g16 | g18 | g20
    F = _aff(-1.0, 0.0, 0.0, 0.0, 1.0, 0.0, like)
    compose(g16 & ((draw(h, 17) >> np.uint64(63)) == 1), F, F)
    k = (draw(h, 19) >> np.uint64(62)).astype(np.int64)
    ck = np.where(k == 2, -1.0, 0.0)
    sk = np.where(k == 1, 1.0, np.where(k == 3, -1.0, 0.0))
    compose(g18 & (k != 0), _aff(ck, -sk, 0.0, sk, ck, 0.0, like), _aff(ck, sk, 0.0, -sk, ck, 0.0, like))
    t = (H + 4) >> 3
    tx = (integer(draw(h, 21), 2 * t + 1) - t).astype(np.float64)
    ty = (integer(draw(h, 22), 2 * t + 1) - t).astype(np.float64)
    compose(g20, _aff(1.0, 0.0, -tx, 0.0, 1.0, -ty, like), _aff(1.0, 0.0, tx, 0.0, 1.0, ty, like))
    c = (H - 1) * 0.5
    ia, ib, ic, id_ = (M[i].astype(np.int32) for i in (0, 1, 3, 4))
    ex = ((c - (M[0] * c + M[1] * c)) + M[2]).astype(np.int32)
    ey = ((c - (M[3] * c + M[4] * c)) + M[5]).astype(np.int32)
    # ---- general geometry
    g23, g36, g38, g51, g53 = gate(23, p24, geom), gate(36, prot24, geom), gate(38, p24, geom), gate(51, prot24, geom), \
        gate(53, p24, geom)
    any_geom = g23 | g36 | g38 | g51 | g53
    e = np.clip(0.2 * normal_np(h, 24), -1.0, 1.0)
    s, si = exp2_np(e), exp2_np(-e)
    compose(g23, _aff(si, 0.0, 0.0, 0.0, si, 0.0, like), _aff(s, 0.0, 0.0, 0.0, s, 0.0, like))
    sn, cs = sincos_np(u24(draw(h, 37)))
    compose(g36, _aff(cs, sn, 0.0, -sn, cs, 0.0, like), _aff(cs, -sn, 0.0, sn, cs, 0.0, like))
    e = np.clip(0.2 * normal_np(h, 39), -1.0, 1.0)
    s, si = exp2_np(e), exp2_np(-e)
    compose(g38, _aff(si, 0.0, 0.0, 0.0, s, 0.0, like), _aff(s, 0.0, 0.0, 0.0, si, 0.0, like))
    sn, cs = sincos_np(u24(draw(h, 52)))
    compose(g51, _aff(cs, sn, 0.0, -sn, cs, 0.0, like), _aff(cs, -sn, 0.0, sn, cs, 0.0, like))
    a = 0.125 * float(H)
    tx, ty = a * normal_np(h, 54), a * normal_np(h, 66)
    compose(g53, _aff(1.0, 0.0, -tx, 0.0, 1.0, -ty, like), _aff(1.0, 0.0, tx, 0.0, 1.0, ty, like))
    # ---- colour
    g78, g91, g104, g106, g108 = (gate(k_, p24, colour) for k_ in (78, 91, 104, 106, 108))
    any_colour = g78 | g91 | g104 | g106 | g108
    C = _col(1.0, 0.0, 0.0, like)
    C = _col_where(g78, _col_mul(_col(1.0, 0.0, 0.2 * normal_np(h, 79), like), C), C)
    C = _col_where(g91, _col_mul(_col(exp2_np(0.5 * normal_np(h, 92)), 0.0, 0.0, like), C), C)
    lo = -2.0 * THIRD
    C = _col_where(g104 & ((draw(h, 105) >> np.uint64(63)) == 1), _col_mul(_col(1.0 + lo, lo, 0.0, like), C), C)
    sn, cs = sincos_np(u24(draw(h, 107)))
    a_, b_ = (1.0 - cs) * THIRD, sn * INV_SQRT3
    R = _col(cs + a_, 0.0, 0.0, like)
    R[0][0][1], R[0][0][2], R[0][1][0], R[0][1][2], R[0][2][0], R[0][2][1] = a_ - b_, a_ + b_, a_ + b_, a_ - b_, a_ - b_, a_ + b_
    C = _col_where(g106, _col_mul(R, C), C)
    s = exp2_np(normal_np(h, 109))
    so = THIRD - THIRD * s
    C = _col_where(g108, _col_mul(_col(so + s, so, 0.0, like), C), C)
    # ---- the words
    out = np.zeros((rows, ROW_WORDS), np.int32)

    def f32(v):
        return v.astype(np.float32).view(np.int32)
    for base, A in ((0, M), (6, G)):
        out[:, base + 0], out[:, base + 1], out[:, base + 2] = f32(A[0]), f32(A[1]), f32(A[2] + c)
        out[:, base + 3], out[:, base + 4], out[:, base + 5] = f32(A[3]), f32(A[4]), f32(A[5] + c)
    out[:, 12] = 1
    out[:, 13] = np.where(any_geom, 0, GEOM_INT) | np.where(any_geom | any_blit, 0, GEOM_ID) | np.where(any_colour, 0, COLOR_ID)
    out[:, 14], out[:, 15] = ex, ey
    for i in range(3):
        for j in range(3):
            out[:, 16 + 4 * i + j] = f32(C[0][i][j])
        out[:, 16 + 4 * i + 3] = f32(C[1][i])
    out[:, 28], out[:, 29], out[:, 30], out[:, 31] = ia, ib, ic, id_
    return out


# ------------------------------------------------------------------------------------------------ rows written by hand
def make_row(H, lin=(1.0, 0.0, 0.0, 1.0), shift=(0.0, 0.0), flags=0, margin=1, colour=None, intmap=None, G=None):
    """A row from M's linear part and translation in centred coordinates (sx' = l00 x' + l01 y' + tx): G is its fp64 inverse
    unless given (as (l00, l01, tx, l10, l11, ty), centred).  colour: 12 floats, default the identity; intmap: (a, b, c, d, ex, ey)."""
    c = (H - 1) * 0.5
    l00, l01, l10, l11 = (float(v) for v in lin)
    tx, ty = float(shift[0]), float(shift[1])
    if G is None:
        with np.errstate(all="ignore"):
            det = np.float64(l00) * l11 - np.float64(l01) * l10
            g00, g01, g10, g11 = l11 / det, -l01 / det + 0.0, -l10 / det + 0.0, l00 / det          # (+ 0.0: no -0.0 words)
            G = (g00, g01, -(g00 * tx + g01 * ty), g10, g11, -(g10 * tx + g11 * ty))
    row = np.zeros(ROW_WORDS, np.int32)
    with np.errstate(all="ignore"):
        row[0:6] = np.asarray([l00, l01, tx + c, l10, l11, ty + c], np.float64).astype(np.float32).view(np.int32)
        row[6:12] = np.asarray([G[0], G[1], G[2] + c, G[3], G[4], G[5] + c], np.float64).astype(np.float32).view(np.int32)
    row[12], row[13] = margin, flags
    col = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] if colour is None else colour
    row[16:28] = np.asarray(col, np.float32).view(np.int32)
    a, b, c_, d, ex, ey = (1, 0, 0, 1, 0, 0) if intmap is None else intmap
    row[14], row[15], row[28:32] = ex, ey, [a, b, c_, d]
    return row


def blit_map(flip, k, tx, ty, H):
    """(a, b, c, d, ex, ey) of out = shift(rot90(flip_x(in), k), ty, tx): the header's composition in Python integers."""
    P, t = [[1, 0], [0, 1]], [0, 0]                  # the inverse map in centred coordinates, doubled translation avoided: integers

    def mul(A, B):
        return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] for j in range(2)] for i in range(2)]
    if flip:
        P = mul(P, [[-1, 0], [0, 1]])
    ck, sk = [(1, 0), (0, 1), (-1, 0), (0, -1)][k % 4]
    P = mul(P, [[ck, -sk], [sk, ck]])
    t = [-(P[0][0] * tx + P[0][1] * ty), -(P[1][0] * tx + P[1][1] * ty)]
    # sx = a (x - c) + b (y - c) + t + c,  2 c = H - 1
    ex2 = (H - 1) * (1 - P[0][0] - P[0][1]) + 2 * t[0]
    ey2 = (H - 1) * (1 - P[1][0] - P[1][1]) + 2 * t[1]
    assert ex2 % 2 == 0 and ey2 % 2 == 0
    return P[0][0], P[0][1], P[1][0], P[1][1], ex2 // 2, ey2 // 2


def blit_np(x, flip, k, tx, ty):
    """numpy's own flip, rot90 and a zero-filled shift of x (H, H, C)."""
    a = np.flip(x, axis=1) if flip else x
    return ac._shift(np.rot90(a, k, axes=(0, 1)), ty, tx)


def blit_adjoint_np(g, flip, k, tx, ty):
    a = np.rot90(ac._shift(g, -ty, -tx), -k, axes=(0, 1))
    return np.flip(a, axis=1) if flip else a


SIGNED_PERMUTATIONS = [(f, k) for f in (0, 1) for k in range(4)]


def blit_shifts(H):
    t = (H + 4) >> 3
    return [(0, 0), (1, 0), (0, -1), (t, -t), (-t, t), (H, 0), (0, -H), (H + 3, -H - 2)]


def _general(H, *args, **kwargs):
    return make_row(H, *args, flags=COLOR_ID, **kwargs)


def hand_rows(H):
    """{name: row}: the general path (neither geometry flag set; the colour flag is) on maps it can go wrong at."""
    r = np.sqrt(0.5)
    big = float(np.finfo(np.float32).max)
    rows = {
        "rot45": _general(H, (r, r, -r, r)),
        "mag4": _general(H, (0.25, 0.0, 0.0, 0.25), (0.3, -0.2)),
        "mag_quarter": _general(H, (4.0, 0.0, 0.0, 4.0), (0.5, 0.25)),
        "aniso_4_quarter": _general(H, (0.25, 0.0, 0.0, 4.0)),
        "rot45_mag4": _general(H, (0.25 * r, 0.25 * r, -0.25 * r, 0.25 * r), (0.1, 0.7)),
        "half_pixel": _general(H, shift=(0.5, 0.5)),
        "out_right": _general(H, shift=(H + 3.0, 0.0)),
        "out_up": _general(H, shift=(0.0, -H - 3.0)),
        "on_integers": _general(H),                                    # sx = x exactly: fx = 0, and x0 + 1 = H at the edge
        "on_integers_shifted": _general(H, shift=(1.0, -1.0)),
        "nan_entry": _general(H, (np.nan, 0.0, 0.0, 1.0), G=(np.nan, 0.0, 0.0, 0.0, 1.0, 0.0)),
        "inf_shift": _general(H, shift=(np.inf, 0.0), G=(1.0, 0.0, -np.inf, 0.0, 1.0, 0.0)),
        "huge_shift": _general(H, shift=(1e30, 1e30), G=(1.0, 0.0, -1e30, 0.0, 1.0, -1e30)),
        "huge_entry": _general(H, (big, 0.0, 0.0, big), (3e38, 3e38), G=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)),
    }
    return rows


def foreign_rows(H):
    """Rows whose G is not M's inverse: the adjoint walks what the kernel's header states — an empty box here — and no more."""
    big = float(np.finfo(np.float32).max)
    return {"huge_forward_map": make_row(H, G=(big, big, 0.0, big, big, 0.0)),
            "nan_forward_map": make_row(H, G=(np.nan, 0.0, 0.0, 0.0, 1.0, 0.0))}


ZERO_ROWS = ("out_right", "out_up", "nan_entry", "inf_shift", "huge_shift", "huge_entry")


# ------------------------------------------------------------------------------------------------ the resampler, float32
def taps_np(row, H):
    """The forward's coordinates by its stated fp32 sequence: (sx, sy, x0, y0, w, live) with w (4, H, H) float32 and
    live (4, H, H) bool for the taps 00, 01, 10, 11 = (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)."""
    m = np.asarray(row[0:6], np.int32).view(np.float32)
    c = F32((H - 1) * 0.5)
    xc = (np.arange(H, dtype=np.float32) - c)[None, :]
    yc = (np.arange(H, dtype=np.float32) - c)[:, None]
    with np.errstate(all="ignore"):
        sx = ((m[0] * xc + m[1] * yc) + m[2]).astype(np.float32)
        sy = ((m[3] * xc + m[4] * yc) + m[5]).astype(np.float32)
        ok = (np.abs(sx) < F32(8388608.0)) & (np.abs(sy) < F32(8388608.0))
        sxs, sys_ = np.where(ok, sx, F32(0)), np.where(ok, sy, F32(0))
        fx0, fy0 = np.floor(sxs), np.floor(sys_)
        wx1, wy1 = sxs - fx0, sys_ - fy0
        wx0, wy0 = F32(1) - wx1, F32(1) - wy1
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    w = np.stack([wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1]).astype(np.float32)
    inx0, inx1 = (x0 >= 0) & (x0 < H), (x0 + 1 >= 0) & (x0 + 1 < H)
    iny0, iny1 = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    live = np.stack([iny0 & inx0, iny0 & inx1, iny1 & inx0, iny1 & inx1]) & ok[None]
    return sx, sy, x0, y0, w, live


def weight_matrix(row, H):
    """W (H H outputs, H H sources) float32 and the matching bool `tap`: W[p, q] is the forward's fp32 weight of source q in
    output p (0 where q is no live tap of p).  No source is two taps of one output, so an entry is one weight."""
    _, _, x0, y0, w, live = taps_np(row, H)
    W = np.zeros((H * H, H * H), np.float32)
    tap = np.zeros((H * H, H * H), bool)
    p = np.arange(H * H).reshape(H, H)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        m = live[k]
        q = (y0 + dy) * H + (x0 + dx)
        W[p[m], q[m]] = w[k][m]
        tap[p[m], q[m]] = True
    return W, tap


def colour_of(row):
    return np.asarray(row[16:28], np.int32).view(np.float32).astype(np.float64).reshape(3, 4)


def colour_fwd(v, row):
    """(r, g, b) float64 (..., 3) -> (the matrix's result by the stated order, the largest intermediate magnitude)."""
    C = colour_of(row)
    out = np.zeros(v.shape)
    L = np.abs(v).max() if v.size else 0.0
    for i in range(3):
        p0, p1, p2 = C[i, 0] * v[..., 0], C[i, 1] * v[..., 1], C[i, 2] * v[..., 2]
        s1 = p0 + p1
        s2 = s1 + p2
        out[..., i] = s2 + C[i, 3]
        L = max([L, abs(C[i, 3])] + [np.abs(t).max() for t in (p0, p1, p2, s1, s2, out[..., i])])
    return out, float(L)


def colour_bwd(g, row):
    C = colour_of(row)
    out = np.zeros(g.shape)
    L = np.abs(g).max() if g.size else 0.0
    for j in range(3):
        p0, p1, p2 = C[0, j] * g[..., 0], C[1, j] * g[..., 1], C[2, j] * g[..., 2]
        s1 = p0 + p1
        out[..., j] = s1 + p2
        L = max([L] + [np.abs(t).max() for t in (p0, p1, p2, s1, out[..., j])])
    return out, float(L)


def random_colour(rng):
    return (np.eye(3, 4) + rng.uniform(-0.7, 0.7, size=(3, 4))).astype(np.float32).reshape(-1)


def special_values(shape, seed):
    """float32 data in about [-1, 1] sprinkled with -0.0, +-inf, NaNs with payloads and denormals, as int32 bits."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32).view(np.int32).reshape(-1).copy()
    specials = np.asarray([0x80000000, 0x7f800000, 0xff800000, 0x7fc0dead, 0xffc12345, 0x7f800001, 0x00000001, 0x807fffff, 0],
                          np.uint32).view(np.int32)
    idx = rng.choice(x.size, size=max(len(specials), x.size // 5), replace=False)
    x[idx] = specials[np.arange(idx.size) % len(specials)]
    return x.reshape(shape)


def box_side_bound(row):
    """The longest side the adjoint's box of this row can have before the clamps (the header's formula), or inf."""
    g = np.asarray(row[6:12], np.int32).view(np.float32).astype(np.float64)
    m = min(max(int(row[12]), 0), MAX_MARGIN)
    h = max(abs(g[0]) + abs(g[1]), abs(g[3]) + abs(g[4]))
    if not np.isfinite(h):
        return float("inf")
    return int(np.floor(2.0 * h + 2.0)) + 1 + 2 * m
