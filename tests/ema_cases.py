"""The cases of the weight-EMA kernel (csrc/ema.hip, ops.ema_update / ema_swap / ema_fill) and a float64 restatement of its
update (no GPU needed to import this file; the library is loaded only when the table is built: the chunk size is the
wrapper's).

THE CONTRACT (include/csg_hip.h).  Kind AVERAGE, with d = (float)D and omd = (float)(1.0 - (double)D) made on the host:
        t  = fl32(omd * p)            one multiplication, rounded
        e' = fl32(d * e + t)          one fused multiply-add: the product d * e is exact, the sum is rounded once
    omd == 0 (D = 1): e' = e, bit for bit.  Kind COPY: e' = p, bit for bit.

THE RESTATEMENT takes the same fp32 inputs and the same host-rounded d, omd and evaluates r = d * e + omd * p in float64.

THE BOUND, per element, derived from the sequence above and nothing else.  With u = 2^-24 (half an fp32 ulp, relative) and
eta = 2^-150 (half the smallest subnormal, the absolute rounding error where a result is subnormal):
        t  = omd p (1 + d1) + h1,                     |d1| <= u, |h1| <= eta
        e' = (d e + t)(1 + d2) + h2,                  |d2| <= u, |h2| <= eta
        e' - r = omd p d1 + h1 + (d e + t) d2 + h2
        |e' - r| <= u |omd p| + u |d e + t| + 2 eta,  and |d e + t| <= |r| + u |omd p| + eta
    so  |e' - r| <= u (|omd p| + |r|) (1 + SECOND) + FLOOR:   two roundings, the issue's 2^-24 (|omd p| + |e'|) with |e'| taken
    from the restatement, SECOND = 2^-20 covering the second-order terms (u^2, and |e'| against |r| over a handful of steps),
    FLOOR = 2^-149 the subnormal floor (2 eta).  The restatement's own float64 error, 2^-52 (|d e| + |omd p|), is added.
    Overflow: fp32 rounds an exact value to +-inf from 2^128 - 2^103 on; where |r| + bound reaches that, +-inf of r's sign is
    as correct a result as the largest finite number.  NaN: exactly where the restatement has NaN (inf * 0, inf - inf, a NaN
    input): NaN generation does not depend on the precision.  An infinite r is matched exactly.

REPEATED UPDATES against a float64 shadow advanced with the same d_n, omd_n and the device's fp32 parameters: the error obeys
    E_n <= d_n E_(n-1) + b_n, so E_K <= max_n b_n * min(K, 1 / (1 - d)), d the largest decay used — the geometric sum of errors
    damped by d (K itself when d = 1).
"""
import numpy as np

AVERAGE, COPY = 0, 1
U = 2.0 ** -24
SECOND = 2.0 ** -20
FLOOR = 2.0 ** -149
TO_INF = 2.0 ** 128 - 2.0 ** 103          # the smallest magnitude fp32 rounds to infinity
SENTINEL = np.uint32(0xDEADBEEF).view(np.int32)     # bits of the shadow's floats outside every slot

SIZES = ("0", "1", "3", "4", "5", "C-1", "C", "C+1", "2C+3")
DECAYS = (0.0, 1.0, 0.5, 0.999, 0.9999)
WARMUP_N = (1, 2, 90, 100000)             # update numbers whose warm-up decay min(0.9999, (1 + n) / (10 + n)) is a case

# values: +-0, the smallest and the largest subnormal, +-inf, NaNs (quiet with a payload, negative quiet, signalling), the
# largest finite number and its neighbourhood, two ordinary numbers
_SPECIAL_BITS = (0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC00001, 0x7F800001,
                 0x7F7FFFFF, 0xFF7FFFFE, 0x7F7FF000, 0x3F800000, 0xC0200000)
SPECIALS = np.array(_SPECIAL_BITS, dtype=np.uint32).view(np.float32)


def chunk():
    """The kernel's chunk size, as the wrapper states it."""
    from canonicalsg2im_amd import ops
    return int(ops.EMA_CHUNK)


def size_of(tag):
    C = chunk()
    return {"0": 0, "1": 1, "3": 3, "4": 4, "5": 5, "C-1": C - 1, "C": C, "C+1": C + 1, "2C+3": 2 * C + 3}[tag]


def warmup_decay(decay, n):
    """The classic num_updates rule, restated: min(decay, (1 + n) / (10 + n))."""
    return min(float(decay), (1.0 + n) / (10.0 + n))


def scalars(decay):
    """(d, omd) exactly as the wrapper computes them, restated with numpy: fp32 values held in Python floats."""
    D = float(decay)
    return float(np.float32(D)), float(np.float32(1.0 - D))


# ------------------------------------------------------------------------------------------------ the table
def _case(name, items, decay):
    return {"name": name, "items": tuple(items), "decay": float(decay)}


_TABLE = None


def table():
    """Every row: {"name", "items": ((numel, kind, values), ...), "decay"}; values "normal" | "special"."""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    C = chunk()
    rows = []
    # tensor sizes, one item, both kinds
    for tag in SIZES:
        for kind in (AVERAGE, COPY):
            rows.append(_case("size %s %s" % (tag, "average" if kind == AVERAGE else "copy"),
                              [(size_of(tag), kind, "normal")], 0.999))
    # two items of different kinds, every decay and the warm-up values
    two = [(5, AVERAGE, "normal"), (C + 1, COPY, "normal")]
    for D in DECAYS:
        rows.append(_case("two items decay %r" % D, two, D))
    for n in WARMUP_N:
        rows.append(_case("two items warm-up n=%d" % n, two[::-1], warmup_decay(0.9999, n)))
    # 300 small items of mixed kinds and sizes: the block-to-item lookup (sizes 0 .. 40, a few of them longer than a chunk)
    rng = np.random.RandomState(7)
    many = [(int(rng.randint(0, 41)), int(rng.randint(0, 2)), "normal") for _ in range(300)]
    for i in (17, 123, 250):
        many[i] = (C + int(rng.randint(1, 9)), many[i][1], "normal")
    for D in (0.999, 0.5, 1.0):
        rows.append(_case("300 items decay %r" % D, many, D))
    # position in a table: slots that need padding to the 4-float boundary; a zero-element item between two others, first, last
    rows.append(_case("padded slots", [(3, AVERAGE, "normal"), (5, COPY, "normal"), (1, AVERAGE, "normal"), (4, AVERAGE, "normal"),
                                       (7, COPY, "normal"), (C + 2, AVERAGE, "normal"), (2, COPY, "normal")], 0.999))
    rows.append(_case("empty between", [(5, AVERAGE, "normal"), (0, COPY, "normal"), (6, AVERAGE, "normal")], 0.999))
    rows.append(_case("empty between chunks", [(C, AVERAGE, "normal"), (0, AVERAGE, "normal"), (3, COPY, "normal")], 0.5))
    rows.append(_case("empty first and last", [(0, AVERAGE, "normal"), (0, COPY, "normal"), (9, AVERAGE, "normal"),
                                               (0, AVERAGE, "normal")], 0.9999))
    # values: every special in p against every special in e, in the 16-byte body and in the tail, both kinds
    ns = len(SPECIALS) ** 2 + 3
    for D in DECAYS + (warmup_decay(0.9999, 1),):
        rows.append(_case("special values decay %r" % D, [(ns, AVERAGE, "special"), (ns, COPY, "special")], D))
    _TABLE = rows
    return rows


def _values(numel, how, rng):
    if how == "normal":
        return rng.standard_normal(numel).astype(np.float32), rng.standard_normal(numel).astype(np.float32)
    n = len(SPECIALS)
    p = np.repeat(SPECIALS, n)                      # every pair (p, e)
    e = np.tile(SPECIALS, n)
    reps = -(-numel // p.size)
    return np.tile(p, reps)[:numel].copy(), np.tile(e, reps)[:numel].copy()


def make(case):
    """[(p, e, kind)] of a case: fp32 arrays of the live values and of the shadow's, reproducible."""
    rng = np.random.RandomState(_seed(case["name"]))
    return [(_values(n, how, rng) + (kind,)) for n, kind, how in case["items"]]


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31)


# ------------------------------------------------------------------------------------------------ the restatement
def restate(p, e, kind, d, omd):
    """-> (exact, ref): exact = True: ref is fp32 and the device's bits must EQUAL it; else ref = d e + omd p in float64."""
    if kind == COPY:
        return True, p
    if omd == 0.0:
        return True, e
    with np.errstate(invalid="ignore", over="ignore"):
        return False, np.float64(d) * e.astype(np.float64) + np.float64(omd) * p.astype(np.float64)


def step_bound(p, e, ref, d, omd):
    """The per-element bound of one update (see the derivation above); inf / NaN where ref is."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(np.float64(omd) * p.astype(np.float64))
        de = np.abs(np.float64(d) * e.astype(np.float64))
        return U * (a + np.abs(ref)) * (1.0 + SECOND) + FLOOR + 2.0 ** -52 * (de + a)


def steps_factor(K, d_max):
    """min(K, 1 / (1 - d)): how many per-step bounds K updates with decays up to d_max can pile up."""
    return float(K) if d_max >= 1.0 else min(float(K), 1.0 / (1.0 - d_max))


def check_average(got, ref, bound, what):
    """`got` (fp32) against the float64 `ref` within `bound`: NaN exactly where ref has it, an infinite ref matched exactly,
    +-inf accepted where |ref| + bound reaches fp32's rounding threshold to infinity.  -> the worst |got - ref| / bound."""
    got = np.asarray(got, dtype=np.float32).astype(np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN at %s, the restatement has NaN at %s" % (
        what, np.flatnonzero(np.isnan(got))[:8], np.flatnonzero(nan)[:8])
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), "%s: an infinite result differs" % what
    fin = ~nan & ~inf
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got - ref)
        over = fin & (np.abs(ref) + bound >= TO_INF) & np.isinf(got) & (np.sign(got) == np.sign(ref))
        bad = fin & ~over & ~(err <= bound)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: element %d is %r, the restatement %r: error %.3e beyond the bound %.3e (%d elements)" % (
            what, i, got[i], ref[i], err[i], bound[i], int(bad.sum())))
    ok = fin & ~over
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def fp32_evaluation(p, e, kind, d, omd):
    """A straightforward fp32 evaluation of the stated sequence on the host: t = fl32(omd p); e' = fl32(d e + t), the fused
    multiply-add formed through float64 (d e is exact there, 48 bits; the sum is rounded to 53 bits and then to 24, a double
    rounding that differs from the single one by at most 2^-29 of an ulp)."""
    if kind == COPY:
        return p.copy()
    if omd == 0.0:
        return e.copy()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = (np.float32(omd) * p).astype(np.float32)
        return (np.float64(d) * e.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
