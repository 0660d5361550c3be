"""The ADA augmentation pipeline without a device: the host half of csrc/csg_ada_pipeline.h (`ops.ada_pipeline_table_host`)
against the numpy restatement of tests/ada_pipeline_cases.py as bits, the polynomials against numpy's own functions, the
flag words, the independence of the groups' draws, the search boxes of generated rows, and the flags with their refusals."""
import numpy as np
import pytest

import ada_cases as ad
import ada_pipeline_cases as ap
import augment_cases as ac


# ------------------------------------------------------------------------------------------------ the host table
@pytest.mark.parametrize("H", ap.TABLE_H)
def test_host_table_equals_the_restatement(H):
    from canonicalsg2im_amd import ops
    rows = 48
    for seed, iteration, pass_id, rank in ap.KEYS:
        for p24 in ap.P24_VALUES:
            for policy in ap.POLICIES:
                got = ops.ada_pipeline_table_host(seed, iteration, pass_id, rows, H, policy, p24, rank=rank).numpy()
                want = ap.table_np(seed, iteration, pass_id, rank, rows, H, policy, p24)
                bad = np.argwhere(got != want)
                assert got.shape == (rows, ap.ROW_WORDS) and bad.size == 0, (H, p24, policy, bad[:4].tolist())


def test_rotation_threshold():
    """prot24 = floor((1 - sqrt(1 - p)) 2^24): 0 at p = 0, 2^24 at p = 1, and p_rot (2 - p_rot) = p within a 2^-24 step."""
    assert ap.prot24_of(0) == 0 and ap.prot24_of(ap.ONE) == ap.ONE
    for p24 in (1, 1 << 12, 1 << 23, ap.ONE - 1):
        r = ap.prot24_of(p24) / ap.ONE
        assert r * (2.0 - r) <= p24 / ap.ONE < (r + 2.0 ** -24) * (2.0 - r - 2.0 ** -24) + 2.0 ** -23, p24


def test_polynomials_against_numpy():
    """sin / cos over every 5th of the 2^24 angles and around the octant boundaries, exp2 over a dense sweep of [-6, 6]:
    within 2^-40 relative of numpy's functions evaluated in long double (64-bit mantissa where the platform has one).  The
    reference's own argument error — 2 pi u 2^-24 rounded to its format — is an ABSOLUTE error of up to eps_ref * 2 pi in the
    angle, which matters only at the zeros of sin and cos, where the relative error of any reference is unbounded: the floor
    4 eps_ref covers it and nothing else."""
    ld = np.longdouble
    eps = float(np.finfo(ld).eps)
    u = np.unique(np.concatenate([np.arange(0, 1 << 24, 5)] + [np.arange(max(b - 64, 0), min(b + 64, 1 << 24))
                                                                for b in range(0, (1 << 24) + 1, 1 << 21)]))
    s, c = ap.sincos_np(u)
    pi = ld("3.14159265358979323846264338327950288")
    ang = u.astype(ld) * (ld(2) * pi / ld(1 << 24))
    for name, got, ref in (("sin", s, np.sin(ang)), ("cos", c, np.cos(ang))):
        err = np.abs(got.astype(ld) - ref)
        bound = ld(2.0 ** -40) * np.abs(ref) + ld(4 * eps)
        worst = float(np.max(err / bound))
        print("%s: worst error / bound %.3g over %d angles" % (name, worst, u.size))
        assert worst <= 1.0, name
    assert np.all(s * s + c * c > 1 - 2.0 ** -50)
    e = np.concatenate([np.linspace(-6.0, 6.0, 1200001), np.arange(-6, 7) + 0.5, np.arange(-6, 7) - 2.0 ** -30])
    got, ref = ap.exp2_np(e), np.exp2(e.astype(ld))
    worst = float(np.max(np.abs(got.astype(ld) - ref) / (ld(2.0 ** -40) * ref)))
    print("exp2: worst error / bound %.3g over %d exponents" % (worst, e.size))
    assert worst <= 1.0
    assert np.array_equal(ap.exp2_np(np.arange(-6.0, 7.0)), 2.0 ** np.arange(-6.0, 7.0))          # exact at integers


def test_normal_is_bounded_and_has_unit_variance():
    """The sum of twelve uniform draws: |z| <= 6 by construction; over 2^16 rows the mean is within 6 / sqrt(n) and the variance
    within 6 sqrt(2 / n) of 1 (six standard errors of a unit-variance sample; the Irwin-Hall kurtosis is below a normal's)."""
    n = 1 << 16
    z = ap.normal_np(ap.key_np(3, 9, 1, 0, n), 24)
    assert np.abs(z).max() <= 6.0 and abs(z.mean()) <= 6.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 6.0 * np.sqrt(2.0 / n)
    assert np.array_equal(z * 2.0 ** 24, np.round(z * 2.0 ** 24))                                   # a multiple of 2^-24: exact


# ------------------------------------------------------------------------------------------------ the flag words
def test_p_zero_rows_are_identities_and_blit_rows_are_integer_maps():
    from canonicalsg2im_amd import ops
    for H in (5, 8):
        for policy in ap.POLICIES:
            t = ops.ada_pipeline_table_host(1, 2, 0, 64, H, policy, 0).numpy()
            assert (t[:, 13] == (ap.GEOM_ID | ap.GEOM_INT | ap.COLOR_ID)).all(), (H, policy)
            ident = ap.make_row(H, flags=7)
            assert (t == ident[None]).all(), "a p = 0 row is the identity's words"
        t = ops.ada_pipeline_table_host(1, 2, 0, 64, H, ap.BLIT, ap.ONE).numpy()
        assert (t[:, 13] == (ap.GEOM_INT | ap.COLOR_ID)).all()
        flip, k, tx, ty, _ = ap.blit_draws(ap.key_np(1, 2, 0, 0, 64), H, ap.ONE)
        assert len(set(zip(flip.tolist(), k.tolist()))) == 8, "64 rows should meet all 8 signed permutations"
        for n in range(64):
            assert tuple(t[n, [28, 29, 30, 31, 14, 15]]) == ap.blit_map(bool(flip[n]), int(k[n]), int(tx[n]), int(ty[n]), H), n
        t = ops.ada_pipeline_table_host(1, 2, 0, 64, H, ap.BLIT | ap.GEOM | ap.COLOR, ap.ONE).numpy()
        assert (t[:, 13] == 0).all() and (t[:, 12] == 1).all()


def test_groups_do_not_move_each_others_draws():
    from canonicalsg2im_amd import ops
    key, H, p24 = (11, 5, 1, 3), 16, 1 << 23

    def table(policy):
        return ops.ada_pipeline_table_host(key[0], key[1], key[2], 96, H, policy, p24, rank=key[3]).numpy()
    full = table(56)
    colour, intmap, geo = list(range(16, 28)), [14, 15, 28, 29, 30, 31], list(range(0, 12))
    for policy in (32, 40, 48):
        assert np.array_equal(table(policy)[:, colour], full[:, colour]), policy
    for policy in (8, 24, 40):
        assert np.array_equal(table(policy)[:, intmap], full[:, intmap]), policy
    assert np.array_equal(table(16)[:, geo], table(48)[:, geo]) and np.array_equal(table(24)[:, geo], full[:, geo])
    assert not np.array_equal(table(16)[:, geo], full[:, geo])
    # DiffAugment's rows (draws 1..7) and gates (8..10) are what they were
    assert np.array_equal(ops.augment_table_host(key[0], key[1], key[2], 96, H, rank=key[3]).numpy(),
                          ac.table_np(key[0], key[1], key[2], key[3], 96, H))
    assert np.array_equal(ops.augment_gate_host(key[0], key[1], key[2], 96, p24, rank=key[3]).numpy(),
                          ad.gate_np(key[0], key[1], key[2], key[3], 96, p24))
    assert [list(r) for r in ops.augment_table_host(*ac.ROW_VECTORS_KEY[:3], 3, ac.ROW_VECTORS_KEY[4],
                                                    rank=ac.ROW_VECTORS_KEY[3]).tolist()] == ac.ROW_VECTORS


def test_search_boxes_of_generated_rows():
    """10^5 keys at p = 1 with every group on: the box side the header's formula gives stays within CSG_ADA_MAX_BOX, the
    margin is 1, and G is M's inverse to fp32 accuracy (|G M - I| entries below 2^-20)."""
    from canonicalsg2im_amd import ops
    assert ops.ADA_MAX_BOX == ap.MAX_BOX and ops.ADA_ROW_WORDS == ap.ROW_WORDS
    t = ops.ada_pipeline_table_host(5, 77, 0, 100000, 256, 56, ap.ONE).numpy()
    g = t[:, 6:12].view(np.float32).astype(np.float64)
    m = t[:, 0:6].view(np.float32).astype(np.float64)
    half = np.maximum(np.abs(g[:, 0]) + np.abs(g[:, 1]), np.abs(g[:, 3]) + np.abs(g[:, 4]))
    side = np.floor(2.0 * half + 2.0) + 1 + 2 * t[:, 12]
    print("largest half side %.4f, largest box side %d" % (half.max(), int(side.max())))
    assert (t[:, 12] == 1).all() and side.max() <= ap.MAX_BOX and half.max() < 4.0 * np.sqrt(2.0) * (1 + 2.0 ** -20)
    assert side.max() == max(ap.box_side_bound(r) for r in t[np.argsort(half)[-4:]])
    prod = np.stack([g[:, 0] * m[:, 0] + g[:, 1] * m[:, 3], g[:, 0] * m[:, 1] + g[:, 1] * m[:, 4],
                     g[:, 3] * m[:, 0] + g[:, 4] * m[:, 3], g[:, 3] * m[:, 1] + g[:, 4] * m[:, 4]], 1)
    assert np.abs(prod - np.asarray([1.0, 0.0, 0.0, 1.0])).max() < 2.0 ** -20


def test_host_entry_refusals():
    import ctypes
    from canonicalsg2im_amd._lib import last_error, lib
    buf = np.zeros((4, 32), np.int32)
    p = ctypes.c_void_p(buf.ctypes.data)
    for args, what in (((0, -1, 0, 0, 4, 8, 56, 0, p), "non-negative"), ((0, 0, 0, 0, -1, 8, 56, 0, p), "rows"),
                       ((0, 0, 0, 0, 4, 1, 56, 0, p), "H = 1"), ((0, 0, 0, 0, 4, 8, 64, 0, p), "policy 64"),
                       ((0, 0, 0, 0, 4, 8, 56, -1, p), "p24 = -1"), ((0, 0, 0, 0, 4, 8, 56, ap.ONE + 1, p), "p24 = "),
                       ((0, 0, 0, 0, 4, 8, 56, 0, None), "null table")):
        assert lib.csg_ada_pipeline_table_host(*args) != 0 and what in last_error(), (what, last_error())
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ the flags
def test_policy_names_and_masks():
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd.d_augment import policy_mask, policy_names
    assert (ops.AUG_ADA_BLIT, ops.AUG_ADA_GEOM, ops.AUG_ADA_COLOR) == (8, 16, 32) == (ap.BLIT, ap.GEOM, ap.COLOR)
    assert [policy_mask(p) for p in ("ada_blit", "ada_geom", "ada_color", "color,ada_geom", "ada_color, ada_blit ,cutout")] == \
        [8, 16, 32, 17, 44]
    assert policy_names(6) == "translation,cutout" and policy_names(63) == "color,translation,cutout,ada_blit,ada_geom,ada_color"
    assert policy_names(48) == "ada_geom,ada_color"
    with pytest.raises(ValueError, match="unknown policy 'ada' .*color,translation,cutout,ada_blit,ada_geom,ada_color"):
        policy_mask("ada")
    with pytest.raises(ValueError, match="comma list out of color,translation,cutout"):
        policy_mask(["color"])


def test_ada_names_need_a_strength():
    from canonicalsg2im_amd.d_augment import ada_settings
    for policies in ("ada_blit", "color,ada_geom", "ada_blit,ada_geom,ada_color"):
        for flags in ({}, {"interval": 2}, {"kimg": 10.0}, {"target": 0.0}, {"target": 0.0, "interval": 3}):
            with pytest.raises(ValueError, match="need a strength.*p = 1 these transforms leak into the generator"):
                ada_settings(policies=policies, **flags)
        assert ada_settings(p=0.5, policies=policies)["p24"] == 1 << 23
        assert ada_settings(p=1.0, policies=policies)["p24"] == ap.ONE            # said on purpose: allowed
        s = ada_settings(target=0.6, policies=policies)
        assert s["adaptive"] and s["p24"] == 0
    # the old names and the old messages are what they were
    assert ada_settings(policies="color,translation,cutout") is None
    with pytest.raises(ValueError, match="without --d_augment policies: there is nothing to gate .*color,translation,cutout"):
        ada_settings(p=0.5)
    with pytest.raises(ValueError, match="--d_augment_p must be in"):
        ada_settings(p=1.5, policies="ada_blit")


def test_parser_refusals(capsys):
    from canonicalsg2im_amd.scripts.args import build_parser
    parser = build_parser()
    ok = parser.parse_args(["--d_augment", "ada_color,ada_blit", "--d_augment_p", "0.25"])
    assert ok.d_augment == "ada_blit,ada_color" and ok.d_augment_p == 0.25
    for argv, what in ((["--d_augment", "ada_geom"], "need a strength"), (["--d_augment", "ada_foo", "--d_augment_p", "1"], "unknown policy"),
                       (["--d_augment", "color,ada_blit", "--d_augment_interval", "2"], "need a strength")):
        with pytest.raises(SystemExit):
            parser.parse_args(argv)
        assert what in capsys.readouterr().err, argv
