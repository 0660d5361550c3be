"""Precision / recall and density / coverage on the host (no GPU): the restatement of tests/prdc_cases.py against hand-worked
integers and a double loop, the margins that make the random rows decidable, the split rule through its host entry, and the
host-only refusals of the parser, `ops` and `quality`."""
import numpy as np
import pytest
import torch

import prdc_cases as pc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from canonicalsg2im_amd import _lib
    return _lib.lib


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_gives_the_hand_worked_integers():
    real, gen = pc.line_points(pc.HAND_REAL_X), pc.line_points(pc.HAND_GEN_X)
    r2_real, r2_gen = pc.radii_ref(real, pc.HAND_K), pc.radii_ref(gen, pc.HAND_K)
    assert r2_real.tolist() == pc.HAND["r2_real"] and r2_gen.tolist() == pc.HAND["r2_gen"]
    inside, holds = pc.counts_ref(gen, real, r2_real)
    assert inside.tolist() == pc.HAND["inside_gen"] and holds.tolist() == pc.HAND["holds_real"]
    inside_r, _ = pc.counts_ref(real, gen, r2_gen)
    assert inside_r.tolist() == pc.HAND["inside_real"]
    # the point 3 lies ON the sphere of 2: the "<=" tie
    assert pc.d2_ref(gen, real)[1, 2] == r2_real[2] == 1.0
    out = pc.prdc_ref(real, gen, pc.HAND_K)
    for name in ("precision", "recall", "density", "coverage"):
        assert out[name] == pc.HAND[name], (name, out[name])
    assert out["k"] == 1 and out["n"] == [4, 3]


def test_restatement_against_a_double_loop():
    real, gen, k = pc.grid_case(9, 7, 64, 2, seed=3)
    real[4] = real[2]                                          # a twin
    d = np.empty((7, 9))
    for j in range(7):
        for i in range(9):
            acc = 0.0
            for c in range(64):
                t = float(gen[j, c]) - float(real[i, c])
                acc += t * t
            d[j, i] = acc
    assert np.array_equal(d, pc.d2_ref(gen, real))
    r2 = []
    for i in range(9):
        others = sorted(float(((real[i].astype(np.float64) - real[j].astype(np.float64)) ** 2).sum()) for j in range(9) if j != i)
        r2.append(others[k - 1])
    assert r2 == pc.radii_ref(real, k).tolist()
    assert pc.radii_ref(real, 1)[2] == 0.0 and pc.radii_ref(real, 1)[4] == 0.0          # the twin counts, self does not
    inside, holds = pc.counts_ref(gen, real, np.array(r2))
    assert inside.tolist() == [sum(d[j, i] <= r2[i] for i in range(9)) for j in range(7)]
    assert holds.tolist() == [sum(d[j, i] <= r2[i] for j in range(7)) for i in range(9)]


def test_grid_rows_are_exact_tied_and_discriminating():
    name, n, m, D, k, ties = pc.GRID_CASES[0]
    real, gen, k = pc.grid_case(n, m, D, k, ties=ties)
    d = pc.d2_ref(gen, real)
    assert np.array_equal(d, np.round(d)) and d.max() < 2.0 ** 20              # exact integers under any order or fusing
    r2 = pc.radii_ref(real, k)
    assert (r2[:4] == 0.0).all() and r2[5] > 0.0                               # four identical rows, k = 3; one twin, k = 3
    assert pc.radii_ref(real, 1)[5] == 0.0 and pc.radii_ref(real, 1)[6] == 0.0
    inside, holds = pc.counts_ref(gen, real, r2)
    assert inside[0] >= 4 and (holds[:4] >= 1).all()                           # the query equal to them is inside, at 0 <= 0
    assert int((d == r2[None, :]).sum()) >= 4                                  # pairs exactly on a sphere
    out = pc.prdc_ref(real, gen, k)
    print("grid ties case: %s, %d pairs on a sphere" % (out, int((d == r2[None, :]).sum())))
    # a read past the end of either operand would change the integers of the masking row
    f_big, q_big, n, m = pc.masked_operands(*pc.MASK_CASE)
    k = pc.MASK_CASE[3]
    clean = pc.counts_ref(q_big[:m], f_big[:n], pc.radii_ref(f_big[:n], k))
    leaky = pc.counts_ref(q_big[:64 * 2], f_big[:64 * 2], pc.radii_ref(f_big[:64 * 2], k))
    assert not np.array_equal(clean[0], leaky[0][:m]) and not np.array_equal(clean[1], leaky[1][:n])
    assert not np.array_equal(pc.radii_ref(f_big[:n], k), pc.radii_ref(f_big[:64 * 2], k)[:n])


@pytest.mark.parametrize("case", pc.RANDOM_CASES)
def test_random_rows_have_no_undecided_pair_or_neighbour(case):
    n, m, D, k, seed = case
    real, gen, k = pc.random_case(*case)
    for f, q in ((real, gen), (gen, real)):
        r2 = pc.radii_ref(f, k)
        d = pc.d2_ref(q, f)
        assert len(pc.undecided_pairs(d, r2, D)) == 0
        pair_margin = float((np.abs(d - r2[None, :]) / r2[None, :]).min())
        margin = pc.neighbour_margin(f, k)
        print("random case %s: smallest relative margin %.2e for pairs, %.2e for neighbours; bound %.2e" % (
            case, pair_margin, margin, (D + 2) * 2.0 ** -51))
        assert pair_margin > (D + 2) * 2.0 ** -51 and margin > (D + 2) * 2.0 ** -51
    out = pc.prdc_ref(real, gen, k)
    print("random case %s: %s" % (case, out))
    if case == pc.INTERIOR_CASE:
        assert all(0.0 < out[name] < 1.0 for name in ("precision", "recall", "coverage")) and out["density"] > 0.0


def test_nonfinite_rows_rank_as_infinitely_far():
    bad, clean, gen, k = pc.nonfinite_case()
    keep = [i for i in range(len(bad)) if i not in pc.NONFINITE_ROWS]
    r2 = pc.radii_ref(bad, k)
    assert np.isinf(r2[list(pc.NONFINITE_ROWS)]).all() and np.array_equal(r2[keep], pc.radii_ref(clean, k))
    inside, holds = pc.counts_ref(gen, bad, r2)
    want_inside, want_holds = pc.counts_ref(gen, clean, pc.radii_ref(clean, k))
    assert (holds[list(pc.NONFINITE_ROWS)] == 0).all() and np.array_equal(holds[keep], want_holds)
    assert np.array_equal(inside, want_inside)
    inside_r, _ = pc.counts_ref(bad, gen, pc.radii_ref(gen, k))
    assert (inside_r[list(pc.NONFINITE_ROWS)] == 0).all()                      # inside nothing


# ------------------------------------------------------------------------------------------------ the split rule
def test_column_chunks_entry_is_the_stated_rule_and_its_boundaries(lib):
    chunks = lib.csg_manifold_column_chunks
    found = pc.chunk_boundaries(lambda r, c: int(chunks(r, c)))
    assert found == pc.chunk_boundaries(pc.chunks_rule) == [128 * i for i in range(1, 8)], found
    for rows, cols in ((1, 1), (64, 64), (65, 65), (130, 130), (1000, 70), (70, 1000), (10000, 10000), (50000, 50000),
                       (4096, 50000), (1 << 20, 1 << 20), (64, 1 << 20)):
        got = int(chunks(rows, cols))
        assert got == pc.chunks_rule(rows, cols) and 1 <= got <= 64, (rows, cols, got)
    assert int(chunks(130, 130)) == 2 and int(chunks(10000, 10000)) == 53 and int(chunks(1 << 20, 1 << 20)) == 1
    for rows, cols in ((0, 5), (5, 0), (-1, 5), ((1 << 20) + 1, 5), (5, (1 << 20) + 1)):
        assert int(chunks(rows, cols)) == -1


def test_workspace_entries_follow_the_rule_and_return_minus_one_outside_the_limits(lib):
    radii, balls, chunks = lib.csg_knn_radii_workspace_bytes, lib.csg_ball_counts_workspace_bytes, lib.csg_manifold_column_chunks
    for n, k in ((2, 1), (17, 16), (130, 3), (10000, 5), (1 << 20, 16)):
        assert int(radii(n, k)) == int(chunks(n, n)) * n * k * 8
    for n, k in ((1, 1), (5, 0), (5, 5), (5, 6), (100, 17), ((1 << 20) + 1, 5), (0, 1), (-3, 1)):
        assert int(radii(n, k)) == -1, (n, k)
    for m, n in ((1, 2), (65, 130), (130, 65), (10000, 10000), (50000, 50000)):
        groups = min(64, -(-m // 64))
        assert int(balls(m, n)) == (m * int(chunks(min(m, 4096), n)) + n * groups) * 4
    # O((n + m) chunks k) with chunks <= 64: never an n x m array
    assert int(radii(50000, 5)) <= 50000 * 64 * 5 * 8 and int(balls(50000, 50000)) <= 2 * 50000 * 64 * 4
    for m, n in ((0, 5), (5, 0), ((1 << 20) + 1, 5), (5, (1 << 20) + 1)):
        assert int(balls(m, n)) == -1


def test_row_groups_of_ball_counts_on_each_side_of_4096(lib):
    """The second launch rule of csg_ball_counts, read off its workspace: (m chunks + n groups) 4 bytes.  Up to m = 4096 every
    group is one query tile; from 4097 on there are more tiles than groups and a block walks several."""
    balls, chunks = lib.csg_ball_counts_workspace_bytes, lib.csg_manifold_column_chunks
    n = 130
    for m, groups, tiles in ((1, 1, 1), (64, 1, 1), (65, 2, 2), (4032, 63, 63), (4095, 64, 64), (4096, 64, 64), (4097, 64, 65),
                             (4161, 64, 66), (8259, 64, 130), (50000, 64, 782), (1 << 20, 64, 16384)):
        got = (int(balls(m, n)) // 4 - m * int(chunks(min(m, 4096), n))) // n
        assert got == groups == pc.row_groups_rule(m) and -(-m // 64) == tiles, (m, got)
    walked = [-(-m // 64) > pc.row_groups_rule(m) for m, _ in pc.ROW_GROUP_CASES]
    assert walked == [False, True, True]                       # the cases stand on both sides of the rule's change
    # the cases discriminate: counts strictly between nothing and everything, and pairs exactly on a sphere
    for m, n in pc.ROW_GROUP_CASES[1:2]:
        for a, b in ((m, n), (n, m)):
            q, f, r2 = pc.row_group_case(a, b)
            d = pc.d2_ref(q, f)
            inside, holds = pc.counts_ref(q, f, r2, d=d)
            assert 0 < inside.sum() < a * b and len(set(holds.tolist())) > 8 and int((d == r2[None, :]).sum()) > 0


# ------------------------------------------------------------------------------------------------ parser
def test_quality_script_parses_prdc_flags():
    from canonicalsg2im_amd.scripts import quality as script
    a = script.build_parser().parse_args(["A", "B", "--fid_weights", "random"])
    assert a.prdc is False and a.prdc_k == 5 and a.prdc_real == "A"
    b = script.build_parser().parse_args(["A", "B", "--fid_weights", "random", "--prdc", "--prdc_k", "3", "--prdc_real", "B"])
    assert b.prdc is True and b.prdc_k == 3 and b.prdc_real == "B"
    with pytest.raises(SystemExit):
        script.build_parser().parse_args(["A", "B", "--fid_weights", "random", "--prdc", "--prdc_real", "C"])


def test_quality_script_refuses_prdc_for_statistics_files():
    from canonicalsg2im_amd.scripts import quality as script
    with pytest.raises(SystemExit, match=r"--prdc needs pictures: stats_A\.npz holds statistics"):
        script.main(["stats_A.npz", "B", "--fid_weights", "random", "--prdc"])
    with pytest.raises(SystemExit, match=r"--kid and --prdc need pictures: .*stats_B\.npz"):
        script.main(["A", "dir/stats_B.npz", "--fid_weights", "random", "--kid", "--prdc"])


# ------------------------------------------------------------------------------------------------ refusals without a device
def test_ops_refuse_bad_operands_on_the_host(lib):
    from canonicalsg2im_amd import ops
    f = torch.zeros(8, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.knn_radii(f, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ball_counts(f, f, torch.zeros(8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="compute in fp32"):
        ops.knn_radii(f.double(), 3)
    with pytest.raises(RuntimeError, match="compute in fp32"):
        ops.ball_counts(f.half(), f, torch.zeros(8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="knn_radii: f must be a dense float32 tensor"):
        ops.knn_radii(torch.zeros(8, 128)[:, ::2], 3)
    with pytest.raises(RuntimeError, match="ball_counts: q must be a dense float32 tensor"):
        ops.ball_counts(torch.zeros(8, 128)[:, ::2], f, torch.zeros(8, dtype=torch.float64))
    # (as with kid_sums, the first operand's device is checked before the next operand is looked at: refusals of f and r2
    # are in tests/test_gpu_prdc.py)


def test_prdc_refuses_bad_operands_on_the_host():
    from canonicalsg2im_amd import quality
    a, b = torch.zeros(6, 64), torch.zeros(9, 64)
    for k in (6, 7, 0, -1):
        with pytest.raises(ValueError, match=r"PRDC: k = -?\d+ needs 1 <= k < min\(n_real, n_gen\) = 6"):
            quality.prdc_from_features(a, b, k)
    with pytest.raises(ValueError, match="differ in width"):
        quality.prdc_from_features(a, torch.zeros(9, 128), 2)
    with pytest.raises(ValueError, match="fp32"):
        quality.prdc_from_features(a.double(), b.double(), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        quality.prdc_from_features(a, b, 5)
