"""KID and the object-level FID on the host (no GPU): the restatements of tests/quality_cases.py against hand-worked values, and
the host-only parts of the feature — quality.crops_from_layouts, quality.class_mean_distance, the new flags of scripts.quality
and its refusal of .npz statistics."""
import json

import numpy as np
import pytest

import quality_cases as qc


# ------------------------------------------------------------------------------------------------ restatements
def test_window_restatement_gives_the_hand_worked_integers():
    got = qc.windows_ref(qc.BOXES, qc.H, qc.W)
    for (name, _, want), row in zip(qc.WINDOW_ROWS, got):
        assert row.tolist() == want, (name, row.tolist(), want)
    # every row, the non-finite ones included: inside the picture, at least one pixel
    assert (got[:, 0] >= 0).all() and (got[:, 1] >= 0).all() and (got[:, 2] <= qc.W).all() and (got[:, 3] <= qc.H).all()
    assert (got[:, 2] > got[:, 0]).all() and (got[:, 3] > got[:, 1]).all()
    assert np.isfinite(qc.BOXES[:qc.N_FINITE]).all() and np.abs(qc.BOXES[:qc.N_FINITE]).max() <= 1.5
    assert [r[0] for r in qc.WINDOW_ROWS[qc.N_FINITE:]] == ["NaN", "+inf", "-inf", "1e30", "mixed"]
    assert len(qc.IMAGE_INDEX) == qc.N_FINITE and set(qc.IMAGE_INDEX.tolist()) == {0, 1}
    # the rule is in fp32: in exact arithmetic 7/13 * 13 = 7 and the window of "fp32 decides" would end at 7
    assert float(np.float32(7 / 13) * np.float32(13)) > 7.0


def _k(u, v, gamma, coef0, degree):
    return (gamma * float(np.dot(u.astype(np.float64), v.astype(np.float64))) + coef0) ** degree


def test_kid_restatement_against_a_triple_loop_and_the_closed_form_for_two_rows():
    nx, ny, m, D, S = qc.KID_CASES[0]
    assert m == 2
    fx, fy = qc.kid_features(nx, ny, D)
    ix, iy = qc.draw_subsets(nx, ny, m, S)
    gamma = 1.0 / D
    sums, mags = qc.kid_sums_ref(fx, fy, ix, iy, gamma, 1.0, 3)
    for s in range(S):
        want = [0.0, 0.0, 0.0]
        for i in range(m):
            for j in range(m):
                if i != j:
                    want[0] += _k(fx[ix[s, i]], fx[ix[s, j]], gamma, 1.0, 3)
                    want[1] += _k(fy[iy[s, i]], fy[iy[s, j]], gamma, 1.0, 3)
                want[2] += _k(fx[ix[s, i]], fy[iy[s, j]], gamma, 1.0, 3)
        assert np.allclose(sums[s], want, rtol=1e-14, atol=0)
        assert np.allclose(mags[s], want, rtol=1e-14, atol=0)           # non-negative features: k > 0
        x0, x1, y0, y1 = fx[ix[s, 0]], fx[ix[s, 1]], fy[iy[s, 0]], fy[iy[s, 1]]
        closed = _k(x0, x1, gamma, 1.0, 3) + _k(y0, y1, gamma, 1.0, 3) - 0.5 * sum(
            _k(a, b, gamma, 1.0, 3) for a in (x0, x1) for b in (y0, y1))
        assert abs(qc.mmd2(sums, m)[s] - closed) <= 1e-13 * abs(closed)


def test_kid_cases_discriminate():
    """|MMD^2| of every case is far above the tolerance the device test allows it."""
    for nx, ny, m, D, S in qc.KID_CASES:
        fx, fy = qc.kid_features(nx, ny, D)
        ix, iy = qc.draw_subsets(nx, ny, m, S)
        sums, mags = qc.kid_sums_ref(fx, fy, ix, iy, 1.0 / D, 1.0, 3)
        _, tol = qc.kid_tolerances(mags, m, D)
        value = qc.mmd2(sums, m)
        print("KID case %s: MMD^2 %s, tolerance %s" % ((nx, ny, m, D, S), value, tol))
        assert (np.abs(value) >= 1.9e-3).all() and (tol <= 1e-9).all() and (np.abs(value) >= 1e6 * tol).all()


# ------------------------------------------------------------------------------------------------ host parts of the feature
def test_crops_from_layouts():
    from canonicalsg2im_amd import quality
    doc = qc.layouts_doc()
    red = json.dumps({"color": "red", "shape": "sphere"}, sort_keys=True)
    gt = quality.crops_from_layouts(doc)
    assert list(gt) == [3, "a7"]
    assert gt[3] == ([[0.1, 0.1, 0.5, 0.5], [0.2, 0.3, 0.1, 0.1]], ["cube", red])          # the NaN box is left out
    assert gt["a7"] == ([[0.5, 0.5, 0.4, 0.4], [0.0, 0.6, 0.05, 0.1]], [red, "cylinder"])  # one key for either key order
    pred = quality.crops_from_layouts(doc, which="pred")
    assert pred[3][0][2] == [0.0, 0.0, 0.3, 0.2] and pred[3][1] == ["cube", red, "cube"]
    big = quality.crops_from_layouts(doc, min_object_size=0.02)                           # w * h: 0.25, 0.01 | 0.16, 0.005
    assert big[3] == ([[0.1, 0.1, 0.5, 0.5]], ["cube"]) and big["a7"] == ([[0.5, 0.5, 0.4, 0.4]], [red])
    with pytest.raises(ValueError, match="'images'"):
        quality.crops_from_layouts({"split": "val"})
    for row in doc["images"]:
        del row["predicted_boxes"]
    with pytest.raises(ValueError, match="predicted_boxes"):
        quality.crops_from_layouts(doc, which="pred")
    assert quality.crops_from_layouts(doc)[3] == gt[3]


def test_class_mean_distance_is_the_per_class_formula():
    from canonicalsg2im_amd import quality
    rng = np.random.RandomState(4)
    feats_a, feats_b = rng.randn(30, 8), rng.randn(25, 8) + 0.5
    cat_a, cat_b = rng.randint(0, 4, 30), rng.randint(0, 4, 25)
    cat_a[cat_a == 2] = 0                       # class 2 on side B only
    cat_b[cat_b == 3] = 1                       # class 3 on side A only; class 4 on neither
    C = 5

    def means(feats, cat):
        out, counts = np.full((C, 8), np.nan), np.zeros(C, np.int64)
        for c in range(C):
            counts[c] = (cat == c).sum()
            if counts[c]:
                out[c] = feats[cat == c].mean(0)
        return out, counts

    got = quality.class_mean_distance(*means(feats_a, cat_a), *means(feats_b, cat_b))
    want = {}                                   # evaluation/fid.py:77-93: norm(test_mean - train_mean) ** 2, then the mean
    for c in (0, 1):
        want[c] = np.linalg.norm(feats_b[cat_b == c].mean(0) - feats_a[cat_a == c].mean(0)) ** 2
    assert set(got["per_class"]) == {0, 1} and got["missing"] == [2, 3]
    for c in want:
        assert abs(got["per_class"][c] - want[c]) <= 1e-14 * want[c]
    assert abs(got["mean"] - np.mean(list(want.values()))) <= 1e-14 * got["mean"]
    need = int((cat_b == 0).sum()) + 1          # class 0 now has too few crops on side B
    few = quality.class_mean_distance(*means(feats_a, cat_a), *means(feats_b, cat_b), min_crops=need)
    assert 0 not in few["per_class"] and (0 in few["missing"]) == bool((cat_a == 0).sum() >= need)
    assert set(few["per_class"]) <= {1}
    none = quality.class_mean_distance(np.zeros((2, 8)), [0, 0], np.zeros((2, 8)), [0, 0])
    assert none["per_class"] == {} and none["missing"] == [] and np.isnan(none["mean"])


def test_quality_script_parses_the_new_flags_with_their_defaults():
    from canonicalsg2im_amd.scripts import quality as script
    a = script.build_parser().parse_args(["A", "B", "--fid_weights", "random"])
    assert a.kid is False and (a.kid_subsets, a.kid_subset_size, a.kid_seed) == (100, 1000, 0)
    assert a.object_crops is None and a.layout_boxes == "gt" and a.min_object_size == 0.0 and a.class_min_crops == 1
    b = script.build_parser().parse_args(["A", "B", "--fid_weights", "random", "--kid", "--kid_subsets", "3", "--kid_subset_size",
                                          "6", "--kid_seed", "9", "--object_crops", "l.json", "--layout_boxes", "pred",
                                          "--min_object_size", "0.02", "--class_min_crops", "4"])
    assert b.kid is True and (b.kid_subsets, b.kid_subset_size, b.kid_seed) == (3, 6, 9)
    assert b.object_crops == "l.json" and b.layout_boxes == "pred" and b.min_object_size == 0.02 and b.class_min_crops == 4


def test_quality_script_refuses_the_new_flags_for_statistics_files():
    from canonicalsg2im_amd.scripts import quality as script
    with pytest.raises(SystemExit, match=r"--kid needs pictures: stats_A\.npz holds statistics"):
        script.main(["stats_A.npz", "B", "--fid_weights", "random", "--kid"])
    with pytest.raises(SystemExit, match=r"--kid and --object_crops need pictures: .*stats_B\.npz"):
        script.main(["A", "dir/stats_B.npz", "--fid_weights", "random", "--kid", "--object_crops", "l.json"])
    args = script.build_parser().parse_args(["stats_A.npz", "B", "--fid_weights", "random"])
    script.refuse_statistics_files(args)                    # without the new flags an .npz is served as before


def test_kid_and_object_fid_refuse_bad_operands_on_the_host():
    from canonicalsg2im_amd import ops, quality
    import torch
    with pytest.raises(ValueError, match="at least 2 rows"):
        quality.kid_from_features(torch.zeros(1, 64), torch.zeros(5, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.crop_windows(torch.zeros(2, 4), 9, 13)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.kid_sums(torch.zeros(4, 64), torch.zeros(4, 64), torch.zeros(1, 2, dtype=torch.int32),
                     torch.zeros(1, 2, dtype=torch.int32), 1.0 / 64)
