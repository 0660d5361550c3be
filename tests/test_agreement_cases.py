"""The restatement of relation agreement (tests/agreement_cases.py) against the reference's own verdicts, and the coverage
of the case table the device is held to (tests/test_gpu_agreement.py).  CPU only; every comparison is exact."""
import numpy as np
import pytest

import agreement_cases as ac
from conftest import load_golden


@pytest.fixture(scope="module")
def golden():
    meta, z = load_golden("clevr_syn")
    return meta, {k: v.numpy() for k, v in z.items()}


def _candidates(n, table):
    """Every (s, p, o), s != o, over the six location predicates: (1, n (n-1) 6, 3)."""
    rows = [(s, table[name], o) for s in range(n) for o in range(n) if s != o for name in ac.NAMES[2:]]
    return np.asarray(rows, np.int64)[None]


@pytest.mark.parametrize("own", [False, True], ids=["boxcentres", "centers"])
def test_restatement_equals_the_reference_verdict_on_perturbed_boxes(golden, own):
    """Part (c) of the golden file: the reference's pair rule on boxes that are not the ground truth.  A candidate triplet
    agrees exactly when the reference lists it."""
    meta, z = golden
    table = meta["pred_name_to_idx"]
    assert [table[n] for n in ac.NAMES] == list(range(8))
    listed = agreeing = 0
    for key in meta["verdicts"]:
        boxes, centers, holds = z[key + "boxes"][None], z[key + "centers"][None], z[key + "holds"].astype(np.int64)
        cand = _candidates(boxes.shape[1], table)
        tested, agrees, per, totals = ac.restate(boxes, centers if own else None, cand, np.zeros(cand.shape[:2], np.int64), table)
        assert tested.all()
        want = {tuple(r) for r in holds.tolist()}
        got = {tuple(r) for r in cand[0][agrees[0] == 1].tolist()}
        assert got == want, (key, sorted(got ^ want)[:5])
        assert per[0, 0].tolist() == [len(want), cand.shape[1]] and int(totals[0, :, 0].sum()) == len(want)
        listed += len(want)
        agreeing += int(agrees.sum())
    assert listed == agreeing > 3000


def test_ground_truth_layouts_obey_their_own_original_triplets(golden):
    """Part (b): the reference's batches.  With a batch's own boxes and centres every tested triplet of type 0 agrees."""
    meta, z = golden
    table = meta["pred_name_to_idx"]
    seen = 0
    for run in meta["runs"]:
        if run.get("getitem"):
            continue
        for lt in (0, 1):
            pre = "%s_lt%d_" % (run["key"], lt)
            tested, agrees, per, _ = ac.restate(z[pre + "boxes"], z[pre + "centers"], z[pre + "triplets"].astype(np.int64),
                                                z[pre + "triplet_type"].astype(np.int64), table)
            assert (per[:, 0, 0] == per[:, 0, 1]).all() and per[:, 0, 1].min() > 0
            assert (per[:, 2:] == 0).all() and ((per[:, 1, 1] > 0).any() == bool(lt))
            seen += int(per[:, 0, 1].sum())
    assert seen > 500


def test_case_table_covers_what_it_says():
    assert len(ac.CASES) == 40 and len({ac.case_id(c) for c in ac.CASES}) == 40
    assert {c[0] for c in ac.CASES} == {1, 3} and {c[1] for c in ac.CASES} == {1, 63, 64, 65, 257} and {c[2] for c in ac.CASES} == {2, 31}
    by_pred = {n: np.zeros(2, np.int64) for n in ac.NAMES}
    by_type = np.zeros((4, 2), np.int64)
    nan_rows = outside = ties = 0
    for case in ac.CASES:
        boxes, centers, triplets, ttype, table = ac.make_case(case)
        assert boxes.dtype == np.float32 and triplets.dtype == np.int64 and ttype.dtype == np.int64
        assert (centers is not None) == case[3] and tuple(triplets.shape) == (case[0], case[1], 3)
        tested, agrees, per, totals = ac.restate(boxes, centers, triplets, ttype, table)
        assert (agrees <= tested).all() and per[..., 1].sum() == tested.sum() == totals[..., 1].sum()
        assert per[..., 0].sum() == agrees.sum() == totals[..., 0].sum()
        for n in ac.NAMES:
            by_pred[n] += totals[:, table[n]].sum(0)
        other = [i for n, i in table.items() if n not in ac.NAMES]
        assert totals[:, other].sum() == 0
        by_type += totals.sum(1)
        s, o = triplets[..., 0], triplets[..., 2]
        pair_nan = np.isnan(np.take_along_axis(boxes.sum(-1), s, 1)) | np.isnan(np.take_along_axis(boxes.sum(-1), o, 1))
        nan_rows += int((tested.astype(bool) & pair_nan).sum())
        assert not (agrees.astype(bool) & pair_nan).any()
        outside += int(((boxes < 0) | (boxes > 1)).any())
        bx = ac.clamp01(boxes)
        same_x0 = np.take_along_axis(bx[..., 0], s, 1) == np.take_along_axis(bx[..., 0], o, 1)
        ties += int((tested.astype(bool) & same_x0 & (s != o)).sum())
    for n in ac.NAMES[:2]:
        assert by_pred[n].tolist() == [0, 0]                     # __padding__ and __in_image__ rows are there, never tested
    for n in ac.NAMES[2:]:
        assert by_pred[n][1] > by_pred[n][0] > 0, (n, by_pred[n])        # every location predicate agrees and disagrees
    assert (by_type[:, 1] > by_type[:, 0]).all() and (by_type[:, 0] > 0).all()
    assert nan_rows > 50 and outside >= 20 and ties > 50        # every O = 31 case holds a box outside [0,1]


def test_restatement_on_hand_made_pairs():
    """The rule's corners, by hand: nested both ways, ties, the clamp, a NaN, rows that are not tested."""
    t = ac.PACKED
    boxes = np.asarray([[[0.125, 0.125, 0.75, 0.75], [0.25, 0.25, 0.25, 0.25], [0.25, 0.5, 0.25, 0.25],
                         [-0.5, 0.0, 1.0, 0.5], [0.0, 0.0, float("nan"), 0.5]]], np.float32)
    rows = [(0, "__surrounding__", 1, 1), (1, "__inside__", 0, 1), (0, "__right of__", 1, 0), (1, "__surrounding__", 0, 0),
            (1, "__above__", 2, 1), (2, "__below__", 1, 1), (1, "__left of__", 2, 0), (1, "__right of__", 2, 0),    # x tie
            (3, "__left of__", 1, 0),            # clamped: (0, 0, 1, .5) has its centre at .5, right of .375
            (3, "__right of__", 1, 1), (4, "__above__", 2, 0), (2, "__below__", 4, 0),                                # NaN pair
            (1, "__in_image__", 0, None), (0, "__padding__", 0, None), (1, "__above__", 1, 0)]
    trip = np.asarray([[(s, t[p], o) for s, p, o, _ in rows]], np.int64)
    ttype = np.asarray([[k % 4 for k in range(len(rows))]], np.int64)
    tested, agrees, per, totals = ac.restate(boxes, None, trip, ttype, t)
    assert tested[0].tolist() == [0 if want is None else 1 for *_, want in rows]
    assert agrees[0].tolist() == [want or 0 for *_, want in rows]
    assert per.sum(1)[0].tolist() == [5, 13] and totals.sum((0, 1)).tolist() == [5, 13]
    # rows the device cannot dereference: an object outside [0, O), a type outside [0, 4) — not tested
    bad = np.asarray([[(5, t["__above__"], 0), (0, t["__above__"], -1), (1, t["__above__"], 2)]], np.int64)
    tested, agrees, _, _ = ac.restate(boxes, None, bad, np.asarray([[0, 0, 4]], np.int64), t)
    assert tested.tolist() == [[0, 0, 0]] and agrees.tolist() == [[0, 0, 0]]
