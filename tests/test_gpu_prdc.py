"""Device tests of the k-nearest-neighbour manifold metrics (csrc/manifold.hip, ops.knn_radii / ops.ball_counts,
quality.prdc_from_features / quality.PRDC, scripts.quality --prdc) against the restatement of tests/prdc_cases.py.  The
outputs are a k-th smallest fp64 distance and integer counts: on integer-valued features they must EQUAL the restatement,
ties included; on random fp32 rows the radii may differ by rounding (prdc_cases.radius_bound) and the counts must be equal
because no pair is within rounding of a sphere (tests/test_prdc_cases.py asserts that of the same inputs).  The network is
the seeded stand-in throughout; no other precision / recall implementation has been compared with."""
import functools
import json

import numpy as np
import pytest
import torch

import prdc_cases as pc
import quality_cases as qc

pytestmark = pytest.mark.gpu

SIDE = (75, 75)            # as test_gpu_quality_objects.py: the stand-in network at 75 x 75 takes milliseconds


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def stand_in_net():
    from canonicalsg2im_amd import inception
    return inception.InceptionV3("fid", "random").to("cuda:0")


def _radii(f_dev, k):
    """ops.knn_radii, called twice: the same bits."""
    from canonicalsg2im_amd import ops
    r2 = ops.knn_radii(f_dev, k)
    assert r2.dtype == torch.float64 and tuple(r2.shape) == (f_dev.shape[0],)
    assert torch.equal(r2.view(torch.int64), ops.knn_radii(f_dev, k).view(torch.int64))
    return r2


def _counts(q_dev, f_dev, r2_dev):
    from canonicalsg2im_amd import ops
    inside, holds = ops.ball_counts(q_dev, f_dev, r2_dev)
    assert inside.dtype == torch.int32 and holds.dtype == torch.int32
    assert tuple(inside.shape) == (q_dev.shape[0],) and tuple(holds.shape) == (f_dev.shape[0],)
    again = ops.ball_counts(q_dev, f_dev, r2_dev)
    assert torch.equal(inside, again[0]) and torch.equal(holds, again[1])
    return inside.cpu().numpy(), holds.cpu().numpy()


def _check_exact(cuda, real, gen, k, what):
    """Both directions of one table row, device against restatement, to equality."""
    for f, q, side in ((real, gen, "real"), (gen, real, "generated")):
        if f.shape[0] < k + 1:
            continue                                               # the generated side of a row with few queries has no radii
        f_dev, q_dev = torch.from_numpy(f).to(cuda), torch.from_numpy(q).to(cuda)
        r2 = _radii(f_dev, k)
        want_r2 = pc.radii_ref(f, k)
        assert np.array_equal(r2.cpu().numpy(), want_r2), (what, side, "radii")
        inside, holds = _counts(q_dev, f_dev, r2)
        want_inside, want_holds = pc.counts_ref(q, f, want_r2)
        assert np.array_equal(inside, want_inside), (what, side, "inside")
        assert np.array_equal(holds, want_holds), (what, side, "holds")
        assert int(inside.sum()) == int(holds.sum())


# ------------------------------------------------------------------------------------------------ the table through ops
def test_hand_worked_row(cuda):
    real, gen = pc.line_points(pc.HAND_REAL_X), pc.line_points(pc.HAND_GEN_X)
    real_dev, gen_dev = torch.from_numpy(real).to(cuda), torch.from_numpy(gen).to(cuda)
    r2_real, r2_gen = _radii(real_dev, pc.HAND_K), _radii(gen_dev, pc.HAND_K)
    assert r2_real.tolist() == pc.HAND["r2_real"] and r2_gen.tolist() == pc.HAND["r2_gen"]
    inside, holds = _counts(gen_dev, real_dev, r2_real)
    assert inside.tolist() == pc.HAND["inside_gen"] and holds.tolist() == pc.HAND["holds_real"]      # 3 ON the sphere of 2
    inside_r, _ = _counts(real_dev, gen_dev, r2_gen)
    assert inside_r.tolist() == pc.HAND["inside_real"]


@pytest.mark.parametrize("case", pc.GRID_CASES, ids=[c[0] for c in pc.GRID_CASES])
def test_integer_grid_rows_equal_the_restatement(cuda, case):
    name, n, m, D, k, ties = case
    real, gen, k = pc.grid_case(n, m, D, k, ties=ties)
    _check_exact(cuda, real, gen, k, name)


@pytest.fixture(scope="module")
def boundaries():
    from canonicalsg2im_amd import _lib
    return pc.chunk_boundaries(lambda r, c: int(_lib.lib.csg_manifold_column_chunks(r, c)))


@pytest.mark.parametrize("which", range(14))
def test_each_side_of_every_chunk_boundary(cuda, boundaries, which):
    """One n on each side of every n below 1024 at which csg_manifold_column_chunks(n, n) changes (seven of them:
    tests/test_prdc_cases.py), as the real rows against 67 generated ones and the other way round."""
    assert len(boundaries) == 7, boundaries
    n = boundaries[which // 2] + which % 2
    real, gen, k = pc.grid_case(n, 67, 64, 3)
    _check_exact(cuda, real, gen, k, "n = %d" % n)


@pytest.mark.parametrize("case", pc.ROW_GROUP_CASES, ids=["m%d" % c[0] for c in pc.ROW_GROUP_CASES])
def test_ball_counts_when_a_block_walks_several_query_tiles(cuda, case):
    """csg_ball_counts above m = 4096: more query tiles than its 64 row groups, so a block accumulates `holds` over several
    tiles in the workspace and closes `inside` once per tile.  Both ways round: many queries against few centres, and few
    queries against many centres (three row groups, 33 chunks of centres)."""
    for m, n in (case, case[::-1]):
        q, f, r2 = pc.row_group_case(m, n)
        inside, holds = _counts(torch.from_numpy(q).to(cuda), torch.from_numpy(f).to(cuda), torch.from_numpy(r2).to(cuda))
        want_inside, want_holds = pc.counts_ref(q, f, r2)
        assert np.array_equal(inside, want_inside), (m, n, "inside")
        assert np.array_equal(holds, want_holds), (m, n, "holds")
        assert 0 < int(holds.sum()) < m * n


def test_rows_behind_a_view_are_never_read(cuda):
    f_big, q_big, n, m = pc.masked_operands(*pc.MASK_CASE)
    k = pc.MASK_CASE[3]
    f_dev, q_dev = torch.from_numpy(f_big).to(cuda)[:n], torch.from_numpy(q_big).to(cuda)[:m]
    assert f_dev.is_contiguous() and q_dev.is_contiguous()
    want_r2 = pc.radii_ref(f_big[:n], k)
    r2 = _radii(f_dev, k)
    assert np.array_equal(r2.cpu().numpy(), want_r2)
    inside, holds = _counts(q_dev, f_dev, r2)
    want_inside, want_holds = pc.counts_ref(q_big[:m], f_big[:n], want_r2)
    assert np.array_equal(inside, want_inside) and np.array_equal(holds, want_holds)
    r2_q = _radii(q_dev, k)
    assert np.array_equal(r2_q.cpu().numpy(), pc.radii_ref(q_big[:m], k))
    inside_r, holds_r = _counts(f_dev, q_dev, r2_q)
    want = pc.counts_ref(f_big[:n], q_big[:m], pc.radii_ref(q_big[:m], k))
    assert np.array_equal(inside_r, want[0]) and np.array_equal(holds_r, want[1])


@pytest.mark.parametrize("case", pc.RANDOM_CASES)
def test_random_rows(cuda, case):
    n, m, D, k, seed = case
    real, gen, k = pc.random_case(*case)
    for f, q in ((real, gen), (gen, real)):
        f_dev, q_dev = torch.from_numpy(f).to(cuda), torch.from_numpy(q).to(cuda)
        r2 = _radii(f_dev, k)
        want_r2 = pc.radii_ref(f, k)
        err = float((np.abs(r2.cpu().numpy() - want_r2) / want_r2).max())
        print("random case %s: largest relative error of a radius %.2e (bound %.2e)" % (case, err, pc.radius_bound(D)))
        assert err <= pc.radius_bound(D)
        d = pc.d2_ref(q, f)
        decided = np.ones(d.shape, bool)
        for j, i in pc.undecided_pairs(d, want_r2, D):
            decided[j, i] = False
        assert decided.all()                                       # the share of undecided pairs allowed is zero
        inside, holds = _counts(q_dev, f_dev, r2)
        want_inside, want_holds = pc.counts_ref(q, f, want_r2, d=d)
        assert np.array_equal(inside, want_inside) and np.array_equal(holds, want_holds)


def test_nonfinite_rows_at_the_abi(cuda):
    bad, clean, gen, k = pc.nonfinite_case()
    rows = list(pc.NONFINITE_ROWS)
    keep = [i for i in range(len(bad)) if i not in rows]
    bad_dev, gen_dev = torch.from_numpy(bad).to(cuda), torch.from_numpy(gen).to(cuda)
    r2 = _radii(bad_dev, k)
    got = r2.cpu().numpy()
    assert np.isposinf(got[rows]).all()
    assert np.array_equal(got[keep], _radii(torch.from_numpy(clean).to(cuda), k).cpu().numpy())      # the others: unchanged
    assert np.array_equal(got, pc.radii_ref(bad, k))
    inside, holds = _counts(gen_dev, bad_dev, r2)
    want_inside, want_holds = pc.counts_ref(gen, bad, got)
    assert np.array_equal(inside, want_inside) and np.array_equal(holds, want_holds) and (holds[rows] == 0).all()
    inside_r, _ = _counts(bad_dev, gen_dev, _radii(gen_dev, k))
    assert (inside_r[rows] == 0).all()                             # inside nothing
    assert np.array_equal(inside_r, pc.counts_ref(bad, gen, pc.radii_ref(gen, k))[0])
    # a NaN radius holds nothing
    r2_nan = r2.clone()
    r2_nan[0] = float("nan")
    assert _counts(gen_dev, bad_dev, r2_nan)[1][0] == 0
    from canonicalsg2im_amd import quality
    with pytest.raises(ValueError, match="PRDC: the real features hold a NaN or an infinity"):
        quality.prdc_from_features(bad_dev, gen_dev, k)
    with pytest.raises(ValueError, match="PRDC: the generated features hold a NaN or an infinity"):
        quality.prdc_from_features(gen_dev, bad_dev, k)
    for value in (float("nan"), float("-inf")):
        spoiled = gen_dev.clone()
        spoiled[3, 5] = value
        with pytest.raises(ValueError, match="PRDC: the generated features hold a NaN or an infinity"):
            quality.prdc_from_features(torch.from_numpy(clean).to(cuda), spoiled, k)


def test_entries_refuse_with_their_messages(cuda):
    from canonicalsg2im_amd import ops
    f = torch.zeros(8, 64, device=cuda)
    for k, message in ((8, r"csg_knn_radii: n=8 rows for k=8"), (9, r"csg_knn_radii: n=8 rows for k=9"),
                       (0, r"csg_knn_radii: k=0 \(served: 1 \.\. 16\)"), (17, r"csg_knn_radii: k=17 \(served: 1 \.\. 16\)")):
        with pytest.raises(RuntimeError, match=message):
            ops.knn_radii(f, k)
    wide = torch.zeros(40, 96, device=cuda)
    with pytest.raises(RuntimeError, match=r"csg_knn_radii: D=96 \(a multiple of 64"):
        ops.knn_radii(wide, 3)
    with pytest.raises(RuntimeError, match=r"csg_ball_counts: D=96 \(a multiple of 64"):
        ops.ball_counts(wide, wide, torch.zeros(40, device=cuda, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="queries and centres must be"):
        ops.ball_counts(f, torch.zeros(8, 128, device=cuda), torch.zeros(8, device=cuda, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"r2 must be \(n,\) = \(8,\)"):
        ops.ball_counts(f, f, torch.zeros(7, device=cuda, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ball_counts: f must be a dense float32 tensor"):
        ops.ball_counts(f, torch.zeros(8, 128, device=cuda)[:, ::2], torch.zeros(8, device=cuda, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="compute in fp32"):
        ops.ball_counts(f, f.half(), torch.zeros(8, device=cuda, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ball_counts: r2 must be a dense float64 tensor"):
        ops.ball_counts(f, f, torch.zeros(8, device=cuda))
    with pytest.raises(RuntimeError, match="forward only"):
        ops.knn_radii(torch.zeros(8, 64, device=cuda, requires_grad=True), 3)


# ------------------------------------------------------------------------------------------------ quality.py
def _four(out):
    return {name: out[name] for name in ("precision", "recall", "density", "coverage")}


@pytest.mark.parametrize("row", ["ties", "uneven", "random0", "random1", "random2"])
def test_prdc_from_features_equals_the_restatement(cuda, row):
    from canonicalsg2im_amd import quality
    if row.startswith("random"):
        real, gen, k = pc.random_case(*pc.RANDOM_CASES[int(row[-1])])
    else:
        name, n, m, D, k, ties = [c for c in pc.GRID_CASES if c[0] == row][0]
        real, gen, k = pc.grid_case(n, m, D, k, ties=ties)
    real_dev, gen_dev = torch.from_numpy(real).to(cuda), torch.from_numpy(gen).to(cuda)
    got = quality.prdc_from_features(real_dev, gen_dev, k)
    want = pc.prdc_ref(real, gen, k)
    print("prdc %s: %s" % (row, got))
    assert got == want                                             # integers divided the same way: equal floats
    assert set(got) == {"precision", "recall", "density", "coverage", "k", "n"}
    turned = quality.prdc_from_features(gen_dev, real_dev, k)      # real and generated swapped: precision <-> recall
    assert turned["precision"] == got["recall"] and turned["recall"] == got["precision"] and turned["n"] == got["n"][::-1]
    if row == "random1":                                           # strictly inside (0, 1): a constant would not pass
        assert all(0.0 < got[name] < 1.0 for name in ("precision", "recall", "coverage"))


def test_prdc_of_the_hand_worked_row(cuda):
    from canonicalsg2im_amd import quality
    real, gen = pc.line_points(pc.HAND_REAL_X), pc.line_points(pc.HAND_GEN_X)
    got = quality.prdc_from_features(torch.from_numpy(real).to(cuda), torch.from_numpy(gen).to(cuda), k=1)
    assert _four(got) == {name: pc.HAND[name] for name in ("precision", "recall", "density", "coverage")}
    assert got["k"] == 1 and got["n"] == [4, 3]
    with pytest.raises(ValueError, match=r"k = 3 needs 1 <= k < min\(n_real, n_gen\) = 3"):
        quality.prdc_from_features(torch.from_numpy(real).to(cuda), torch.from_numpy(gen).to(cuda), k=3)


def test_prdc_class_fed_in_two_calls_equals_one_call(cuda):
    from canonicalsg2im_amd import quality
    net = stand_in_net()
    sets = [torch.from_numpy(qc.pictures(7, 64, seed=41)).to(cuda), torch.from_numpy(qc.pictures(9, 64, seed=42)).to(cuda)]
    fid = quality.FID(net, dims=192, size=SIDE)
    two = quality.PRDC(net, dims=192, size=SIDE, k=2)
    for which, pics in enumerate(sets):
        two.update(pics[:4], which)
        two.update(pics[4:], which)
    got = two.compute()
    feats = [torch.cat([fid.features(pics[:4]), fid.features(pics[4:])]) for pics in sets]
    want = quality.prdc_from_features(feats[0], feats[1], k=2)
    assert got["stand_in"] is True and {k: v for k, v in got.items() if k != "stand_in"} == want
    assert two.n == [7, 9] and got["n"] == [7, 9] and got["k"] == 2
    whole = quality.PRDC(net, dims=192, size=SIDE, k=2)            # one update(images) per side
    for which, pics in enumerate(sets):
        whole.update(pics, which)
    assert whole.n == [7, 9] and whole.compute() == got
    one = quality.PRDC(net, dims=192, size=SIDE, k=2)              # the same rows in one call per side
    for which in (0, 1):
        one.update_features(feats[which], which)
    assert one.compute() == got
    halves = quality.PRDC(net, dims=192, size=SIDE, k=2)
    for which in (0, 1):
        halves.update_features(feats[which][:3], which)
        halves.update_features(feats[which][3:], which)
    assert halves.compute() == got
    one.clean()
    assert one.n == [0, 0]
    with pytest.raises(ValueError, match="k = 2 needs more than k pictures per side, got 2 and 9"):
        one.update_features(feats[0][:2], 0)
        one.update_features(feats[1], 1)
        one.compute()
    with pytest.raises(ValueError, match="which must be 0"):
        one.update_features(feats[0], 2)


# ------------------------------------------------------------------------------------------------ scripts.quality
def test_quality_script_with_prdc(cuda, tmp_path, capsys):
    from PIL import Image
    from canonicalsg2im_amd import quality
    from canonicalsg2im_amd.inception import InceptionV3
    from canonicalsg2im_amd.scripts import quality as script
    rng = np.random.RandomState(9)
    names = ["cube", "sphere", "cylinder"]
    sets, folders, rows = [], [], []
    for i in range(8):
        n = 2 + i % 2
        rows.append({"image_id": 100 + i, "objects": [names[(i + k) % 3] for k in range(n)],
                     "gt_boxes": np.concatenate([rng.uniform(0, 0.5, (n, 2)), rng.uniform(0.2, 0.5, (n, 2))], axis=1).tolist()})
    for k in range(2):
        d = tmp_path / ("set%d" % k)
        d.mkdir()
        sets.append(qc.pictures(8, 75, seed=60 + k))
        for i, pic in enumerate(sets[-1]):
            Image.fromarray(pic).save(str(d / ("%d.png" % (100 + i))))
        folders.append(str(d))
    layouts = tmp_path / "layouts.json"
    layouts.write_text(json.dumps({"split": "val", "images": rows}))
    out = tmp_path / "out"
    common = ["--fid_weights", "random", "--dims", "64", "--batch-size", "4", "--output_dir", str(out),
              "--kid", "--kid_subsets", "3", "--kid_subset_size", "6", "--object_crops", str(layouts)]
    before = script.main(folders + common)
    capsys.readouterr()
    res = script.main(folders + common + ["--prdc", "--prdc_k", "2"])
    text = capsys.readouterr().out
    for line in ("Precision:", "Recall:", "Density:", "Coverage:", "PRDC:", "ScenePrecision:", "SceneRecall:", "SceneDensity:",
                 "SceneCoverage:", "ScenePRDC:"):
        hit = [l for l in text.splitlines() if l.startswith(line)]
        assert len(hit) == 1 and "stand-in" in hit[0], (line, text)
    assert "real = folder A" in [l for l in text.splitlines() if l.startswith("PRDC:")][0]
    saved = json.load(open(str(out / "quality.json")))
    assert saved == json.loads(json.dumps(res))
    # FID, KID and the objects of the same run are what they are without --prdc
    assert set(res) == set(before) | {"prdc"} and set(res["objects"]) == set(before["objects"]) | {"prdc"}
    assert all(res[key] == before[key] for key in before if key != "objects")
    assert all(res["objects"][key] == before["objects"][key] for key in before["objects"])
    keys = {"precision", "recall", "density", "coverage", "k", "n", "real", "stand_in"}
    assert set(res["prdc"]) == keys and set(res["objects"]["prdc"]) == keys
    assert res["prdc"]["stand_in"] and res["prdc"]["real"] == "A" and res["prdc"]["k"] == 2 and res["prdc"]["n"] == [8, 8]
    # the API on the same files, called as the script calls it (bgr, 4 pictures per update)
    net = InceptionV3("fid", "random").to(cuda)
    crops = quality.crops_from_layouts({"images": rows})
    classes = sorted({key for _, keys_ in crops.values() for key in keys_})
    fid = quality.FID(net, dims=64, channel_order="bgr")
    feats, crop_feats = [], []
    for pics in sets:
        ofid = quality.ObjectFID(net, dims=64, channel_order="bgr", batch_size=4, classes=classes)
        part, crop_part = [], []
        for i in (0, 4):
            dev_pics = torch.from_numpy(pics[i:i + 4]).to(cuda)
            part.append(fid.features(dev_pics))
            boxes = [b for r in rows[i:i + 4] for b in r["gt_boxes"]]
            index = [k for k, r in enumerate(rows[i:i + 4]) for _ in r["objects"]]
            ids = [classes.index(key) for r in rows[i:i + 4] for key in crops[r["image_id"]][1]]
            crop_part.append(ofid.update(dev_pics, boxes, index, ids))
        feats.append(torch.cat(part))
        crop_feats.append(torch.cat(crop_part))
    want = quality.prdc_from_features(feats[0], feats[1], 2)
    assert {k: v for k, v in res["prdc"].items() if k not in ("real", "stand_in")} == want
    n_crops = sum(len(r["objects"]) for r in rows)
    want = quality.prdc_from_features(crop_feats[0], crop_feats[1], 2)
    assert {k: v for k, v in res["objects"]["prdc"].items() if k not in ("real", "stand_in")} == want
    assert want["n"] == [n_crops, n_crops]
    # --prdc_real B: the other folder is the real one
    plain = ["--fid_weights", "random", "--dims", "64", "--batch-size", "4", "--output_dir", str(out)]
    turned = script.main(folders + plain + ["--prdc", "--prdc_k", "2", "--prdc_real", "B"])
    text = capsys.readouterr().out
    assert "real = folder B" in [l for l in text.splitlines() if l.startswith("PRDC:")][0]
    assert turned["prdc"]["real"] == "B" and turned["fid"] == res["fid"]
    assert turned["prdc"]["precision"] == res["prdc"]["recall"] and turned["prdc"]["recall"] == res["prdc"]["precision"]
    assert turned["prdc"] == dict(quality.prdc_from_features(feats[1], feats[0], 2), real="B", stand_in=True)
    with pytest.raises(SystemExit, match=r"--prdc: PRDC: k = 8 needs 1 <= k < min"):
        script.main(folders + plain + ["--prdc", "--prdc_k", "8"])
