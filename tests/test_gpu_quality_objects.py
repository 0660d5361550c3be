"""Device tests of KID and the object-level FID (csrc/quality.hip, canonicalsg2im_amd/quality.py, scripts/quality.py) against
the restatements of tests/quality_cases.py.  The network is the seeded stand-in throughout: the real weight files have never
been loaded, and no other KID or SceneFID implementation has been compared with."""
import functools
import json

import numpy as np
import pytest
import torch

import quality_cases as qc

pytestmark = pytest.mark.gpu

SIDE = (75, 75)            # as the end-to-end tests of test_gpu_inception.py: the stand-in network at 75 x 75 takes milliseconds


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def stand_in_net():
    from canonicalsg2im_amd import inception
    return inception.InceptionV3("fid", "random").to("cuda:0")


# ------------------------------------------------------------------------------------------------ windows
def test_crop_windows_equals_the_restatement_for_every_row(cuda):
    from canonicalsg2im_amd import ops
    got = ops.crop_windows(torch.from_numpy(qc.BOXES).to(cuda), qc.H, qc.W).cpu().numpy()
    want = qc.windows_ref(qc.BOXES, qc.H, qc.W)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got.tolist(), want.tolist())
    assert np.array_equal(got, qc.HAND_WINDOWS)
    tail = got[qc.N_FINITE:]                                    # NaN, +-inf, 1e30: inside the picture, at least one pixel
    assert (tail[:, :2] >= 0).all() and (tail[:, 2] <= qc.W).all() and (tail[:, 3] <= qc.H).all()
    assert (tail[:, 2] > tail[:, 0]).all() and (tail[:, 3] > tail[:, 1]).all()
    # another picture size, more than one block of rows
    rng = np.random.RandomState(5)
    boxes = np.concatenate([rng.uniform(-0.2, 0.9, (700, 2)), rng.uniform(0.0, 0.6, (700, 2))], axis=1).astype(np.float32)
    got = ops.crop_windows(torch.from_numpy(boxes).to(cuda), 64, 48).cpu().numpy()
    assert np.array_equal(got, qc.windows_ref(boxes, 64, 48))


# ------------------------------------------------------------------------------------------------ crop + resize
@pytest.fixture(scope="module")
def crop_inputs(cuda):
    pics = qc.crop_pictures()
    windows = qc.windows_ref(qc.BOXES[:qc.N_FINITE], qc.H, qc.W)          # the finite rows only
    return pics, windows, torch.from_numpy(pics).to(cuda), torch.from_numpy(windows).to(cuda), \
        torch.from_numpy(qc.IMAGE_INDEX).to(cuda)


def _check_crops(ops, cuda, crop_inputs, rows, size, a, b, rev):
    pics, windows, pics_dev, win_dev, idx_dev = crop_inputs
    sel = torch.tensor(rows, device=cuda)
    got = ops.crop_resize_bilinear(pics_dev, win_dev[sel].contiguous(), idx_dev[sel].contiguous(), size, a, b, reverse=rev).cpu()
    assert tuple(got.shape) == (len(rows), 4) + tuple(size) and bool((got[:, 3] == 0).all())
    worst = 0.0
    for k, n in enumerate(rows):
        window = qc.cut(pics, windows[n], qc.IMAGE_INDEX[n])
        alone = ops.resize_bilinear(torch.from_numpy(window[None]).to(cuda), size, a, b, reverse=rev).cpu()
        assert torch.equal(got[k], alone[0]), "row %d (%s) size %s a=%g rev=%d: not resize_bilinear's bits" % (
            n, qc.WINDOW_ROWS[n][0], size, a, rev)
        err = float((got[k, :3].double() - qc.interpolate64(window, size, a, b, rev)).abs().max())
        worst = max(worst, err)
        assert err <= abs(a) * 2 * 2.0 ** -15 + 1e-6, (n, size, err)
        if tuple(window.shape[:2]) == tuple(size):              # the identity: bytes / 255 * a + b, bit for bit
            want = torch.from_numpy(window).float().permute(2, 0, 1) / 255.0
            want = (want.flip(0) if rev else want) * a + b
            assert torch.equal(got[k, :3], want), (n, size)
        # a one-pixel window at (4, 4): the weights are multiples of 1/8 and w0 * v + w1 * v rounds back to v — a constant
        # crop.  (At other sizes the two clamped taps still carry weights like 1/18 and 17/18, and the sum is v to an ulp,
        # as it is in resize_bilinear and in torch: the equality above covers those.)
        if tuple(window.shape[:2]) == (1, 1) and tuple(size) == (4, 4):
            assert bool((got[k, :3] == got[k, :3, :1, :1]).all()), (n, size)
    print("crop_resize %s a=%g rev=%d: %d rows, max err vs fp64 %.2e (bound %.2e)" % (
        size, a, rev, len(rows), worst, abs(a) * 2 * 2.0 ** -15 + 1e-6))


@pytest.mark.parametrize("size", qc.CROP_SIZES)
def test_crop_resize_bilinear_is_resize_bilinear_of_the_window(cuda, crop_inputs, size):
    from canonicalsg2im_amd import ops
    rows = list(range(qc.N_FINITE))
    if size == (qc.H, qc.W):
        assert qc.HAND_WINDOWS[0].tolist() == [0, 0, qc.W, qc.H]              # the identity row is among them
    if size == (4, 4):
        assert qc.HAND_WINDOWS[1].tolist() == [0, 0, 1, 1]                    # and the one-pixel window
    for a, b, rev in qc.AFFINES:
        _check_crops(ops, cuda, crop_inputs, rows, size, a, b, rev)


def test_crop_resize_bilinear_at_the_networks_size(cuda, crop_inputs):
    from canonicalsg2im_amd import ops
    for a, b, rev in qc.AFFINES:
        _check_crops(ops, cuda, crop_inputs, qc.CROP_ROWS_299, (299, 299), a, b, rev)


# ------------------------------------------------------------------------------------------------ KID sums
def _kid_case(cuda, case, degree=3, signed=False):
    from canonicalsg2im_amd import ops
    nx, ny, m, D, S = case
    fx, fy = qc.kid_features(nx, ny, D, signed=signed)
    ix, iy = qc.draw_subsets(nx, ny, m, S)
    gamma = 1.0 / D
    dev = [torch.from_numpy(t).to(cuda) for t in (fx, fy, ix, iy)]
    got = ops.kid_sums(*dev, gamma, 1.0, degree)
    assert got.dtype == torch.float64 and tuple(got.shape) == (S, 3)
    again = ops.kid_sums(*dev, gamma, 1.0, degree)
    assert torch.equal(got, again), "two calls differ"
    got = got.cpu().numpy()
    want, mags = qc.kid_sums_ref(fx, fy, ix, iy, gamma, 1.0, degree)
    tol, tol_mmd = qc.kid_tolerances(mags, m, D)
    err = np.abs(got - want)
    err_mmd = np.abs(qc.mmd2(got, m) - qc.mmd2(want, m))
    print("kid_sums %s degree %d%s: max err / bound per sum %s; MMD^2 %s, err %s, bound %s" % (
        case, degree, " signed" if signed else "", (err / tol).max(axis=0), qc.mmd2(want, m), err_mmd, tol_mmd))
    assert (err <= tol).all(), (err, tol)
    assert (err_mmd <= tol_mmd).all(), (err_mmd, tol_mmd)
    if S > 1:                               # the subsets in another order: the same bits per subset
        order = list(range(S))[::-1]
        turned = ops.kid_sums(dev[0], dev[1], torch.from_numpy(ix[order].copy()).to(cuda),
                              torch.from_numpy(iy[order].copy()).to(cuda), gamma, 1.0, degree).cpu().numpy()
        assert np.array_equal(turned, got[order])


@pytest.mark.parametrize("case", qc.KID_CASES)
def test_kid_sums(cuda, case):
    _kid_case(cuda, case)


def test_kid_sums_other_degrees_and_signed_features(cuda):
    _kid_case(cuda, qc.KID_CASES[1], degree=1)
    _kid_case(cuda, qc.KID_CASES[1], degree=2)
    _kid_case(cuda, (70, 90, 63, 64, 3), signed=True)


def test_kid_sums_refuses_a_subset_of_one_row(cuda):
    from canonicalsg2im_amd import ops
    f = torch.zeros(4, 64, device=cuda)
    one = torch.zeros(2, 1, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="csg_kid_sums: a subset needs 2"):
        ops.kid_sums(f, f, one, one, 1.0 / 64)
    with pytest.raises(RuntimeError, match="degree 4"):
        ops.kid_sums(f, f, torch.zeros(2, 2, dtype=torch.int32, device=cuda), torch.zeros(2, 2, dtype=torch.int32, device=cuda),
                     1.0 / 64, 1.0, 4)


# ------------------------------------------------------------------------------------------------ class sums
def test_feat_class_sums_over_two_updates(cuda):
    from canonicalsg2im_amd import ops
    parts = qc.class_case()
    sums = torch.zeros(qc.CLASS_C, qc.CLASS_D, device=cuda, dtype=torch.float64)
    counts = torch.zeros(qc.CLASS_C, device=cuda, dtype=torch.int64)
    for x, ids in parts:
        ops.feat_class_sums(torch.from_numpy(x).to(cuda), torch.from_numpy(ids).to(cuda), sums, counts)
    want, mags, want_counts = qc.class_sums_ref(parts, qc.CLASS_C)
    n = 2 * qc.CLASS_N
    err = np.abs(sums.cpu().numpy() - want)
    print("feat_class_sums: max err %.2e, counts %s" % (err.max(), counts.cpu().tolist()))
    assert (err <= n * 2.0 ** -53 * mags).all()
    assert np.array_equal(counts.cpu().numpy(), want_counts) and want_counts[3] == 0 and want_counts.sum() == n - 4


# ------------------------------------------------------------------------------------------------ wiring
@pytest.fixture(scope="module")
def scene(cuda):
    """6 pictures of 64 x 64 with 4 boxes each, 3 classes."""
    rng = np.random.RandomState(21)
    pics = qc.pictures(6, 64, seed=31)
    xy = rng.uniform(0.0, 0.6, (24, 2))
    wh = rng.uniform(0.15, 0.4, (24, 2))
    boxes = np.concatenate([xy, wh], axis=1).astype(np.float32)
    index = np.repeat(np.arange(6), 4).astype(np.int64)
    ids = rng.randint(0, 3, 24)
    return pics, torch.from_numpy(pics).to(cuda), boxes, index, ids


def test_object_fid_wiring(cuda, scene):
    from canonicalsg2im_amd import ops, quality
    net = stand_in_net()
    pics, pics_dev, boxes, index, ids = scene
    ofid = quality.ObjectFID(net, dims=192, size=SIDE, classes=["a", "b", "c"])
    assert ofid.stand_in
    feats = ofid.features(pics_dev, boxes, index)
    boxes_dev, index_dev = torch.from_numpy(boxes).to(cuda), torch.from_numpy(index).to(cuda).int()
    crops = ops.crop_resize_bilinear(pics_dev, ops.crop_windows(boxes_dev, 64, 64), index_dev, SIDE, 2.0, -1.0)
    assert torch.equal(feats, net(crops, dims=192))                          # bit for bit
    assert torch.equal(feats, ofid.features(pics_dev, boxes_dev, index_dev))  # device operands: the same
    kept = ofid.update(pics_dev, boxes, index, ids)
    assert torch.equal(kept, feats) and ofid.n == 24
    plain = quality.FID(net, dims=192, size=SIDE)
    plain.update_features(feats)
    (mu, sigma), (mu2, sigma2) = ofid.statistics(), plain.statistics()
    assert np.array_equal(mu, mu2) and np.array_equal(sigma, sigma2)
    same = quality.frechet_distance(mu, sigma, mu, sigma)
    print("SceneFID(A, A) = %.3e, tr sigma = %.3e" % (same, np.trace(sigma)))
    assert abs(same) < 1e-6 * np.trace(sigma)
    means, counts = ofid.class_means()
    f64 = feats.double().cpu().numpy()
    for c in range(3):
        assert counts[c] == (ids == c).sum()
        if counts[c]:
            assert np.abs(means[c] - f64[ids == c].mean(0)).max() <= 1e-14 * np.abs(f64).max()
    with pytest.raises(ValueError, match="boxes row 2 is not finite"):
        bad = boxes.copy()
        bad[2, 1] = np.nan
        ofid.update(pics_dev, bad, index)
    with pytest.raises(ValueError, match="image_index row 23 is 6"):
        ofid.update(pics_dev, boxes, np.where(np.arange(24) == 23, 6, index))


def test_object_fid_runs_the_remainder_batch(cuda, scene):
    """24 crops at batch_size 5: batches of 5, 5, 5, 5 and 4.  No crop is dropped, and what reaches the statistics is, bit for
    bit, the network on the same batches of ops.crop_resize_bilinear's output."""
    from canonicalsg2im_amd import ops, quality
    net = stand_in_net()
    pics, pics_dev, boxes, index, ids = scene
    ofid = quality.ObjectFID(net, dims=192, size=SIDE, batch_size=5)
    kept = ofid.update(pics_dev, boxes, index)
    assert ofid.n == 24 and tuple(kept.shape) == (24, 192)
    windows = ops.crop_windows(torch.from_numpy(boxes).to(cuda), 64, 64)
    index_dev = torch.from_numpy(index).to(cuda).int()
    want = torch.cat([net(ops.crop_resize_bilinear(pics_dev, windows[i:i + 5], index_dev[i:i + 5], SIDE, 2.0, -1.0), dims=192)
                      for i in range(0, 24, 5)])
    assert torch.equal(kept, want)
    plain = quality.FID(net, dims=192, size=SIDE)
    for i in range(0, 24, 5):
        plain.update_features(want[i:i + 5])
    for got, ref in zip(ofid.statistics(), plain.statistics()):
        assert np.array_equal(got, ref)


def test_kid_class_equals_kid_from_features(cuda, scene, capsys):
    from canonicalsg2im_amd import quality
    net = stand_in_net()
    sets = [torch.from_numpy(qc.pictures(7, 64, seed=41)).to(cuda), torch.from_numpy(qc.pictures(9, 64, seed=42)).to(cuda)]
    kid = quality.KID(net, dims=192, size=SIDE, subsets=4, subset_size=6)
    fid = quality.FID(net, dims=192, size=SIDE)
    for which, pics in enumerate(sets):
        kid.update(pics[:4], which)
        kid.update(pics[4:], which)
    got = kid.compute()
    feats = [torch.cat([fid.features(pics[:4]), fid.features(pics[4:])]) for pics in sets]
    want = quality.kid_from_features(feats[0], feats[1], subsets=4, subset_size=6)
    assert got["stand_in"] is True and {k: v for k, v in got.items() if k != "stand_in"} == want
    assert got["n"] == [7, 9] and got["subsets"] == 4 and got["subset_size"] == 6 and got["std"] >= 0.0
    capped = quality.kid_from_features(feats[0], feats[1], subsets=2, subset_size=1000)
    assert capped["subset_size"] == 7 and "capped to 7" in capsys.readouterr().out
    # the rule, restated: seed 0 subsets, the fp64 sums, mean and np.std
    f0, f1 = (f.cpu().numpy() for f in feats)
    ix, iy = qc.draw_subsets(7, 9, 6, 4)
    sums, mags = qc.kid_sums_ref(f0, f1, ix, iy, 1.0 / 192, 1.0, 3)
    _, tol = qc.kid_tolerances(mags, 6, 192)
    values = qc.mmd2(sums, 6)
    assert abs(want["mean"] - values.mean()) <= tol.max() and abs(want["std"] - values.std()) <= 2 * tol.max()
    with pytest.raises(ValueError, match="at least 2"):
        one = quality.KID(net, dims=192, size=SIDE)
        one.update(sets[0][:1], 0)
        one.update(sets[1], 1)
        one.compute()


# ------------------------------------------------------------------------------------------------ scripts.quality
def test_quality_script_with_kid_and_object_crops(cuda, tmp_path, capsys):
    from PIL import Image
    from canonicalsg2im_amd import quality
    from canonicalsg2im_amd.inception import InceptionV3
    from canonicalsg2im_amd.scripts import quality as script
    rng = np.random.RandomState(9)
    names = ["cube", {"shape": "sphere", "color": "red"}, "cylinder"]
    sets, folders, rows = [], [], []
    for i in range(8):
        n = 2 + i % 2
        rows.append({"image_id": 100 + i, "objects": [names[(i + k) % 3] for k in range(n)],
                     "gt_boxes": np.concatenate([rng.uniform(0, 0.5, (n, 2)), rng.uniform(0.2, 0.5, (n, 2))], axis=1).tolist()})
    for k in range(2):
        d = tmp_path / ("set%d" % k)
        d.mkdir()
        sets.append(qc.pictures(8, 32, seed=50 + k))
        for i, pic in enumerate(sets[-1]):
            Image.fromarray(pic).save(str(d / ("%d.png" % (100 + i))))
        folders.append(str(d))
    layouts = tmp_path / "layouts.json"
    layouts.write_text(json.dumps({"split": "val", "images": rows}))
    out = tmp_path / "out"
    common = ["--fid_weights", "random", "--dims", "64", "--batch-size", "4", "--output_dir", str(out)]
    before = script.main(folders + common)
    assert set(before) == {"fid", "dims", "batch_size", "channel_order", "images", "stand_in"}          # today's keys, exactly
    assert set(json.load(open(str(out / "quality.json")))) == set(before)
    capsys.readouterr()
    res = script.main(folders + common + ["--kid", "--kid_subsets", "3", "--kid_subset_size", "6", "--object_crops", str(layouts)])
    text = capsys.readouterr().out
    for line in ("FID:", "KID:", "SceneFID:", "class_mean_distance:", "SceneKID:"):
        hit = [l for l in text.splitlines() if l.startswith(line)]
        assert len(hit) == 1 and "stand-in" in hit[0], (line, text)
    saved = json.load(open(str(out / "quality.json")))
    assert saved == json.loads(json.dumps(res)) and res["fid"] == before["fid"]
    assert set(res) == set(before) | {"kid", "objects"}
    assert set(res["kid"]) == {"mean", "std", "subsets", "subset_size", "n", "stand_in"}
    obj = res["objects"]
    assert set(obj) == {"scene_fid", "crops", "layout_boxes", "min_object_size", "class_mean_distance", "kid", "stand_in"}
    assert set(obj["class_mean_distance"]) == {"mean", "per_class", "missing"} and obj["class_mean_distance"]["missing"] == []
    assert res["stand_in"] and res["kid"]["stand_in"] and obj["stand_in"] and obj["kid"]["stand_in"]
    n_crops = sum(len(r["objects"]) for r in rows)
    assert obj["crops"] == [n_crops, n_crops] and obj["layout_boxes"] == "gt" and obj["min_object_size"] == 0.0
    assert res["kid"]["n"] == [8, 8] and res["kid"]["subset_size"] == 6 and obj["kid"]["n"] == [n_crops, n_crops]
    # the API on the same files, called as the script calls it (bgr, 4 pictures per update)
    net = InceptionV3("fid", "random").to(cuda)
    crops = quality.crops_from_layouts({"images": rows})
    classes = sorted({key for _, keys in crops.values() for key in keys})
    assert len(classes) == 3 and sorted(obj["class_mean_distance"]["per_class"]) == classes
    kid = quality.KID(net, dims=64, channel_order="bgr", subsets=3, subset_size=6)
    sides = []
    for which, pics in enumerate(sets):
        ofid = quality.ObjectFID(net, dims=64, channel_order="bgr", batch_size=4, classes=classes)
        feats = []
        for i in (0, 4):
            dev_pics = torch.from_numpy(pics[i:i + 4]).to(cuda)
            kid.update(dev_pics, which)
            boxes = [b for r in rows[i:i + 4] for b in r["gt_boxes"]]
            index = [k for k, r in enumerate(rows[i:i + 4]) for _ in r["objects"]]
            ids = [classes.index(key) for r in rows[i:i + 4] for key in crops[r["image_id"]][1]]
            feats.append(ofid.update(dev_pics, boxes, index, ids))
        sides.append((ofid, torch.cat(feats), ofid.statistics()))
        with np.load(str(out / ("stats_%s_objects.npz" % "AB"[which]))) as f:
            assert np.array_equal(f["mu"], sides[-1][2][0]) and np.array_equal(f["sigma"], sides[-1][2][1])
    assert res["kid"] == kid.compute()
    assert obj["scene_fid"] == quality.frechet_distance(*sides[0][2], *sides[1][2])
    per = quality.class_mean_distance(*sides[0][0].class_means(), *sides[1][0].class_means())
    assert obj["class_mean_distance"]["mean"] == per["mean"]
    assert obj["class_mean_distance"]["per_class"] == {classes[c]: d for c, d in per["per_class"].items()}
    scene_kid = quality.kid_from_features(sides[0][1], sides[1][1], 3, 6, 0)
    assert {k: v for k, v in obj["kid"].items() if k != "stand_in"} == scene_kid
    # a picture without a row, and a row without a picture, end the run with the id named
    Image.fromarray(sets[0][0]).save(str(tmp_path / "set1" / "999.png"))
    with pytest.raises(SystemExit, match="999"):
        script.main(folders + common + ["--object_crops", str(layouts)])
    (tmp_path / "set1" / "999.png").unlink()
    (tmp_path / "set1" / "103.png").unlink()
    with pytest.raises(SystemExit, match="image id 103 has a row and no picture"):
        script.main(folders + common + ["--object_crops", str(layouts)])
