"""COCO segmentation masks and mask centroids on a real MI355X: csg_coco_masks (csrc/coco_masks.hip) through ops.coco_masks
against the restatement of tests/mask_cases.py (which tests/test_mask_cases.py pins on the CPU), and the two COCO folder
datasets with `segmentations=True` end to end.

No tolerance on the masks or on the centres against the numpy closed form: the device makes the same integer and fp64
operations, so the results are equal; the centres are also held within 8 ulp of torch's own fp32 recipe (3 measured on the
CPU).  Shapes: batches of 3 samples with 1, 3 and 5 objects, M in {2, 4, 16, 32, 64}, pictures up to 200 x 180."""
import os
import random

import numpy as np
import pytest
import torch

import mask_cases as mc
import pair_cases as pc
from oracle import canon

pytestmark = pytest.mark.gpu

MODEL = ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--batch_size", "3", "--no_vgg_loss", "--gconv_hidden_dim", "64",
         "--gconv_dim", "32", "--loader_num_workers", "2", "--min_objects", "1", "--min_object_size", "0",
         "--coco_segmentations", "1"]
_EXPECTED = {}


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def expected(bi, M):
    """mc.expected of table batch `bi` at M: computed once, shared, never written to."""
    if (bi, M) not in _EXPECTED:
        out = mc.expected(mc.table()[bi], M)
        for a in out:
            a.setflags(write=False)
        _EXPECTED[(bi, M)] = out
    return _EXPECTED[(bi, M)]


def table_fields(batch):
    """The operands of ops.coco_masks made from the table directly (not through the dataset): numpy arrays by name."""
    from canonicalsg2im_amd.sg2im.data.packed_coco import pack_segmentations
    O = max(len(s["objects"]) for s in batch)
    segs, boxes = [], np.full((len(batch), O, 4), -1.0, np.float32)
    for b, s in enumerate(batch):
        WW, HH = s["size"]
        rows = []
        for o, obj in enumerate(s["objects"]):
            seg = obj["segmentation"]
            boxes[b, o] = mc.box_of(obj["bbox"], WW, HH)
            if isinstance(seg, list):
                rows.append((1, mc.crop_of(obj["bbox"], WW, HH), [np.asarray(p, np.float64).reshape(-1, 2) for p in seg]))
            else:
                counts = seg["counts"] if isinstance(seg["counts"], list) else mc.rle_from_string(seg["counts"])
                rows.append((2, mc.crop_of(obj["bbox"], WW, HH), mc.toggles_of(counts)))
        segs.append(rows)
    f = pack_segmentations(segs, np.asarray([[s["size"][1], s["size"][0]] for s in batch], np.int64), O)
    f["boxes"] = boxes
    return f


def launch(ops, cuda, f, M, **kw):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in f.items()}
    d = {k: v.to(cuda) for k, v in t.items()}
    out = ops.coco_masks(d["seg_kind"], d["seg_crop"], d["seg_sizes"], d["boxes"], d["seg_obj_poly"], d["seg_poly_off"],
                         d["seg_poly_xy"], d["seg_obj_runs"], d["seg_toggles"], M, kind_host=t["seg_kind"],
                         crop_host=t["seg_crop"], sizes_host=t["seg_sizes"], obj_poly_host=t["seg_obj_poly"],
                         poly_off_host=t["seg_poly_off"], poly_xy_host=t["seg_poly_xy"], obj_runs_host=t["seg_obj_runs"], **kw)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize("M", mc.MASK_SIZES)
@pytest.mark.parametrize("bi", [0, 1])
def test_masks_and_centres_equal_the_restatement_on_every_table_row(cuda, bi, M):
    from canonicalsg2im_amd import ops
    batch = mc.table()[bi]
    want_masks, want_centres, boxes = expected(bi, M)
    f = table_fields(batch)
    masks, centres = launch(ops, cuda, f, M)
    again = launch(ops, cuda, f, M)
    B, O = f["seg_kind"].shape
    assert masks.dtype == torch.int64 and tuple(masks.shape) == (B, O + 1, M, M)
    assert centres.dtype == torch.float32 and tuple(centres.shape) == (B, O, 2)
    assert torch.equal(masks, again[0]) and np.array_equal(centres.cpu().numpy().view(np.uint32),
                                                           again[1].cpu().numpy().view(np.uint32))       # the same bytes
    got_m, got_c = masks.cpu().numpy(), centres.cpu().numpy()
    for b, s in enumerate(batch):
        for o, obj in enumerate(s["objects"]):
            assert np.array_equal(got_m[b, o], want_masks[b, o]), "%s at M = %d: %d pixels differ" % (
                obj["what"], M, int((got_m[b, o] != want_masks[b, o]).sum()))
            assert np.array_equal(got_c[b, o].view(np.uint32), want_centres[b, o].view(np.uint32)), (obj["what"], M, got_c[b, o],
                                                                                                     want_centres[b, o])
            far = mc.ulps(got_c[b, o], mc.centre_torch(boxes[b, o], want_masks[b, o])).max()
            assert far <= 8.0, (obj["what"], M, far)
        n = len(s["objects"])
        assert not got_m[b, n:O].any() and (got_c[b, n:] == np.float32(-1.5)).all()           # padding rows: 0, the box centre of -1
    assert (got_m[:, O] == 1).all()                                                             # the __image__ row
    assert np.array_equal(got_m, want_masks) and np.array_equal(got_c.view(np.uint32), want_centres.view(np.uint32))
    if M == 16:                                              # centres alone, and caller-owned buffers
        none, only = launch(ops, cuda, f, M, want_masks=False)
        assert none is None and torch.equal(only, centres)
        om = torch.full((B, O + 1, M, M), 7, dtype=torch.int64, device=cuda)
        oc = torch.full((B, O, 2), 7.0, device=cuda)
        rm, rc = launch(ops, cuda, f, M, out_masks=om, out_centers=oc)
        assert rm is om and rc is oc and torch.equal(om, masks) and torch.equal(oc, centres)


def test_refusals_carry_a_message_and_launch_nothing(cuda):
    from canonicalsg2im_amd import _lib, ops
    f = table_fields(mc.table()[0])
    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        for bad in (3, 128, 0, 1):
            with pytest.raises(RuntimeError, match="mask_size must be a power of two in 2 .. 64, got %d" % bad):
                launch(ops, cuda, f, bad)
        t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in f.items()}
        d = {k: v.to(cuda) for k, v in t.items()}
        order = ("seg_kind", "seg_crop", "seg_sizes", "boxes", "seg_obj_poly", "seg_poly_off", "seg_poly_xy", "seg_obj_runs",
                 "seg_toggles")
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.coco_masks(*[t[k] if k == "boxes" else d[k] for k in order], 16)
        with pytest.raises(RuntimeError, match="crop must be contiguous torch.int32"):
            ops.coco_masks(*[d[k].long() if k == "seg_crop" else d[k] for k in order], 16)
        g = dict(f, seg_kind=f["seg_kind"].copy())
        g["seg_kind"][1, 0] = 3
        with pytest.raises(RuntimeError, match="sample 1 object 0: kind = 3"):
            launch(ops, cuda, g, 16)
        g = dict(f, seg_crop=f["seg_crop"].copy())
        g["seg_crop"][2, 1] = (4, 4, 4, 9)
        with pytest.raises(RuntimeError, match=r"sample 2 object 1: crop \(4, 4, 4, 9\) is empty or outside the 33 x 27 picture"):
            launch(ops, cuda, g, 16)
        g = dict(f, seg_crop=f["seg_crop"].copy())
        g["seg_crop"][0, 0] = (0, 0, 25, 20)
        with pytest.raises(RuntimeError, match="sample 0 object 0: crop .0, 0, 25, 20. is empty or outside the 24 x 20 picture"):
            launch(ops, cuda, g, 16)
        g = dict(f, seg_obj_poly=f["seg_obj_poly"].copy())
        g["seg_obj_poly"][2, 4] = (f["seg_poly_off"].shape[0] - 2, 2)
        with pytest.raises(RuntimeError, match="sample 2 object 4: polygons"):
            launch(ops, cuda, g, 16)
        g = dict(f, seg_poly_off=f["seg_poly_off"].copy())
        g["seg_poly_off"][-1] += 1
        with pytest.raises(RuntimeError, match="poly_off runs from 0 to"):
            launch(ops, cuda, g, 16)
        g = dict(f, seg_poly_xy=f["seg_poly_xy"].copy())
        g["seg_poly_xy"][3, 1] = 2.0e6
        with pytest.raises(RuntimeError, match="polygon coordinate 7 is 2e.06"):
            launch(ops, cuda, g, 16)
        g = dict(f, seg_sizes=f["seg_sizes"].copy())
        g["seg_sizes"][1] = (0, 40)
        with pytest.raises(RuntimeError, match="the picture of sample 1 is 0 x 40"):
            launch(ops, cuda, g, 16)
        r = table_fields(mc.table()[1])
        r["seg_obj_runs"] = r["seg_obj_runs"].copy()
        r["seg_obj_runs"][2, 1, 1] = r["seg_toggles"].shape[0]
        with pytest.raises(RuntimeError, match="sample 2 object 1: toggles"):
            launch(ops, cuda, r, 16)
        with pytest.raises(RuntimeError, match="out_masks must be contiguous int64 .B,O.1,M,M."):
            launch(ops, cuda, f, 16, out_masks=torch.zeros((3, 6, 16, 16), dtype=torch.int32, device=cuda))
        torch.cuda.synchronize()
        assert "coco_masks" not in _lib.prof_read()
        launch(ops, cuda, f, 16)
        assert _lib.prof_read()["coco_masks"][1] == 1
        assert _lib.lib.csg_version() >= 119
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


def test_a_stale_device_row_becomes_a_padding_row(cuda):
    """The host copies pass, the device buffer disagrees (as under a replayed graph whose buffer was not refreshed): a row whose
    device crop leaves the picture, whose kind is unknown or whose polygons / toggles leave their arrays is an empty mask with
    the box centre; nothing is indexed with it, and the other rows are theirs."""
    from canonicalsg2im_amd import ops
    for bi, spoil in ((0, {"seg_crop": ((1, 0), (0, 0, 4000, 20)), "seg_kind": ((2, 1), 9),
                           "seg_obj_poly": ((2, 4), (2 ** 30, 2 ** 30))}),
                      (1, {"seg_obj_runs": ((2, 0), (5, 2 ** 31 - 1)), "seg_sizes": ((1,), (2 ** 40, 2 ** 40))})):
        f = table_fields(mc.table()[bi])
        t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in f.items()}
        d = {k: v.to(cuda) for k, v in t.items()}
        dead = set()
        for name, (where, value) in spoil.items():
            d[name][where] = torch.as_tensor(value, dtype=d[name].dtype, device=cuda)
            dead |= {(where[0], o) for o in range(f["seg_kind"].shape[1])} if name == "seg_sizes" else {where}
        masks, centres = ops.coco_masks(d["seg_kind"], d["seg_crop"], d["seg_sizes"], d["boxes"], d["seg_obj_poly"],
                                        d["seg_poly_off"], d["seg_poly_xy"], d["seg_obj_runs"], d["seg_toggles"], 16,
                                        kind_host=t["seg_kind"], crop_host=t["seg_crop"], sizes_host=t["seg_sizes"],
                                        obj_poly_host=t["seg_obj_poly"], poly_off_host=t["seg_poly_off"],
                                        poly_xy_host=t["seg_poly_xy"], obj_runs_host=t["seg_obj_runs"])
        torch.cuda.synchronize()
        want_masks, want_centres, boxes = (a.copy() for a in expected(bi, 16))
        for b, o in dead:
            want_masks[b, o] = 0
            want_centres[b, o] = boxes[b, o, :2] + np.float32(0.5) * boxes[b, o, 2:]
        assert np.array_equal(masks.cpu().numpy(), want_masks)
        assert np.array_equal(centres.cpu().numpy().view(np.uint32), want_centres.view(np.uint32))


# ------------------------------------------------------------------------------------------------- 2. the datasets
@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """[dataroot] per table batch: written once, shared, never written to."""
    roots = []
    for bi, batch in enumerate(mc.table()):
        root = str(tmp_path_factory.mktemp("masks%d" % bi))
        mc.write_folder(root, batch)
        roots.append(root)
    return roots


def _built(cuda, root, dataset, mask_size, extra=(), rng_seed=5):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    argv = MODEL + ["--dataset", dataset, "--mask_size", str(mask_size), "--dataroot", root] + list(extra)
    ds = folder_dataset(build_parser().parse_args(argv), "train")
    assert len(ds) == 3 and ds.segmentations and ds.mask_size == mask_size
    opt = T.make_opt(ds.vocab, argv)
    builder = folder_builder(ds, opt, None, cuda, rng=random.Random(rng_seed))
    pending = builder.start([0, 1, 2])
    batch = builder.finish(pending)
    torch.cuda.synchronize()
    builder.close()
    return ds, opt, pending, batch


def _with_image_row(centres, boxes):
    B = boxes.shape[0]
    return (np.concatenate([centres, np.full((B, 1, 2), -1.5, np.float32)], 1),
            np.concatenate([boxes, np.full((B, 1, 4), -1.0, np.float32)], 1))


@pytest.mark.parametrize("mask_size", [16, 0])
@pytest.mark.parametrize("bi", [0, 1])
def test_packed_coco_batches_carry_the_masks_and_the_graph_of_the_mask_centres(cuda, folders, bi, mask_size):
    M = mask_size or 64                                     # the reference's working size for packed_coco
    ds, opt, pending, batch = _built(cuda, folders[bi], "packed_coco", mask_size)
    imgs, objs, boxes, triplets, conv_counts, ttype, masks, ids = batch
    want_masks, want_centres, want_boxes = expected(bi, M)
    centres, boxes_all = _with_image_row(want_centres, want_boxes)
    assert ids.tolist() == [101, 102, 103] and tuple(imgs.shape) == (3, 3, 64, 64)
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), boxes_all.view(np.uint32))
    if mask_size:
        assert masks.dtype == torch.int64 and np.array_equal(masks.cpu().numpy(), want_masks)
    else:
        assert masks is None
    # the graph is built over the first n = objects + 1 rows of a sample: the row after its objects is its __image__ row (a
    # padding row is one: object 0, box -1), as in the oracle
    objs0 = objs.cpu().numpy()[..., 0]
    n = np.asarray([len(s["objects"]) + 1 for s in mc.table()[bi]])
    want_t, want_tt, _ = canon.canonical_batch(objs0, boxes_all, centres, n, ds.vocab)
    assert np.array_equal(triplets.cpu().numpy(), want_t) and np.array_equal(ttype.cpu().numpy(), want_tt)
    if bi == 0:                                             # the concave L: the box centres give another graph
        box_c = boxes_all[..., :2] + np.float32(0.5) * boxes_all[..., 2:]
        other_t, _, _ = canon.canonical_batch(objs0, boxes_all, box_c, n, ds.vocab)
        assert other_t.shape != want_t.shape or not np.array_equal(other_t[1], want_t[1])
        assert np.array_equal(other_t[0], want_t[0]) if other_t.shape == want_t.shape else True


@pytest.mark.parametrize("mask_size", [16, 0])
@pytest.mark.parametrize("bi", [0, 1])
def test_coco_batches_relate_the_sampled_pairs_by_the_mask_centres(cuda, folders, bi, mask_size):
    M = mask_size or 32                                     # the reference's working size for coco
    ds, opt, pending, batch = _built(cuda, folders[bi], "coco", mask_size, extra=["--max_objects", "8"])
    imgs, objs, boxes, triplets, conv_counts, ttype, masks, ids = batch
    want_masks, want_centres, want_boxes = expected(bi, M)
    centres, boxes_all = _with_image_row(want_centres, want_boxes)
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), boxes_all.view(np.uint32))
    if mask_size:
        assert np.array_equal(masks.cpu().numpy(), want_masks)
    else:
        assert masks is None
    p2i = ds.vocab["pred_name_to_idx"]
    other, flip, counts = pending.other.numpy(), pending.flip.numpy(), pending.counts.numpy()

    def graph(cen):                                         # the row after a sample's objects is its __image__ row
        rows = [pc.pair_rows_atan2(boxes_all[b], cen[b], int(counts[b]), other[b], flip[b], p2i) for b in range(3)]
        return pc.batch_from_rows(rows, counts, ds.vocab)[:2]

    want_t, want_tt = graph(centres)
    assert np.array_equal(triplets.cpu().numpy(), want_t) and np.array_equal(ttype.cpu().numpy(), want_tt)
    if bi == 0:                                             # the seed draws the concave L and its partner as a pair
        assert other[1][0] == 1 or other[1][1] == 0
        box_t, _ = graph(boxes_all[..., :2] + np.float32(0.5) * boxes_all[..., 2:])
        assert box_t.shape != want_t.shape or not np.array_equal(box_t[1], want_t[1])


def test_a_training_step_at_mask_size_16_has_the_mask_terms(cuda, folders):
    from canonicalsg2im_amd import train as T
    ds, opt, pending, batch = _built(cuda, folders[0], "coco", 16, extra=["--max_objects", "8", "--mask_pred_loss_weight", "1",
                                                                       "--g_mask_dim", "40", "--mask_noise_dim", "8"])
    torch.manual_seed(6)
    trainer = T.Trainer(opt, cuda)
    G, D = trainer.step(batch)
    torch.cuda.synchronize()
    for k, val in list(G.items()) + list(D.items()):
        assert bool(torch.isfinite(val).all()), k
    assert {"masks_pred", "GAN_Mask"} <= set(G) and {"D_mask_fake", "D_mask_real", "total_mask_loss"} <= set(D)
    assert float(G["masks_pred"]) > 0
