"""The unpacked CLEVR dataset on a real MI355X: the graph kernels (csrc/clevr_graph.hip, csg_clevr_graph_*) against the
reference's recorded output (tests/golden/clevr_unpacked.npz) and the bit-row restatement of tests/clevr_graph_cases.py
(which tests/test_clevr_graph_cases.py pins to the reference on the CPU); then the folder dataset that feeds them, a trainer
step, the sampler and the command lines on its vocabulary.

Every output is an integer, or a float the reference recorded: equality everywhere, no tolerance."""
import os

import numpy as np
import pytest
import torch

import clevr_graph_cases as gc

pytestmark = pytest.mark.gpu

MODEL = ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--batch_size", "2", "--no_vgg_loss", "--use_img_disc", "1",
         "--gconv_hidden_dim", "64", "--gconv_dim", "32", "--dataset", "clevr", "--loader_num_workers", "2"]
P = len(gc.PREDS)
PAD = gc.PREDS["__padding__"]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("clevruroot"))
    base = gc.write_folder(root)
    gc.write_folder(root, split="val")
    return root, base


def _vocab():
    meta, _ = gc.golden()
    return meta["vocab"]


def _run(rows, n_objs, keep, O=None, rows_dev=None, **kw):
    """clevr_triplets on a padded batch -> host arrays (triplets, conv_counts, triplet_type)."""
    from canonicalsg2im_amd.sg2im.data import clevr_triplets
    rows = torch.from_numpy(np.ascontiguousarray(rows))
    n_objs = torch.from_numpy(np.ascontiguousarray(n_objs))
    objs = torch.zeros((rows.shape[0], int(n_objs.max()) if O is None else O), dtype=torch.int64, device="cuda")
    dev = rows.cuda() if rows_dev is None else torch.from_numpy(np.ascontiguousarray(rows_dev)).cuda()
    out = clevr_triplets(objs, n_objs, _vocab(), dev, rows_host=rows, use_transitivity=keep, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check(got, want_triplets, counts):
    t, cc, tt = got
    B = want_triplets.shape[0]
    assert t.dtype == np.int64 and t.shape == want_triplets.shape and np.array_equal(t, want_triplets)
    assert tt.dtype == np.int64 and tt.shape == t.shape[:2] and not tt.any()              # ORIGINAL_EDGE, 0 on padding
    assert cc.dtype == np.float32 and cc.shape == (B, P, P + 1) and not cc.any()          # never drawn
    assert [int((row[:, 1] != PAD).sum()) for row in t] == list(counts) and t.shape[1] == max(counts)


# ------------------------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("keep", [0, 1], ids=["keep0", "keep1"])
@pytest.mark.parametrize("name", gc.NAMES + ("mixed",))
def test_golden_cases_equal_the_reference_and_themselves(cuda, name, keep):
    """Every case alone and the mixed batch (1, 3, 10 and 63 objects): triplets, counts, types and conv_counts are the
    reference's, element for element, and a second run gives the same bytes."""
    meta, g = gc.golden()
    rows, n_objs = gc.padded_rows(gc.MIXED if name == "mixed" else (name,))
    want = g["%s_k%d_triplets" % (name, keep)].astype(np.int64)
    got = _run(rows, n_objs, keep)
    print("%s keep %d: R = %d, T = %d, counts %s" % (name, keep, rows.shape[1], got[0].shape[1], meta["counts"]["%s_k%d" % (name, keep)]))
    _check(got, want, meta["counts"]["%s_k%d" % (name, keep)])
    again = _run(rows, n_objs, keep)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("keep", [0, 1], ids=["keep0", "keep1"])
def test_every_case_in_one_batch_equals_the_restatement(cuda, keep):
    """Twelve blocks in one launch, objects padded to a wider O, the padding rows of a sample in front of its rows."""
    rows, n_objs = gc.padded_rows(gc.NAMES)
    want, counts = gc.batch(rows, n_objs, keep)
    _check(_run(rows, n_objs, keep, O=80), want, counts)
    short = [b for b, nm in enumerate(gc.NAMES) if nm != "n63"]
    shifted = rows.copy()
    shifted[short] = np.roll(rows[short], 5, axis=1)                                      # 5 padding rows lead every short sample
    assert (shifted[short, :5, 1] == PAD).all()
    _check(_run(shifted, n_objs, keep, O=80), want, counts)


def test_two_launches_and_none_of_the_canonical_ones(cuda):
    from canonicalsg2im_amd import _lib
    rows, n_objs = gc.padded_rows(gc.MIXED)
    _run(rows, n_objs, 0)
    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        _run(rows, n_objs, 0)
        seen = _lib.prof_read()
        assert seen["clevr_graph_count"][1] == 1 and seen["clevr_graph_emit"][1] == 1
        assert not any(k.startswith("canon") for k in seen), sorted(seen)
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


def test_bad_inputs_are_refused_before_any_launch(cuda):
    from canonicalsg2im_amd import _lib
    from canonicalsg2im_amd.sg2im.data import clevr_triplets
    rows, n_objs = gc.padded_rows(("three_order", "ten_orders"))

    def edit(b, r, c, v):
        out = rows.copy()
        out[b, r, c] = v
        return out

    many = np.asarray([4, 65], np.int64)
    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        for what, kw, err, msg in (
                ("object == n", dict(rows=edit(0, 0, 2, 3)), RuntimeError, "sample 0 row 0: object .* outside"),
                ("negative", dict(rows=edit(1, 7, 0, -1)), RuntimeError, "sample 1 row 7: object .* outside"),
                ("predicate == P", dict(rows=edit(1, 0, 1, P)), RuntimeError, "predicate 6 outside"),
                ("64 objects", dict(n_objs=many, O=80), RuntimeError, "at most 63 objects per sample"),
                ("more rows than objs has", dict(O=10), RuntimeError, r"n_objs\[1\] = 11 outside"),
                ("no __image__ row", dict(n_objs=np.asarray([4, 0], np.int64)), RuntimeError, r"n_objs\[1\] = 0 outside"),
                ("use_transitivity", dict(keep=2), ValueError, "use_transitivity must be 0 or 1"),
                ("use_transitivity", dict(keep=0.5), ValueError, "use_transitivity must be 0 or 1"),
                ("rows (B,R,2)", dict(rows=rows[..., :2]), ValueError, "rows must be"),
                ("n_objs (B+1,)", dict(n_objs=np.asarray([4, 11, 2], np.int64)), ValueError, "n_objs, and n_objs_host, must be")):
            a = dict(rows=rows, n_objs=n_objs, keep=0)
            a.update(kw)
            with pytest.raises(err, match=msg):
                _run(**a)
        with pytest.raises(ValueError, match="rows_host of the same shape"):
            clevr_triplets(torch.zeros((2, 11), dtype=torch.int64, device=cuda), torch.from_numpy(n_objs), _vocab(),
                           torch.from_numpy(rows).cuda(), rows_host=torch.from_numpy(rows[:, :5].copy()))
        torch.cuda.synchronize()
        seen = _lib.prof_read()
        assert "clevr_graph_count" not in seen and "clevr_graph_emit" not in seen, sorted(seen)   # nothing was enqueued
        # a device copy that is not the host's rows: the kernel indexes nothing with the row, marks the sample, no emit
        with pytest.raises(RuntimeError, match="sample 0 on the device are not the rows the host holds"):
            _run(rows, n_objs, 0, rows_dev=edit(0, 1, 0, 3))
        seen = _lib.prof_read()
        assert seen["clevr_graph_count"][1] == 1 and "clevr_graph_emit" not in seen
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


# ------------------------------------------------------------------------------------------------- 2. the dataset
def _opt(vocab, extra=()):
    from canonicalsg2im_amd import train as T
    return T.make_opt(vocab, MODEL + list(extra))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("flags", [(), ("--use_transitivity", "1"), ("--include_relationships", "0")],
                         ids=["keep0", "keep1", "no_relationships"])
def test_whole_batch_equals_the_reference_collate(cuda, folder, flags):
    """The dataset of the command line and its builder on RGBA and RGB pictures: objects, boxes — the (0, 0, 1, 1) row of
    `__image__` and the -1 rows after it — and triplets of the 8-tuple are the reference collate's."""
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    from canonicalsg2im_amd.sg2im.data.clevr import ClevrDialogBatchBuilder
    meta, g = gc.golden()
    flags = list(flags)
    ds = folder_dataset(build_parser().parse_args(["--dataset", "clevr", "--dataroot", folder[0], "--image_size", "64,64"] + flags),
                        "train")
    opt = _opt(ds.vocab, flags)
    builder = folder_builder(ds, opt, None, cuda)
    assert isinstance(builder, ClevrDialogBatchBuilder)
    pending = builder.start([0, 1, 2, 3])
    assert pending.desc[:, 3].tolist() == [4, 3, 4, 3] and tuple(pending.rel.shape) == (4, 4 * 1953, 3)
    assert not pending.rel.is_cuda and pending.rel.dtype == torch.int64 and pending.counts.tolist() == [1, 3, 10, 63]
    imgs, objs, boxes, triplets, conv_counts, ttype, masks, ids = builder.finish(pending)
    torch.cuda.synchronize()
    builder.close()
    assert masks is None and ids.tolist() == [10, 12, 13, 21]
    assert objs.dtype == torch.int64 and np.array_equal(objs.cpu().numpy(), g["mixed_objs"].astype(np.int64))
    got_boxes = boxes.cpu().numpy()
    assert _same_bits(got_boxes, g["mixed_boxes"])
    assert got_boxes[0, 1].tolist() == [0, 0, 1, 1] and (got_boxes[0, 2:] == -1).all() and got_boxes[3, 63].tolist() == [0, 0, 1, 1]
    if "--include_relationships" in flags:
        want = np.zeros((4, 63, 3), np.int64)
        want[..., 1] = PAD
        for b, n in enumerate((1, 3, 10, 63)):
            want[b, :n] = [[i, 0, n] for i in range(n)]
        counts = [1, 3, 10, 63]
    else:
        keep = int("--use_transitivity" in flags)
        want, counts = g["mixed_k%d_triplets" % keep].astype(np.int64), meta["counts"]["mixed_k%d" % keep]
    _check([triplets.cpu().numpy(), conv_counts.cpu().numpy(), ttype.cpu().numpy()], want, counts)
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (4, 3, 64, 64) and bool(torch.isfinite(imgs).all())


def test_a_trainer_step_and_the_sampler_on_the_datasets_vocabulary(cuda, folder):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    ds = folder_dataset(build_parser().parse_args(["--dataset", "clevr", "--dataroot", folder[0], "--image_size", "64,64"]), "train")
    opt = _opt(ds.vocab)
    torch.manual_seed(4)
    trainer = T.Trainer(opt, cuda)
    builder = folder_builder(ds, opt, trainer, cuda)
    batch = builder.build([2, 1])
    builder.close()
    assert batch[7].tolist() == [13, 12] and tuple(batch[1].shape) == (2, 11, 4) and tuple(batch[3].shape) == (2, 46, 3)
    G, D = trainer.step(batch)
    for k, val in list(G.items()) + list(D.items()):
        assert bool(torch.isfinite(val).all()), k
    sampler = Sampler(opt, cuda)
    imgs, boxes_pred, _ = sampler.generate(batch[1], batch[3], batch[5], deprocess="decode_img")
    torch.cuda.synchronize()
    assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == (2, 3, 64, 64) and tuple(boxes_pred.shape)[:2] == (2, 11)


def test_command_lines_train_validate_and_sample_on_the_folder(cuda, folder, tmp_path, capsys):
    from canonicalsg2im_amd.scripts import evaluate as val_cli, sample as sample_cli, train as train_cli
    root, base = folder
    pictures = os.path.join(base, "images")
    out = str(tmp_path / "out")
    common = list(MODEL) + ["--dataroot", root]
    train_cli.main(common + ["--num_iterations", "2", "--print_every", "1", "--output_dir", out, "--checkpoint_every", "2",
                             "--val_every", "2", "--num_val_samples", "4"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: 4 pictures of %s, 2 loader threads" % pictures in lines, lines
    assert sum(l.startswith("t = ") for l in lines) == 2 and sum(l.startswith("Iter: 2, ") for l in lines) == 2
    train_cli.main(list(MODEL) + ["--dataroot", str(tmp_path / "nowhere"), "--num_iterations", "1", "--print_every", "1"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: seeded synthetic batches (clevr shapes)" in lines and not any(l.startswith("loader:") for l in lines)
    ck = os.path.join(out, "itr_2.pt")
    val_cli.main(common + ["--checkpoint_name", ck, "--num_val_samples", "4"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: 4 pictures of %s" % pictures in lines
    assert len([l for l in lines if l.startswith("Iter: 2, ")]) == 2, lines
    pics = str(tmp_path / "pics")
    sample_cli.main(common + ["--checkpoint_name", ck, "--split", "val", "--output_dir", pics])
    assert "data: 4 pictures of %s" % pictures in capsys.readouterr().out.splitlines()
    written = sorted(os.path.relpath(os.path.join(d, f), pics) for d, _, files in os.walk(pics) for f in files if f.endswith(".png"))
    sets = ("gt", "generation/gt_box_gt_mask", "generation/pred_box_pred_mask", "layout/gt", "layout/pred")
    assert written == sorted("%s/%d.png" % (k, i) for k in sets for i in (10, 12, 13, 21)), written
