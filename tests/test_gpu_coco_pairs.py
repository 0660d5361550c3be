"""The unpacked `coco` dataset's input stage on a real MI355X: csg_pair_relations and csg_canon_general_build_dev
(csrc/canon.hip) against the reference's recorded samples (tests/golden/coco_pairs.npz) and the Python restatement of
tests/pair_cases.py (which tests/test_pair_cases.py pins to the reference on the CPU), and the folder dataset that feeds
them.

No tolerance anywhere: a predicate is decided by fp32 comparisons that both sides make operation by operation, the graph is
integers, the pictures go through the bit-exact input stage; so the results are equal.  Shapes: B <= 8, O <= 9, pictures
<= 64 x 64; one launch of (8,40) rows for a second, ragged block."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import pair_cases as pc
import preprocess_cases as pre

pytestmark = pytest.mark.gpu

MODEL = ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--batch_size", "5", "--no_vgg_loss", "--use_img_disc", "1",
         "--gconv_hidden_dim", "64", "--gconv_dim", "32", "--dataset", "coco", "--loader_num_workers", "2",
         "--min_objects", "1"]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """(dataroot, image dir, the host pipeline's 64 x 64 fp32 images): written and computed once, shared, never written to."""
    root = str(tmp_path_factory.mktemp("cocoroot"))
    image_dir, decoded = pc.write_folder(root)
    pc.write_folder(root, split="val")
    return root, image_dir, [pre.to_float(pre.pil_resize_u8(px, 64, 64)) for px in decoded]


def _pairs(ops, cuda, vocab, boxes, counts, other, flip, use_converse, stale_other=None, **kw):
    boxes, counts, other, flip = (torch.from_numpy(np.ascontiguousarray(a)) for a in (boxes, counts, other, flip))
    centers = torch.from_numpy(pc.centers_of(boxes.numpy()))
    other_dev = other.to(cuda) if stale_other is None else torch.from_numpy(stale_other).to(cuda)
    rows = ops.pair_relations(boxes.to(cuda), centers.to(cuda), counts.to(cuda), other_dev, flip.to(cuda), vocab,
                              use_converse=use_converse, other_host=other, flip_host=flip, counts_host=counts, **kw)
    torch.cuda.synchronize()
    return rows.cpu().numpy()


def _row_counts(g):
    return (g["other"] >= 0).sum(1).astype(np.int64)


# ------------------------------------------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize("use_converse", [0, 1])
def test_pair_relations_match_the_restatement_row_for_row(cuda, use_converse):
    """Every golden group drawn with this use_converse (the ties among them: group 1), then the hand-written pairs in both
    directions and with both coins."""
    from canonicalsg2im_amd import ops
    vocab = pc.vocab()
    p2i = vocab["pred_name_to_idx"]
    checked = 0
    for si, gi in pc.cases():
        s, _, g = pc.case_arrays(si, gi)
        if s["use_converse"] != use_converse or not s["include_relationships"]:
            continue
        B, O = g["other"].shape
        boxes = np.ascontiguousarray(g["boxes"][:, :O])
        got = _pairs(ops, cuda, vocab, boxes, _row_counts(g), g["other"], g["flip"], use_converse)
        centers = pc.centers_of(boxes)
        want = pc.padded_rows([pc.pair_rows_atan2(boxes[b], centers[b], int(g["n"][b]), g["other"][b], g["flip"][b], p2i,
                                                  use_converse=bool(use_converse)) for b in range(B)], O, p2i)
        print("%s: (B,O) = (%d,%d), %d rows differ from the restatement, %d from the reference" % (
            pc.case_id((si, gi)), B, O, int((got != want).any(-1).sum()), int((got != g["rows"]).any(-1).sum())))
        assert got.dtype == np.int64 and np.array_equal(got, want) and np.array_equal(got, g["rows"])
        checked += 1
    assert checked == (6 if use_converse else 9)
    hand = pc.hand_written()
    for flips in ((0, 0), (1, 1), (0, 1)):
        for lo in range(0, len(hand), 8):
            boxes = np.stack([b for b, _ in hand[lo:lo + 8]])
            B = boxes.shape[0]
            other = np.tile(np.asarray([1, 0], np.int32), (B, 1))
            flip = np.tile(np.asarray(flips, np.uint8), (B, 1))
            got = _pairs(ops, cuda, vocab, boxes, np.full(B, 2, np.int64), other, flip, use_converse)
            centers = pc.centers_of(boxes)
            want = pc.padded_rows([pc.pair_rows_atan2(boxes[b], centers[b], 2, other[b], flip[b], p2i,
                                                      use_converse=bool(use_converse)) for b in range(B)], 2, p2i)
            assert np.array_equal(got, want), [what for (_, what), g, w in zip(hand[lo:lo + 8], got, want) if (g != w).any()]


def test_more_than_one_block_and_padding_rows(cuda):
    """(B,O) = (8,9) is 72 rows of one block; (8,40) is 320 rows, a full block of 256 lanes and a ragged one.  Seeded boxes,
    counts 0, 2 and the full row among them; rows at or beyond a count are [0, __padding__, 0]."""
    from canonicalsg2im_amd import ops
    vocab = pc.vocab()
    p2i = vocab["pred_name_to_idx"]
    for B, O, seed in ((8, 9, 1), (8, 40, 2)):
        rng = np.random.default_rng(seed)
        boxes = np.concatenate([rng.uniform(0, 0.5, (B, O, 2)), rng.uniform(0.05, 0.5, (B, O, 2))], -1).astype(np.float32)
        counts = np.asarray([0, 2, O, O - 1, 3, O, 2, 5][:B], np.int64)
        other, flip = np.full((B, O), -1, np.int32), np.zeros((B, O), np.uint8)
        for b in range(B):
            for cur in range(int(counts[b])):
                other[b, cur] = rng.choice([j for j in range(int(counts[b])) if j != cur])
                flip[b, cur] = rng.integers(0, 2)
        for conv in (0, 1):
            got = _pairs(ops, cuda, vocab, boxes, counts, other, flip, conv)
            centers = pc.centers_of(boxes)
            want = pc.padded_rows([pc.pair_rows_atan2(boxes[b], centers[b], int(counts[b]), other[b], flip[b], p2i,
                                                      use_converse=bool(conv)) for b in range(B)], O, p2i)
            assert np.array_equal(got, want)
            assert (got[0] == [0, p2i["__padding__"], 0]).all() and (got[3, O - 1] == [0, p2i["__padding__"], 0]).all()


def test_refusals_carry_a_message_and_launch_nothing(cuda):
    from canonicalsg2im_amd import _lib, ops
    vocab = pc.vocab()
    B, O = 2, 3
    boxes = np.tile(np.asarray([0.1, 0.1, 0.2, 0.2], np.float32), (B, O, 1))
    counts = np.asarray([3, 2], np.int64)
    other = np.asarray([[1, 2, 0], [1, 0, -1]], np.int32)
    flip = np.zeros((B, O), np.uint8)
    out = torch.full((B, O, 3), 77, dtype=torch.int64, device=cuda)

    def call(boxes=boxes, counts=counts, other=other, flip=flip, **kw):
        kw.setdefault("out", out)
        return _pairs(ops, cuda, vocab, boxes, counts, other, flip, 0, **kw)

    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        o = other.copy()
        o[0, 1] = 1
        with pytest.raises(RuntimeError, match="sample 0 row 1: other = 1, another row of .0, 3."):
            call(other=o)
        o = other.copy()
        o[1, 0] = 2                                        # sample 1 has two rows: row 2 is not one of them
        with pytest.raises(RuntimeError, match="sample 1 row 0: other = 2, another row of .0, 2."):
            call(other=o)
        o = other.copy()
        o[0, 2] = -1
        with pytest.raises(RuntimeError, match="sample 0 row 2: other = -1"):
            call(other=o)
        f = flip.copy()
        f[0, 0] = 2
        with pytest.raises(RuntimeError, match="sample 0 row 0: flip = 2, 0 or 1"):
            call(flip=f)
        for bad in (4, -1):
            c = counts.copy()
            c[1] = bad
            with pytest.raises(RuntimeError, match="sample 1 has %d rows, 0 .. O = 3" % bad):
                call(counts=c)
        wide = 257
        with pytest.raises(RuntimeError, match="at most 256 objects per sample .got 257."):
            call(boxes=np.zeros((1, wide, 4), np.float32), counts=np.zeros(1, np.int64), other=np.full((1, wide), -1, np.int32),
                 flip=np.zeros((1, wide), np.uint8), out=None)
        twice = dict(vocab, pred_name_to_idx=dict(vocab["pred_name_to_idx"], __inside__=vocab["pred_name_to_idx"]["__above__"]))
        with pytest.raises(RuntimeError, match="the eight predicate ids must be distinct"):
            _pairs(ops, cuda, twice, boxes, counts, other, flip, 0, out=out)
        with pytest.raises(RuntimeError, match="out must be contiguous int64 .B,O,3."):
            call(out=torch.zeros((B, O, 3), dtype=torch.int32, device=cuda))
        dev = [torch.from_numpy(a).to(cuda) for a in (boxes, pc.centers_of(boxes), counts, other, flip)]
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.pair_relations(dev[0].cpu(), *dev[1:], vocab)
        with pytest.raises(RuntimeError, match="other must be contiguous torch.int32"):
            ops.pair_relations(dev[0], dev[1], dev[2], dev[3].long(), dev[4], vocab)
        misaligned = torch.zeros(B * O * 4 + 1, device=cuda)[1:].view(B, O, 4)
        with pytest.raises(RuntimeError, match="boxes must be 16-byte aligned"):
            ops.pair_relations(misaligned, *dev[1:], vocab, out=out)
        host = [ctypes.c_void_p(torch.from_numpy(a).data_ptr()) for a in (counts, other, flip)]
        ids = (ctypes.c_int32 * 8)(*range(8))
        args = [_lib.ptr(t) for t in dev] + host + [B, O, ids, 0, _lib.ptr(out), _lib.stream()]
        for k in (0, 1, 2, 3, 4, 5, 6, 7, 10, 12):
            with pytest.raises(RuntimeError, match="null operand"):
                _lib.check(_lib.lib.csg_pair_relations(*[None if j == k else a for j, a in enumerate(args)]), "pair_relations")
        torch.cuda.synchronize()
        assert "canon_build" not in _lib.prof_read() and bool((out == 77).all())
        got = call()                                        # and the same operands, unspoilt, launch once
        assert _lib.prof_read()["canon_build"][1] == 1 and (got[1, 2] == [0, 0, 0]).all() and not (got == 77).any()
        read_back = ops.pair_relations(*dev, vocab)        # without host copies: read back
        assert np.array_equal(read_back.cpu().numpy(), got)
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


def test_a_stale_device_row_becomes_a_padding_row(cuda):
    """The host copies pass, the device buffer disagrees (as under a replayed graph whose buffer was not refreshed): a row
    whose device `other` is itself, negative, or at or beyond the count is padding; nothing is indexed with it."""
    from canonicalsg2im_amd import ops
    vocab = pc.vocab()
    _, _, g = pc.case_arrays(0, 0)
    O = g["other"].shape[1]
    boxes = np.ascontiguousarray(g["boxes"][:, :O])
    stale = g["other"].copy()
    stale[4, 0], stale[4, 3], stale[3, 1], stale[2, 2] = 0, 8, 2 ** 31 - 1, -5
    got = _pairs(ops, cuda, vocab, boxes, _row_counts(g), g["other"], g["flip"], 0, stale_other=stale)
    want = g["rows"].copy()
    for where in ((4, 0), (4, 3), (3, 1), (2, 2)):
        want[where] = [0, vocab["pred_name_to_idx"]["__padding__"], 0]
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------- 2. the graph
def _graph_inputs(cuda, g):
    B, O = g["other"].shape
    boxes = torch.from_numpy(np.array(g["boxes"])).to(cuda)
    centers = boxes[..., :2] + 0.5 * boxes[..., 2:]
    other = torch.from_numpy(np.concatenate([g["other"], np.full((B, 1), -1, np.int32)], 1))
    flip = torch.from_numpy(np.concatenate([g["flip"], np.zeros((B, 1), np.uint8)], 1))
    return torch.from_numpy(g["objs"]).to(cuda), boxes, centers, torch.from_numpy(g["n"] + 1), other, flip


@pytest.mark.parametrize("case", pc.cases(), ids=pc.case_id)
def test_canonical_triplets_over_the_pairs_equal_the_reference_collate(cuda, case):
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    s, group, g = pc.case_arrays(*case)
    vocab = pc.vocab()
    objs, boxes, centers, n, other, flip = _graph_inputs(cuda, g)
    kw = {}
    if s["learned_converse"]:
        kw = {"learned_converse": True, "converse_weights": g["weights"],
              "uniforms": pc.golden_uniforms(group, group["converse_draws"])}
    state = np.random.get_state()[1].copy()
    trip, conv, tt = canonical_triplets(objs, boxes, centers, n, vocab, learned_transitivity=bool(s["learned_transitivity"]),
                                        pairs=(other.to(cuda), flip.to(cuda)), pairs_host=(other, flip),
                                        use_converse=bool(s["use_converse"]), **kw)
    torch.cuda.synchronize()
    assert trip.dtype == tt.dtype == torch.int64 and conv.dtype == torch.float32 and list(trip.shape) == group["triplets"]
    assert np.array_equal(trip.cpu().numpy(), g["triplets"]) and np.array_equal(tt.cpu().numpy(), g["tt"])
    assert np.array_equal(conv.cpu().numpy(), g["conv"]) and np.array_equal(np.random.get_state()[1], state)
    if case[1] == 2:                                        # host tensors alone, and device tensors alone: the same graph
        for pairs in ((other, flip), (other.to(cuda), flip.to(cuda))):
            again = canonical_triplets(objs, boxes, centers, n, vocab, learned_transitivity=bool(s["learned_transitivity"]),
                                       pairs=pairs, use_converse=bool(s["use_converse"]), **kw)
            assert all(torch.equal(a, b) for a, b in zip(again, (trip, conv, tt)))


def test_learned_converse_draws_from_numpys_global_stream_by_default(cuda):
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    s, group, g = pc.case_arrays(5, 0)
    assert s["learned_converse"] and group["converse_draws"] > 0
    objs, boxes, centers, n, other, flip = _graph_inputs(cuda, g)
    np.random.seed(group["seed"])
    trip, conv, tt = canonical_triplets(objs, boxes, centers, n, pc.vocab(), learned_transitivity=True, learned_converse=True,
                                        converse_weights=g["weights"], pairs=(other, flip))
    assert np.array_equal(trip.cpu().numpy(), g["triplets"]) and np.array_equal(conv.cpu().numpy(), g["conv"])
    assert np.array_equal(tt.cpu().numpy(), g["tt"])


def test_pairs_are_refused_with_triplets_or_without_boxes(cuda):
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    _, _, g = pc.case_arrays(0, 2)
    objs, boxes, centers, n, other, flip = _graph_inputs(cuda, g)
    with pytest.raises(ValueError, match="pairs needs boxes and obj_centers, and no `triplets`"):
        canonical_triplets(objs, boxes, centers, n, pc.vocab(), pairs=(other, flip), triplets=torch.zeros((2, 0, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="pairs must be two .B, O. = .2, 3. tensors"):
        canonical_triplets(objs, boxes, centers, n, pc.vocab(), pairs=(other[:, :2], flip[:, :2]))
    o = other.clone()
    o[1, 0] = 0                                             # other[b][i] == i: refused on the host, before any launch
    with pytest.raises(RuntimeError, match="sample 1 row 0: other = 0, another row of .0, 2."):
        canonical_triplets(objs, boxes, centers, n, pc.vocab(), pairs=(o, flip))


def _roles(vocab):
    from canonicalsg2im_amd.sg2im.data import augmented_relations
    p2i = vocab["pred_name_to_idx"]
    roles = [-1] * len(p2i)
    roles[p2i["__padding__"]], roles[p2i["__in_image__"]] = -2, -3
    for slot, name in enumerate(augmented_relations):
        roles[p2i[name]] = slot
    return (ctypes.c_int32 * len(roles))(*roles)


def test_a_corrupted_device_row_raises_and_writes_nothing_out_of_range(cuda):
    """Rows on the device cannot be checked by the host.  A row naming object n_b (one past the sample's objects), a
    predicate outside the vocabulary or __padding__ is dropped by the packing kernel: counts[b][0] is negative after
    _build_dev and after _close, the other samples' counts are theirs, the guard words behind the workspace and the
    bit matrices of the refused sample are untouched by it, and canonical_triplets raises instead of emitting."""
    from canonicalsg2im_amd import _lib
    from canonicalsg2im_amd.sg2im.data import base_dataset as bd
    vocab = pc.vocab()
    p2i = vocab["pred_name_to_idx"]
    s, _, g = pc.case_arrays(2, 0)                          # learned_transitivity 1, group 0
    objs, boxes, centers, n, other, flip = _graph_inputs(cuda, g)
    B, O = objs.shape
    P = len(p2i)
    good = torch.from_numpy(np.concatenate([g["rows"], np.tile([[[0, p2i["__padding__"], 0]]], (B, 1, 1))], 1)).to(cuda)
    rel_counts = torch.from_numpy(_row_counts(g))
    n_b = int(g["n"][3]) + 1                                # sample 3: 5 objects and __image__, rows 0 .. 5
    for bad_row in ([n_b, p2i["__left of__"], 0], [0, p2i["__above__"], n_b], [0, P, 1], [0, -1, 1], [1, p2i["__padding__"], 0],
                    [-1, p2i["__below__"], 0], [2 ** 40, p2i["__below__"], 0]):
        rel = good.clone()
        rel[3, 2] = torch.tensor(bad_row, device=cuda)
        with pytest.raises(RuntimeError, match="sample 3 has a sampled row .* no graph was written"):
            bd._canonical_general(objs, None, None, n, vocab, 0, True, True, False, None, None, None, rel_dev=rel,
                                  rel_counts=rel_counts)
    state = np.random.get_state()[1].copy()
    with pytest.raises(RuntimeError, match="sample 3 has a sampled row"):     # learned_converse: refused before a number is drawn
        bd._canonical_general(objs, None, None, n, vocab, 0, True, True, True, np.zeros((P, P), np.float32), None, None,
                              rel_dev=rel, rel_counts=rel_counts)
    assert np.array_equal(np.random.get_state()[1], state)
    # the entries themselves, over a workspace with guard words behind it
    nbytes = _lib.lib.csg_canon_general_workspace(B, P, O)
    guard = 4096
    ws = torch.full(((nbytes + 7) // 8 + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=cuda)
    counts = torch.full((B, 2), 99, dtype=torch.int64, device=cuda)
    rel = good.clone()
    rel[3, 2] = torch.tensor([n_b, p2i["__left of__"], n_b + 200], device=cuda)
    n_host = n.to(torch.int64).contiguous()
    roles = _roles(vocab)

    def build(r):
        _lib.check(_lib.lib.csg_canon_general_build_dev(_lib.ptr(objs), None, None, ctypes.c_void_p(n_host.data_ptr()), B, O,
                                                        _lib.ptr(r), ctypes.c_void_p(rel_counts.data_ptr()), O, roles, P, 0, 1,
                                                        _lib.ptr(ws), nbytes, _lib.ptr(counts), _lib.stream()), "build_dev")
        first = counts.cpu().clone()
        _lib.check(_lib.lib.csg_canon_general_close(B, roles, P, 1, _lib.ptr(ws), nbytes, _lib.ptr(counts), _lib.stream()), "close")
        torch.cuda.synchronize()
        return first, counts.cpu().clone()

    first, closed = build(rel)
    assert bool((ws[(nbytes + 7) // 8:] == 0x5A5A5A5A5A5A5A5A).all())
    assert first[3, 0] < 0 and closed[3, 0] < 0 and bool((first[[0, 1, 2, 4], 0] >= 0).all())
    first_ok, closed_ok = build(good)
    assert bool((closed_ok >= 0).all()) and bool((ws[(nbytes + 7) // 8:] == 0x5A5A5A5A5A5A5A5A).all())
    assert torch.equal(closed[[0, 1, 2, 4]], closed_ok[[0, 1, 2, 4]])        # the other samples' counts are theirs
    assert int(closed_ok.sum(1).max()) == g["triplets"].shape[1]
    missing = int(closed_ok[3, 0]) - int(-1 - closed[3, 0])                 # the dropped row alone (0 if it had a twin)
    assert missing in (0, 1)
    # refusals of the entry itself: on the host, before anything is enqueued
    for kw, text in (({"boxes": _lib.ptr(boxes)}, "boxes and centers must be NULL"), ({"rel_counts": None}, "null argument"),
                     ({"O": 257}, "at most 256 objects per sample .got 257.")):
        args = {"boxes": None, "rel_counts": ctypes.c_void_p(rel_counts.data_ptr()), "O": O}
        args.update(kw)
        counts.fill_(99)
        with pytest.raises(RuntimeError, match=text):
            _lib.check(_lib.lib.csg_canon_general_build_dev(_lib.ptr(objs), args["boxes"], None, ctypes.c_void_p(n_host.data_ptr()),
                                                            B, args["O"], _lib.ptr(good), args["rel_counts"], O, roles, P, 0, 1,
                                                            _lib.ptr(ws), nbytes, _lib.ptr(counts), _lib.stream()), "build_dev")
        torch.cuda.synchronize()
        assert bool((counts == 99).all())
    too_many = rel_counts.clone()
    too_many[1] = O + 1
    with pytest.raises(RuntimeError, match="rel_counts.1. = %d outside .0, %d." % (O + 1, O)):
        _lib.check(_lib.lib.csg_canon_general_build_dev(_lib.ptr(objs), None, None, ctypes.c_void_p(n_host.data_ptr()), B, O,
                                                        _lib.ptr(good), ctypes.c_void_p(too_many.data_ptr()), O, roles, P, 0, 1,
                                                        _lib.ptr(ws), nbytes, _lib.ptr(counts), _lib.stream()), "build_dev")
    assert _lib.lib.csg_version() >= 116


# ------------------------------------------------------------------------------------------------- 3. the dataset
def _args(vocab, extra=()):
    from canonicalsg2im_amd import train as T
    return T.make_opt(vocab, MODEL + list(extra))


def _dataset(folder, **kw):
    from canonicalsg2im_amd.sg2im.data.coco import CocoSceneGraphDataset
    ann = os.path.join(folder[0], "MSCoco", "annotations")
    return CocoSceneGraphDataset(folder[1], os.path.join(ann, "instances_train2017.json"), os.path.join(ann, "stuff_train2017.json"),
                                 image_size=(64, 64), min_objects=1, **kw)


@pytest.mark.parametrize("si", range(6), ids=pc.setting_id)
def test_whole_batch_equals_the_reference_collate(cuda, folder, si):
    """CocoPairsBatchBuilder.build over the tiny folder, drawing from the seed the reference drew from: objects and boxes with
    the __image__ row, triplets, triplet types and converse counts are the reference's collate output; the images are the
    host pipeline's."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import folder_builder
    from canonicalsg2im_amd.sg2im.data.coco import CocoPairsBatchBuilder
    s, group, g = pc.case_arrays(si, 0)
    ds = _dataset(folder, include_relationships=bool(s["include_relationships"]), use_converse=bool(s["use_converse"]))
    assert ds.vocab == pc.vocab() and len(ds) == 5
    opt = _args(ds.vocab, ["--learned_transitivity", str(s["learned_transitivity"]), "--use_converse", str(s["use_converse"]),
                           "--include_relationships", str(s["include_relationships"]),
                           "--learned_converse", str(s["learned_converse"])])
    trainer = None
    if s["learned_converse"]:                               # the loader reads the model's converse weights: give it the golden's
        from canonicalsg2im_amd.sg2im.model import get_conv_converse
        torch.manual_seed(1)
        trainer = T.Trainer(opt, cuda)
        want_w = torch.from_numpy(np.array(g["weights"])).to(cuda)
        with torch.no_grad():
            trainer.model.sg_to_layout.module.converse_candidates_weights.copy_(torch.triu(want_w) - torch.diag(torch.diag(want_w) / 2))
        assert torch.equal(get_conv_converse(trainer.model), want_w)
    builder = folder_builder(ds, opt, trainer, cuda, rng=random.Random(group["seed"]))
    assert isinstance(builder, CocoPairsBatchBuilder) and builder.num_workers == 2
    pending = builder.start(list(range(5)))
    assert np.array_equal(pending.other.numpy(), g["other"]) and np.array_equal(pending.flip.numpy(), g["flip"])
    assert pending.counts.tolist() == g["n"].tolist() and tuple(pending.desc.shape) == (5, 3)
    np.random.seed(group["seed"])
    imgs, objs, boxes, triplets, conv_counts, ttype, masks, ids = builder.finish(pending)
    torch.cuda.synchronize()
    builder.close()
    assert masks is None and ids.tolist() == [11, 12, 13, 14, 15]
    assert objs.dtype == torch.int64 and np.array_equal(objs.cpu().numpy()[..., 0], g["objs"])
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), g["boxes"].view(np.uint32))
    assert triplets.dtype == torch.int64 and list(triplets.shape) == group["triplets"]
    assert np.array_equal(triplets.cpu().numpy(), g["triplets"]) and np.array_equal(ttype.cpu().numpy(), g["tt"])
    assert np.array_equal(conv_counts.cpu().numpy(), g["conv"])
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (5, 3, 64, 64)
    for b in range(5):
        assert torch.equal(imgs[b].cpu(), folder[2][b]), "picture %d" % b


def test_a_step_on_built_batches_and_the_draws_ignore_the_loader_threads(cuda, folder):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    ds = folder_dataset(build_parser().parse_args(["--dataroot", folder[0], "--image_size", "64,64", "--min_objects", "1"]), "train")
    assert len(ds) == 5 and ds.image_dir == folder[1]
    opt = _args(ds.vocab, ["--learned_transitivity", "1"])
    torch.manual_seed(4)
    trainer = T.Trainer(opt, cuda)
    lists = [[3, 0, 2, 1, 4], [1, 2, 0, 3, 4]]
    built = {}
    for workers in (1, 3):
        opt.loader_num_workers = workers
        builder = folder_builder(ds, opt, trainer, cuda, rng=random.Random(5))
        assert builder.num_workers == workers
        built[workers] = list(builder.batches(lists))
        torch.cuda.synchronize()
        assert builder.steps == 2
        builder.close()
    for one, three in zip(built[1], built[3]):               # the stream is consumed in batch order, by the consumer's thread
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(one, three))
    assert built[1][0][7].tolist() == [14, 11, 13, 12, 15] and tuple(built[1][0][1].shape) == (5, 9, 1)
    G, D = trainer.step(built[1][0])
    for k, val in list(G.items()) + list(D.items()):
        assert bool(torch.isfinite(val).all()), k
    state = random.getstate()                               # the default stream is the builder's own, seeded from the rank
    one, two = (folder_builder(ds, opt, trainer, cuda) for _ in range(2))
    assert one.rng is not two.rng and one.rng.random() == two.rng.random() and random.getstate() == state
    one.close()
    two.close()


# ------------------------------------------------------------------------------------------------- 4. command lines
def test_command_lines_train_and_validate_on_the_folder(cuda, folder, tmp_path, capsys):
    from canonicalsg2im_amd.scripts import evaluate as val_cli, train as train_cli
    root, image_dir = folder[:2]
    out = str(tmp_path / "out")
    common = [a for a in MODEL] + ["--dataroot", root]
    train_cli.main(common + ["--num_iterations", "2", "--print_every", "1", "--output_dir", out, "--checkpoint_every", "2",
                             "--learned_transitivity", "1"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: 5 pictures of %s, 2 loader threads" % image_dir in lines, lines
    assert sum(l.startswith("loader: ") and l.endswith("of 2 steps waited for their batch") for l in lines) == 1
    assert sum(l.startswith("t = ") for l in lines) == 2
    train_cli.main(MODEL[:-2] + ["--dataroot", str(tmp_path / "nowhere"), "--num_iterations", "1", "--print_every", "1"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: seeded synthetic batches (coco shapes)" in lines and not any(l.startswith("loader:") for l in lines)
    val_cli.main(common + ["--checkpoint_name", os.path.join(out, "itr_2.pt"), "--num_val_samples", "5"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: 5 pictures of %s" % image_dir.replace("train2017", "val2017") in lines
    val = [l for l in lines if l.startswith("Iter: 2, ")]
    assert len(val) == 2 and "GT VAL avg_iou:" in val[0] and val[1].startswith("Iter: 2, VAL avg_iou:"), lines
