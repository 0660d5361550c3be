"""The unpacked Visual Genome dataset on a real MI355X: the small-graph kernels (csrc/canon_small.hip, csg_canon_small_*)
against the numpy restatement of tests/vg_unpacked_cases.py (which tests/test_vg_unpacked_cases.py pins to the reference on
the CPU), against the reference's recorded samples (tests/golden/vg_unpacked.npz) and against the general kernels on the
same rows; then the folder dataset that feeds them, a trainer step and the sampler on its vocabulary.

Every output is an integer or an integer-valued float: equality everywhere."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import vg_unpacked_cases as uc

pytestmark = pytest.mark.gpu

MODEL = ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--batch_size", "4", "--no_vgg_loss", "--use_img_disc", "1",
         "--gconv_hidden_dim", "64", "--gconv_dim", "32", "--dataset", "vg", "--loader_num_workers", "2"]
# P -> (id of __in_image__, id of __padding__): the meta ids anywhere; at P = 47 and 256 the id P - 1 is an ordinary predicate
META = {3: (0, 2), 47: (5, 20), 256: (0, 100)}
_CACHE = {}


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("vguroot"))
    base = uc.write_folder(root)
    uc.write_folder(root, split="val")
    return root, base


def _vocab(P):
    """A vocabulary of P predicates without location predicates, the objects of the golden's."""
    in_image, pad = META[P]
    names = ["p%d" % i for i in range(P)]
    names[in_image], names[pad] = "__in_image__", "__padding__"
    v = uc.dataset_vocab()
    v["pred_idx_to_name"] = names
    v["pred_name_to_idx"] = {nm: i for i, nm in enumerate(names)}
    return v


def _shared(P):
    """(vocab, cases, converse weights and uniforms per case, {(case, trans, conv): restatement}) of a vocabulary size:
    computed once, shared by the tests, never written to."""
    if P not in _CACHE:
        vocab = _vocab(P) if P in META else P
        cases = uc.build_cases(vocab)
        conv = {name: uc.converse_operands(vocab, c["rel"]) for name, c in cases.items()}
        want = {}
        for name, c in cases.items():
            for trans in (False, True):
                want[name, trans, False] = uc.annotated_batch(c["objs"], c["n"], c["rel"], vocab, trans, c["include_dummies"])
                want[name, trans, True] = uc.annotated_batch(c["objs"], c["n"], c["rel"], vocab, trans, c["include_dummies"],
                                                             True, conv[name][0], conv[name][1])
        _CACHE[P] = (vocab, cases, conv, want)
    return _CACHE[P]


def _run(c, vocab, trans, conv=None, fn=None, **kw):
    from canonicalsg2im_amd.sg2im.data import annotated_triplets
    objs, rel = torch.from_numpy(np.array(c["objs"])).cuda(), torch.from_numpy(np.array(c["rel"]))
    if conv is not None:
        kw.update(learned_converse=True, converse_weights=conv[0], uniforms=conv[1])
    if fn is None:
        out = annotated_triplets(objs, torch.from_numpy(np.array(c["n"])), vocab, rel.cuda(), rows_host=rel,
                                 learned_transitivity=trans, include_dummies=c["include_dummies"], **kw)
    else:
        out = fn(objs, None, None, torch.from_numpy(np.array(c["n"])), vocab, triplets=rel, learned_transitivity=trans,
                 include_dummies=c["include_dummies"], **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


# ------------------------------------------------------------------------------------------------- 1. the kernels
def test_the_cases_are_the_cases_they_are_meant_to_be():
    vocab, cases, conv, want = _shared(47)
    assert len(cases) == 10 and all(c["objs"].shape == (3, 64) for c in cases.values())
    assert cases["n64_object63"]["n"][0] == 64 and (cases["n64_object63"]["rel"][0][:, [0, 2]] == 63).any()
    assert cases["image_alone"]["n"][1] == 1 and want["image_alone", True, False][2][1] == 0
    assert want["no_rows", False, False][2][0] == 11                      # the dummies alone
    t, tt, counts, _ = want["chain", True, False]
    assert int((tt[1] == 1).sum()) == 1891 and counts[1] == 62 + 63 + 1891
    t, tt, _, _ = want["cycle", True, False]
    assert ((tt == 1) & (t[..., 0] == t[..., 2])).any()                   # path() marks i -> i on a cycle
    assert (cases["last_predicate"]["rel"][..., 1] == 46).any() and 46 not in META[47]
    assert want["no_dummies", False, False][2].tolist()[2] == 0 and not cases["no_dummies"]["include_dummies"]
    assert (cases["no_image_id"]["objs"][0, :6] != 0).all()
    w, u = conv["chain"]
    assert want["chain", False, True][3].sum() == uc.draw_count(cases["chain"]["rel"], vocab) > 100


@pytest.mark.parametrize("trans", [False, True], ids=["trans0", "trans1"])
@pytest.mark.parametrize("P", [3, 47, 256])
def test_every_case_equals_the_restatement_and_itself(cuda, P, trans):
    """The ten graphs, with and without converse draws (given uniforms, one exactly a threshold, one in "none"): triplets,
    types and conv_counts equal the restatement's, and a second call gives the same bytes."""
    vocab, cases, conv, want = _shared(P)
    for name, c in cases.items():
        for cv in (None, conv[name]):
            t, cc, tt = _run(c, vocab, trans, cv)
            wt, wtt, counts, wcc = want[name, trans, cv is not None]
            print("P %d %s trans %d conv %d: T = %d, %d originals and extras, %d draws" % (
                P, name, trans, cv is not None, t.shape[1], int(counts.sum()), int(wcc.sum())))
            assert t.dtype == np.int64 and t.shape == wt.shape and np.array_equal(t, wt), (name, cv is not None)
            assert np.array_equal(tt, wtt), name
            assert cc.dtype == np.float32 and cc.shape == (3, P, P + 1) and np.array_equal(cc, wcc), name
            t2, cc2, tt2 = _run(c, vocab, trans, cv)
            assert t.tobytes() == t2.tobytes() and tt.tobytes() == tt2.tobytes() and cc.tobytes() == cc2.tobytes(), name


@pytest.mark.parametrize("trans", [False, True], ids=["trans0", "trans1"])
def test_equal_to_the_general_kernels_on_a_vocabulary_with_location_predicates(cuda, trans):
    """make_vocab("vg") has the six location predicates: canonical_triplets takes its general kernels for the same rows, and
    the small-graph kernels serve the vocabulary the same way, bit for bit."""
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    from canonicalsg2im_amd.synth import make_vocab
    if "vg" not in _CACHE:
        _CACHE["vg"] = None
        vocab = make_vocab("vg")
        cases = uc.build_cases(vocab)
        _CACHE["vg"] = (vocab, cases, {name: uc.converse_operands(vocab, c["rel"]) for name, c in cases.items()})
    vocab, cases, conv = _CACHE["vg"]
    assert "__left of__" in vocab["pred_name_to_idx"]
    for name, c in cases.items():
        for cv in (None, conv[name]):
            got = _run(c, vocab, trans, cv)
            want = _run(c, vocab, trans, cv, fn=canonical_triplets)
            for a, b, what in zip(got, want, ("triplets", "conv_counts", "triplet_type")):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, what)


def test_two_launches_and_none_of_the_general_ones(cuda):
    from canonicalsg2im_amd import _lib
    vocab, cases, conv, _ = _shared(47)
    _run(cases["chain"], vocab, True, conv["chain"])                      # nothing is built on first use under the timer
    _lib.prof_enable(1)
    _lib.prof_reset()
    try:
        _run(cases["chain"], vocab, True, conv["chain"])
        seen = _lib.prof_read()
        assert seen["canon_small_build"][1] == 1 and seen["canon_small_emit"][1] == 1
        assert "canon_build" not in seen and "canon_emit" not in seen
    finally:
        _lib.prof_enable(0)
        _lib.prof_reset()


def _abi_call(objs, n, rel, P, ids, short=0, rel_dev=None):
    """csg_canon_small_build on prepared buffers -> (rc, counts after the call, workspace after the call)."""
    from canonicalsg2im_amd._lib import lib, ptr, stream
    B, O = objs.shape
    R = rel.shape[1]
    nbytes = lib.csg_canon_small_workspace(B, min(P, 256))
    ws = torch.full((nbytes // 8 + 1,), 7, dtype=torch.int64, device="cuda")
    counts = torch.full((B, 2), -5, dtype=torch.int64, device="cuda")
    objs_d = torch.from_numpy(np.array(objs)).cuda()
    n_c = np.ascontiguousarray(n, np.int64)
    rel_c = np.ascontiguousarray(rel, np.int64)
    n_d = torch.from_numpy(n_c).cuda()
    rel_d = torch.from_numpy(rel_c if rel_dev is None else np.ascontiguousarray(rel_dev, np.int64)).cuda()
    rc = lib.csg_canon_small_build(ptr(objs_d), ptr(n_d), n_c.ctypes.data_as(ctypes.c_void_p), B, O, ptr(rel_d),
                                   rel_c.ctypes.data_as(ctypes.c_void_p), R, P, ids[1], ids[0], 0, 1, 1, None, None, None, 0,
                                   None, ptr(ws), nbytes - short, ptr(counts), stream())
    torch.cuda.synchronize()
    return rc, counts.cpu(), ws.cpu()


def test_bad_inputs_are_refused_before_any_launch(cuda):
    from canonicalsg2im_amd._lib import last_error
    from canonicalsg2im_amd.sg2im.data import annotated_triplets, canonical_triplets
    vocab, cases, _, _ = _shared(47)
    c = cases["duplicates_self"]
    objs, n, rel = np.array(c["objs"]), np.array(c["n"]), np.array(c["rel"])
    rc, counts, _ = _abi_call(objs, n, rel, 47, META[47])
    assert rc == 0 and (counts[:, 0] > 0).all() and (counts[:, 1] > 0).any()
    wide = np.zeros((3, 80), np.int64)
    wide[:, :64] = objs
    many = n.copy()
    many[1] = 65
    bad_obj = rel.copy()
    bad_obj[0, 0, 2] = n[0]                                               # object index == n_objs[0]
    bad_pred = rel.copy()
    bad_pred[2, 0, 1] = 47                                                # predicate id == P
    neg = rel.copy()
    neg[1, 1, 0] = -1
    for what, kw, code, msg in (("rows", dict(objs=wide, n=many), -2, "at most 64 rows per sample"),
                                ("object", dict(rel=bad_obj), -1, "outside"), ("predicate", dict(rel=bad_pred), -1, "outside"),
                                ("negative", dict(rel=neg), -1, "outside"), ("workspace", dict(short=8), -1, "workspace too small"),
                                ("predicates", dict(P=300), -2, "at most 256 predicates"),
                                ("meta", dict(ids=(5, 5)), -1, "two ids")):
        a = dict(objs=objs, n=n, rel=rel, P=47, ids=META[47])
        a.update(kw)
        rc, counts, ws = _abi_call(**a)
        assert rc == code and msg in last_error(), (what, rc, last_error())
        assert (counts == -5).all() and (ws == 7).all(), what             # nothing was enqueued
    args = (torch.from_numpy(wide).cuda(), torch.from_numpy(many), vocab, torch.from_numpy(rel))
    with pytest.raises(RuntimeError, match="at most 64 rows per sample"):
        annotated_triplets(*args)
    with pytest.raises(RuntimeError, match="at most 64 rows per sample"):   # where today's KeyError: '__below__' was
        canonical_triplets(args[0], None, None, many, vocab, triplets=rel)
    # a device copy that is not the host's rows: the kernel indexes nothing with the row and marks the sample
    rc, counts, _ = _abi_call(objs, n, rel, 47, META[47], rel_dev=bad_obj)
    assert rc == 0 and counts[0, 0] < 0 and (counts[1:, 0] > 0).all()
    with pytest.raises(RuntimeError, match="sample 0 on the device are not the rows the host holds"):
        annotated_triplets(torch.from_numpy(objs).cuda(), torch.from_numpy(n), vocab, torch.from_numpy(bad_obj).cuda(),
                           rows_host=torch.from_numpy(rel))


# ------------------------------------------------------------------------------------------------- 2. the golden
@pytest.mark.parametrize("si", range(10), ids=uc.setting_id)
def test_golden_settings_equal_the_reference(cuda, folder, si):
    """The reference's own samples: its objects, the rows `select` keeps under its seed, its draws from numpy's global
    stream -> its triplets, types and conv_counts; the stream advances by exactly its draws."""
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    from canonicalsg2im_amd.sg2im.data.vg import VGSceneGraphDataset
    meta, g = uc.golden()
    s = meta["settings"][si]
    base = folder[1]
    ds = VGSceneGraphDataset(os.path.join(base, "train.npz"), base, os.path.join(base, "vocab.json"), image_size=(64, 64),
                             max_objects=s["max_objects"], use_orphaned_objects=bool(s["use_orphaned_objects"]),
                             include_relationships=bool(s["include_relationships"]))
    vocab = ds.vocab
    P = len(vocab["pred_idx_to_name"])
    rel = uc.padded_rel(uc.select_all(ds, si), vocab["pred_name_to_idx"]["__padding__"])
    c = {"objs": g["s%d_objs" % si].astype(np.int64), "n": g["s%d_n" % si], "rel": rel, "include_dummies": True}
    kw = {}
    if s["learned_converse"]:
        kw = {"learned_converse": True, "converse_weights": g["s%d_weights" % si]}
        np.random.seed(s["seed"])
        np.random.random_sample(s["draws"])
        expect_next = np.random.random_sample()
    np.random.seed(s["seed"])
    t, cc, tt = _run(c, vocab, bool(s["learned_transitivity"]), fn=canonical_triplets, **kw)   # routed: no location predicate
    assert t.shape == tuple(s["triplets"]) and np.array_equal(t, g["s%d_triplets" % si].astype(np.int64))
    assert np.array_equal(tt, g["s%d_tt" % si].astype(np.int64))
    assert np.array_equal(cc, uc.golden_conv(g, si, len(c["n"]), P)) and int(cc.sum()) == s["draws"]
    if s["learned_converse"]:
        assert np.random.random_sample() == expect_next


# ------------------------------------------------------------------------------------------------- 3. the dataset
def _args(vocab, extra=()):
    from canonicalsg2im_amd import train as T
    return T.make_opt(vocab, MODEL + list(extra))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("si", [1, 3, 4, 5], ids=uc.setting_id)
def test_whole_batch_equals_the_reference_collate(cuda, folder, si):
    """The dataset of the command line, its builder drawing from the seeded `random` module as the reference did: the fields
    of the 8-tuple are the reference's collate output."""
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    from canonicalsg2im_amd.sg2im.data.vg import VGAnnotatedBatchBuilder
    meta, g = uc.golden()
    s = meta["settings"][si]
    flags = ["--max_objects", str(s["max_objects"]), "--vg_use_orphaned_objects", str(s["use_orphaned_objects"]),
             "--include_relationships", str(s["include_relationships"]), "--learned_transitivity", str(s["learned_transitivity"])]
    ds = folder_dataset(build_parser().parse_args(["--dataset", "vg", "--dataroot", folder[0], "--image_size", "64,64"] + flags),
                        "train")
    opt = _args(ds.vocab, flags)
    builder = folder_builder(ds, opt, None, cuda, rng=random)
    assert isinstance(builder, VGAnnotatedBatchBuilder)
    random.seed(s["seed"])
    pending = builder.start(s["samples"])
    assert pending.rel.shape[2] == 3 and not pending.rel.is_cuda and pending.rel.dtype == torch.int64
    imgs, objs, boxes, triplets, conv_counts, ttype, masks, ids = builder.finish(pending)
    torch.cuda.synchronize()
    builder.close()
    P = len(ds.vocab["pred_idx_to_name"])
    assert masks is None and ids.tolist() == meta["image_ids"]
    assert objs.dtype == torch.int64 and np.array_equal(objs.cpu().numpy()[..., 0], g["s%d_objs" % si].astype(np.int64))
    assert _same_bits(boxes.cpu().numpy(), g["s%d_boxes" % si])
    assert triplets.dtype == torch.int64 and tuple(triplets.shape) == tuple(s["triplets"])
    assert np.array_equal(triplets.cpu().numpy(), g["s%d_triplets" % si].astype(np.int64))
    assert np.array_equal(ttype.cpu().numpy(), g["s%d_tt" % si].astype(np.int64))
    assert conv_counts.dtype == torch.float32 and tuple(conv_counts.shape) == (4, P, P + 1) and not bool(conv_counts.any())
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (4, 3, 64, 64) and bool(torch.isfinite(imgs).all())


def test_a_trainer_step_and_the_sampler_on_the_datasets_vocabulary(cuda, folder):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.scripts.train import build_parser, folder_builder, folder_dataset
    ds = folder_dataset(build_parser().parse_args(["--dataset", "vg", "--dataroot", folder[0], "--image_size", "64,64"]), "train")
    flags = ["--learned_transitivity", "1", "--learned_converse", "1"]
    opt = _args(ds.vocab, flags)
    torch.manual_seed(4)
    trainer = T.Trainer(opt, cuda)
    builder = folder_builder(ds, opt, trainer, cuda, rng=random.Random(5))
    np.random.seed(6)
    batch = builder.build([3, 0, 2, 1])
    builder.close()
    assert batch[7].tolist() == [7, 100, 2317, 101] and tuple(batch[1].shape) == (4, 11, 1) and bool(batch[4].any())
    G, D = trainer.step(batch)
    for k, val in list(G.items()) + list(D.items()):
        assert bool(torch.isfinite(val).all()), k
    names, preds = ds.vocab["object_idx_to_name"], ds.vocab["pred_idx_to_name"]
    graphs = [{"objects": [names[3], names[9], names[4]], "relationships": [[0, preds[1], 1], [1, preds[1], 2]]},
              {"objects": [names[7], names[2]], "relationships": [[1, preds[5], 0]]}]
    sampler = Sampler(opt, cuda)
    imgs, boxes, _ = sampler.generate_from_graphs(graphs)                 # a vocabulary without location predicates
    torch.cuda.synchronize()
    assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == (2, 3, 64, 64) and tuple(boxes.shape)[:2] == (2, 4)


def test_command_lines_train_validate_and_sample_on_the_folder(cuda, folder, tmp_path, capsys):
    from canonicalsg2im_amd.scripts import evaluate as val_cli, sample as sample_cli, train as train_cli
    root, base = folder
    out = str(tmp_path / "out")
    common = list(MODEL) + ["--dataroot", root]
    train_cli.main(common + ["--num_iterations", "2", "--print_every", "1", "--output_dir", out, "--checkpoint_every", "2",
                             "--val_every", "2", "--num_val_samples", "4"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: 4 pictures of %s, 2 loader threads" % base in lines, lines
    assert sum(l.startswith("t = ") for l in lines) == 2 and sum(l.startswith("Iter: 2, ") for l in lines) == 2
    train_cli.main(list(MODEL) + ["--dataroot", str(tmp_path / "nowhere"), "--num_iterations", "1", "--print_every", "1"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: seeded synthetic batches (vg shapes)" in lines and not any(l.startswith("loader:") for l in lines)
    ck = os.path.join(out, "itr_2.pt")
    val_cli.main(common + ["--checkpoint_name", ck, "--num_val_samples", "4"])
    lines = capsys.readouterr().out.splitlines()
    assert "data: 4 pictures of %s" % base in lines
    assert len([l for l in lines if l.startswith("Iter: 2, ")]) == 2, lines
    pics = str(tmp_path / "pics")
    sample_cli.main(common + ["--checkpoint_name", ck, "--split", "val", "--output_dir", pics])
    assert "data: 4 pictures of %s" % base in capsys.readouterr().out.splitlines()
    written = sorted(os.path.relpath(os.path.join(d, f), pics) for d, _, files in os.walk(pics) for f in files if f.endswith(".png"))
    sets = ("gt", "generation/gt_box_gt_mask", "generation/pred_box_pred_mask", "layout/gt", "layout/pred")
    assert written == sorted("%s/%d.png" % (k, i) for k in sets for i in (100, 101, 2317, 7)), written
