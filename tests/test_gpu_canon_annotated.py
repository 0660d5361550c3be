"""Canonical graphs with annotated relationships on any vocabulary (csrc/canon.hip, csg_canon_general_*) on a real
MI355X: bit-exact against the reference's own outputs (tests/golden/canon_annotated.npz), against the numpy restatement
(tests/canon_annotated.py) on dense seeded batches, and against the location-only fixtures when the general kernels are
forced onto them."""
import ctypes

import numpy as np
import pytest
import torch

import canon_annotated as ca
from canonicalsg2im_amd.synth import annotated_relations, make_vocab
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _run(objs, boxes, cen, n, vocab, **kw):
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    t, cc, tt = canonical_triplets(torch.from_numpy(objs).cuda(), torch.from_numpy(boxes).cuda(),
                                   torch.from_numpy(cen).cuda(), torch.from_numpy(n), vocab, **kw)
    return t.cpu().numpy(), cc.cpu().numpy(), tt.cpu().numpy()


def _scene(rng, sizes, vocab, rel=True):
    """Real objects per sample in `sizes`, the __image__ object after them (id 0, as padding: n_objs tells them apart),
    annotated rows from synth.annotated_relations padded with __padding__."""
    B, O = len(sizes), max(sizes) + 1
    objs = np.zeros((B, O), np.int64)
    boxes = -np.ones((B, O, 4), np.float32)
    cen = np.zeros((B, O, 2), np.float32)
    rows = []
    for b, n in enumerate(sizes):
        wh = rng.uniform(0.05, 0.6, size=(n, 2))
        xy = rng.uniform(0.0, 1.0, size=(n, 2)) * (1.0 - wh)
        bx = np.concatenate([xy, wh], axis=1).astype(np.float32)
        boxes[b, :n] = bx
        cen[b, :n] = bx[:, :2] + np.float32(0.5) * bx[:, 2:]
        objs[b, :n] = rng.integers(1, len(vocab["object_idx_to_name"]), size=n)
        rows.append(annotated_relations(rng, n, vocab) if rel else [])
    R = max(len(r) for r in rows)
    t = np.zeros((B, R, 3), np.int64)
    t[:, :, 1] = vocab["pred_name_to_idx"]["__padding__"]
    for b, r in enumerate(rows):
        if r:
            t[b, :len(r)] = r
    return objs, boxes, cen, np.asarray([n + 1 for n in sizes], np.int64), t


def test_annotated_vs_reference_golden():
    """Triplets, types and conv_counts bit for bit, the draws taken from numpy's global stream as the reference did."""
    meta, a = load_golden("canon_annotated")
    for ci in range(len(meta["cases"])):
        case, g, vocab = ca.fixture_case(meta, a, ci)
        kw = dict(learned_transitivity=bool(case["learned_transitivity"]), triplets=g["rel"])
        if case["learned_converse"]:
            kw.update(learned_converse=True, converse_weights=g["weights"])
        np.random.seed(case["seed"])
        t, cc, tt = _run(g["objs"], g["boxes"], g["centers"], g["n"], vocab, **kw)
        assert t.dtype == np.int64 and t.shape == g["triplets"].shape, (ci, t.shape, g["triplets"].shape)
        assert np.array_equal(t, g["triplets"]), ci
        assert np.array_equal(tt, g["tt"]), ci
        P = len(vocab["pred_name_to_idx"])
        assert cc.shape == (len(g["n"]), P, P + 1)
        if case["learned_converse"]:
            assert np.array_equal(cc, g["conv"]), ci
            np.random.seed(case["seed"])                          # the stream advanced by exactly the reference's draws
            np.random.random_sample(case["draws"])
            expect_next = np.random.random_sample()
            np.random.seed(case["seed"])
            _run(g["objs"], g["boxes"], g["centers"], g["n"], vocab, **kw)
            assert np.random.random_sample() == expect_next
        else:
            assert not cc.any()


def test_annotated_vs_restatement_dense_batches():
    """B = 48, up to 101 objects, VG vocabulary, transitivity and converse on, explicit uniforms: thousands of draws per
    sample, converse edges closing cycles (transitive self-loops)."""
    rng = np.random.default_rng(5150)
    vocab = make_vocab("vg")
    sizes = [2, 3, 100] + [int(v) for v in rng.integers(2, 101, size=45)]
    objs, boxes, cen, n, rel = _scene(rng, sizes, vocab)
    P = len(vocab["pred_name_to_idx"])
    w = rng.normal(size=(P, P)).astype(np.float32)
    w = np.triu(w) + np.triu(w).T
    u = rng.random(400000)
    t, cc, tt = _run(objs, boxes, cen, n, vocab, learned_transitivity=True, learned_converse=True, converse_weights=w,
                     uniforms=u, triplets=rel)
    to, tto, _, conv = ca.canonical_batch(objs, boxes, cen, n, rel, vocab, True, True, True, w, u)
    assert t.shape == to.shape and np.array_equal(t, to) and np.array_equal(tt, tto)
    assert np.array_equal(cc, conv.astype(np.float32)) and conv[:, :, :-1].sum() > 1000
    assert ((tt == 1) & (t[..., 0] == t[..., 2])).any()
    # without converse, both transitivity settings
    for trans in (False, True):
        t, cc, tt = _run(objs[:8], boxes[:8], cen[:8], n[:8], vocab, learned_transitivity=trans, triplets=rel[:8])
        to, tto, _, _ = ca.canonical_batch(objs[:8], boxes[:8], cen[:8], n[:8], rel[:8], vocab, trans)
        assert np.array_equal(t, to) and np.array_equal(tt, tto) and not cc.any()


@pytest.mark.parametrize("name", ["canon_graph", "canon_converse"])
def test_general_kernels_on_location_only_fixtures(name):
    """An empty (B, 0, 3) `triplets` routes the location-only fixtures through the general kernels: the same bytes."""
    meta, a = load_golden(name)
    vocab = make_vocab(meta["vocab"])
    for ci, case in enumerate(meta["cases"]):
        g = {k[len("c%d_" % ci):]: v.numpy() for k, v in a.items() if k.startswith("c%d_" % ci)}
        kw = dict(learned_transitivity=bool(case["learned_transitivity"]),
                  triplets=np.zeros((len(g["n"]), 0, 3), np.int64))
        if name == "canon_converse":
            kw.update(learned_converse=True, converse_weights=g["weights"])
            np.random.seed(case["seed"])
        t, cc, tt = _run(g["objs"], g["boxes"], g["centers"], g["n"], vocab, **kw)
        assert np.array_equal(t, g["triplets"]) and np.array_equal(tt, g["tt"]), ci
        if name == "canon_converse":
            assert np.array_equal(cc, g["conv"].astype(np.float32)), ci


def test_vg_vocabulary_converse_matches_oracle_without_annotations():
    """No `triplets`, VG vocabulary: the converse candidates are all other non-meta predicates, as oracle/canon.py (and
    scripts/graphs_utils.py:126-152) draw them — not only the five other location relations."""
    from oracle import canon
    rng = np.random.default_rng(8)
    vocab = make_vocab("vg")
    objs, boxes, cen, n, _ = _scene(rng, (2, 9, 33, 70), vocab, rel=False)
    P = len(vocab["pred_name_to_idx"])
    w = rng.normal(size=(P, P)).astype(np.float32)
    w = np.triu(w) + np.triu(w).T
    u = rng.random(50000)
    for trans in (False, True):
        t, cc, tt = _run(objs, boxes, cen, n, vocab, learned_transitivity=trans, learned_converse=True,
                         converse_weights=w, uniforms=u)
        to, tto, _, conv = canon.canonical_batch(objs, boxes, cen, n, vocab, trans, True, True, w, u)
        assert np.array_equal(t, to) and np.array_equal(tt, tto)
        assert np.array_equal(cc, conv.astype(np.float32))
        assert conv[:, :, 8:P].sum() > 0                    # converse edges into annotated-only predicates


def _abi_call(objs, boxes, cen, n, rel, vocab, O=None, roles=None):
    """csg_canon_general_build on prepared buffers; -> (rc, counts after the call, workspace after the call)."""
    from canonicalsg2im_amd._lib import lib, ptr, stream
    p2i = vocab["pred_name_to_idx"]
    P = len(p2i)
    if roles is None:
        roles = [-1] * P
        roles[p2i["__padding__"]], roles[p2i["__in_image__"]] = -2, -3
        for k, nm in enumerate(ca.AUGMENTED):
            roles[p2i[nm]] = k
    B = objs.shape[0]
    O = objs.shape[1] if O is None else O
    R = rel.shape[1]
    nbytes = lib.csg_canon_general_workspace(B, P, R)
    ws = torch.full((nbytes // 8 + 1,), 7, dtype=torch.int64, device="cuda")
    counts = torch.full((B, 2), -5, dtype=torch.int64, device="cuda")
    d = [torch.from_numpy(x).cuda() for x in (objs, boxes, cen)]
    n_c = np.ascontiguousarray(n, np.int64)
    rel_c = np.ascontiguousarray(rel, np.int64)
    rc = lib.csg_canon_general_build(ptr(d[0]), ptr(d[1]), ptr(d[2]), n_c.ctypes.data_as(ctypes.c_void_p), B, O,
                                     rel_c.ctypes.data_as(ctypes.c_void_p), None, R, (ctypes.c_int32 * P)(*roles), P, 0,
                                     1, ptr(ws), nbytes, ptr(counts), stream())
    torch.cuda.synchronize()
    return rc, counts.cpu(), ws.cpu()


def test_bad_inputs_are_refused_before_any_launch():
    from canonicalsg2im_amd._lib import last_error
    rng = np.random.default_rng(2)
    vocab = make_vocab("vg")
    objs, boxes, cen, n, rel = _scene(rng, (5, 9), vocab)
    rc, counts, _ = _abi_call(objs, boxes, cen, n, rel, vocab)
    assert rc == 0 and (counts[:, 1] == 0).all() and (counts[:, 0] > 0).all()
    bad_obj = rel.copy()
    bad_obj[0, 0, 2] = n[0]                                   # object index == n_objs[0]
    bad_pred = rel.copy()
    bad_pred[1, 0, 1] = len(vocab["pred_name_to_idx"])        # predicate id == P
    neg = rel.copy()
    neg[1, 1, 0] = -1
    roles = [-1] * len(vocab["pred_name_to_idx"])             # no location relations
    roles[0], roles[1] = -2, -3
    for what, args, kw, code, msg in (("object", bad_obj, {}, -1, "outside"), ("predicate", bad_pred, {}, -1, "outside"),
                                      ("negative", neg, {}, -1, "outside"), ("roles", rel, {"roles": roles}, -1, "role"),
                                      ("objects", rel, {"O": 300}, -2, "at most 256 objects")):
        rc, counts, ws = _abi_call(objs, boxes, cen, n, args, vocab, **kw)
        assert rc == code and msg in last_error(), (what, rc, last_error())
        assert (counts == -5).all() and (ws == 7).all(), what      # nothing was enqueued
    with pytest.raises(RuntimeError, match="outside"):
        _run(objs, boxes, cen, n, vocab, triplets=bad_obj)
    too_many = make_vocab("coco", num_preds=300)
    with pytest.raises(RuntimeError, match="at most 256 predicates"):
        _run(objs, boxes, cen, n, too_many, triplets=rel)


def test_packed_vg_trainer_steps():
    """Two trainer steps on synthetic packed_vg batches with --learned_transitivity 1 --learned_converse 1: the annotated
    predicates reach the model as ORIGINAL_EDGE rows, the losses are finite; --include_relationships 0 drops them."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts.train import packed_batch
    from canonicalsg2im_amd.synth import BatchConfig, make_batch
    vocab = make_vocab("vg")
    argv = ["--dataset", "packed_vg", "--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32",
            "--gconv_hidden_dim", "64", "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss",
            "--batch_size", "4", "--gpu_ids", "0", "--learned_transitivity", "1", "--learned_converse", "1"]
    opt = T.make_opt(vocab, argv)
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    tr = T.Trainer(opt, dev)
    cfg = BatchConfig(4, 64, 3, 12, "annotated")
    annotated = [i for nm, i in vocab["pred_name_to_idx"].items() if nm.startswith("rel_")]
    for step in range(2):
        raw = make_batch(vocab, cfg, seed=100 + step)
        batch = packed_batch(opt, tr, raw, dev)
        t, tt = batch[3].cpu().numpy(), batch[5].cpu().numpy()
        for b in range(4):
            rows = raw[3][b].numpy()
            rows = rows[rows[:, 1] != vocab["pred_name_to_idx"]["__padding__"]]
            orig = {tuple(r) for r in t[b][tt[b] == 0].tolist()}
            assert {tuple(r) for r in rows.tolist()} <= orig                  # every annotated row is an original edge
        assert np.isin(t[..., 1][tt == 0], annotated).any()
        G, D = tr.step(batch)
        for k, v in list(G.items()) + list(D.items()):
            if torch.is_tensor(v) and v.numel() == 1:
                assert torch.isfinite(v).all(), k
    opt.include_relationships, opt.learned_converse = False, 0   # packed_vg.py:128-130; no converse edge into them either
    batch = packed_batch(opt, tr, make_batch(vocab, cfg, seed=102), dev)
    t, tt = batch[3].cpu().numpy(), batch[5].cpu().numpy()
    assert (tt == 0).all() or (tt == 1).any()
    assert not np.isin(t[..., 1], annotated).any()
