"""Graph rewriting and layout consistency on a real MI355X (csrc/rewrite.hip, csg_layout_consistency in csrc/metrics.hip)
against their numpy restatements (tests/rewrite_cases.py, held to fixed vectors and the golden scenes by
tests/test_rewrite_cases.py), the graph identities of the robustness walk, and the run end to end on a 64 x 64
random-weight model.  Rows, counts and flags are integers and the fp32 / fp64 values are compared by their bits (a NaN
equals a NaN): no tolerance anywhere."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import agreement_cases as ac
import rewrite_cases as rc
from conftest import load_golden
from test_gpu_split import _checkpoint

pytestmark = pytest.mark.gpu

MODEL = ["--image_size", "64,64", "--ngf", "8", "--ndf", "8", "--no_vgg_loss", "--use_img_disc", "1", "--gconv_hidden_dim", "64",
         "--gconv_dim", "32", "--dataset", "packed_clevr_syn"]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", rc.SELECT_CASES, ids=rc.select_case_id)
def test_select_and_rewrite_equal_the_restatement(cuda, case):
    from canonicalsg2im_amd import _lib, ops
    assert hasattr(_lib.lib, "csg_graph_rows_select") and hasattr(_lib.lib, "csg_graph_rewrite")      # found by their symbols
    triplets, ttype, ids, table, O = rc.make_select_case(case)
    vocab = ac.vocab_of(table)
    want_rows, want_counts = rc.restate_select(triplets, ttype, table, O)
    d_trip, d_type, d_ids = (torch.from_numpy(a).to(cuda) for a in (triplets, ttype, ids))
    rows, counts = ops.select_location_rows(d_trip, d_type, vocab, num_objs=O)
    assert _same_bits(rows, want_rows) and _same_bits(counts, want_counts)
    print("%s: T = %d, counts %s" % (rc.select_case_id(case), triplets.shape[1], want_counts.tolist()))
    assert torch.equal(d_trip.cpu(), torch.from_numpy(triplets))                   # the input is left alone
    for mode, share, direction in rc.REWRITES:
        want = rc.restate_rewrite(want_rows, want_counts, ids, table, mode, share, direction, seed=7)
        got = ops.rewrite_rows(rows, counts, d_ids, vocab, mode, share, direction, seed=7)
        assert _same_bits(got, want), (mode, share, direction)
        if share == 0.0:
            assert _same_bits(got, want_rows)
    assert _same_bits(rows, want_rows)                                             # rewrite_rows writes a second buffer
    # in place is allowed by the entry: out = rows
    mode, share, direction = "one_sided", 0.5, "random"
    inplace = rows.clone()
    P = len(table)
    pred = (_lib.ctypes.c_int32 * 8)(*[table[n] for n in ac.NAMES])
    rcode = _lib.lib.csg_graph_rewrite(_lib.ptr(inplace), _lib.ptr(counts), _lib.ptr(d_ids), rows.shape[0], rows.shape[1], P, pred,
                                      0, 2, share, 7, _lib.ptr(inplace), None)
    torch.cuda.synchronize()
    assert rcode == 0 and _same_bits(inplace, rc.restate_rewrite(want_rows, want_counts, ids, table, mode, share, direction, seed=7))


@pytest.mark.timeout(120)
def test_rewrite_entries_refuse_before_any_launch(cuda):
    from canonicalsg2im_amd import _lib
    lib = _lib.lib
    buf = torch.zeros(4096, dtype=torch.int64, device=cuda)
    a = _lib.ptr(buf)
    ids = (_lib.ctypes.c_int32 * 8)(*range(8))

    def rewrite(B=1, R=4, P=8, ids=ids, mode=0, direction=2, share=0.5, ptrs=(a, a, a, a)):
        return lib.csg_graph_rewrite(ptrs[0], ptrs[1], ptrs[2], B, R, P, ids, mode, direction, share, 3, ptrs[3], None)

    for kw, what in (({"share": 1.0000001}, "outside [0, 1]"), ({"share": -1e-9}, "outside [0, 1]"), ({"share": float("nan")}, "outside [0, 1]"),
                     ({"mode": 2}, "mode 2"), ({"direction": 3}, "direction 3"), ({"direction": -1}, "direction -1"),
                     ({"B": 0}, "bad shape"), ({"R": (1 << 20) + 1}, "bad shape"), ({"P": 7}, "outside [0, P = 7)"),
                     ({"ids": (_lib.ctypes.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 6)}, "must be distinct"),
                     ({"ptrs": (a, None, a, a)}, "null operand"), ({"ptrs": (a, a, None, a)}, "null operand"),
                     ({"ptrs": (a, a, a, None)}, "null operand")):
        assert rewrite(**kw) == -1 and what in _lib.last_error(), (kw, _lib.last_error())

    def select(B=1, T=4, O=4, P=8, ids=ids, ptrs=(a, a, _lib.ctypes.c_void_p(buf.data_ptr() + 2048 * 8), a)):
        return lib.csg_graph_rows_select(ptrs[0], ptrs[1], B, T, O, P, ids, ptrs[2], ptrs[3], None)

    for kw, what in (({"B": 65536}, "bad shape"), ({"T": -1}, "bad shape"), ({"O": 0}, "bad shape"), ({"P": 4097}, "bad shape"),
                     ({"ptrs": (a, a, a, a)}, "rows must not be triplets"), ({"ptrs": (None, a, a, a)}, "null operand"),
                     ({"ptrs": (a, a, a, None)}, "null operand")):
        assert select(**kw) == -1 and what in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0                                       # nothing was launched


@pytest.mark.timeout(120)
def test_rewrite_is_stream_ordered_and_capturable(cuda):
    from canonicalsg2im_amd import ops
    triplets, ttype, ids, table, O = rc.make_select_case((3, 257, 1))
    vocab = ac.vocab_of(table)
    d_trip, d_type, d_ids = (torch.from_numpy(a).to(cuda) for a in (triplets, ttype, ids))
    want_rows, want_counts = rc.restate_select(triplets, ttype, table, O)
    want = rc.restate_rewrite(want_rows, want_counts, ids, table, "noise", 0.5, seed=1)
    ops.select_location_rows(d_trip, d_type, vocab, num_objs=O)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                          # a synchronising call raises (where this torch build checks)
    try:
        rows, counts = ops.select_location_rows(d_trip, d_type, vocab, num_objs=O)
        ops.rewrite_rows(rows, counts, d_ids, vocab, "noise", 0.5, seed=1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows, counts = ops.select_location_rows(d_trip, d_type, vocab, num_objs=O)
        out = ops.rewrite_rows(rows, counts, d_ids, vocab, "noise", 0.5, seed=1)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(rows, want_rows) and _same_bits(counts, want_counts) and _same_bits(out, want)


def _syn_batch(ds, indices, lt, cuda):
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    args = argparse.Namespace(dataset="packed_clevr_syn", vocab=ds.vocab, learned_transitivity=lt, learned_converse=0)
    (batch,) = list(syn.SynClevrBatches(ds, args, None, cuda).batches([indices]))
    return batch


@pytest.mark.timeout(120)
@pytest.mark.parametrize("lt", [0, 1])
@pytest.mark.parametrize("which", ["golden", "two_objects"])
def test_the_graph_of_the_boxes_is_the_graph_of_its_selected_rows(cuda, which, lt):
    """canonical_triplets(boxes) == select -> canonical_triplets(boxes=None, rows): graph A of the robustness walk is the
    graph the dataset builds; and at share 0 graph B is graph A."""
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    from canonicalsg2im_amd.sg2im.data.base_dataset import canonical_triplets
    if which == "golden":
        meta, _ = load_golden("clevr_syn")
        run = [r for r in meta["runs"] if r["min_objects"] == 15][0]          # scenes of 15 to 30 objects
        ds, indices = syn.SynClevrScenes(run["min_objects"], run["max_objects"], run["max_samples"], run["seed"]), [0, 1]
    else:
        ds, indices = syn.SynClevrScenes(2, 2, 1, 3), [0]
    want = _syn_batch(ds, indices, lt, cuda)
    minimal = _syn_batch(ds, indices, 0, cuda)
    objs, ids = minimal[1], minimal[7].to(cuda)
    n_objs = (minimal.objs_host[..., 0] != 0).sum(1) + 1
    rows, counts = ops.select_location_rows(minimal[3], minimal[5], ds.vocab, num_objs=objs.shape[1])
    counts_h = counts.cpu()
    assert int(counts_h.min()) > 0
    again = canonical_triplets(objs, None, None, n_objs, ds.vocab, learned_transitivity=bool(lt), triplets=rows,
                               triplet_counts=counts_h)
    assert torch.equal(again[0], want[3]) and torch.equal(again[2], want[5])
    assert bool((want[5] == 1).any()) == bool(lt and which == "golden")
    # the ORIGINAL rows of the graph with transitive edges are the minimal graph's
    rows_lt, counts_lt = ops.select_location_rows(want[3], want[5], ds.vocab, num_objs=objs.shape[1])
    assert torch.equal(counts_lt, counts) and torch.equal(rows_lt[:, :rows.shape[1]], rows)
    for mode in ("one_sided", "noise"):
        same = ops.rewrite_rows(rows, counts, ids, ds.vocab, mode, 0.0)
        b = canonical_triplets(objs, None, None, n_objs, ds.vocab, learned_transitivity=bool(lt), triplets=same,
                               triplet_counts=counts_h)
        assert torch.equal(b[0], again[0]) and torch.equal(b[2], again[2])
    # an equivalent graph at share 1 states every pair once: half the location rows, the same dummies
    fwd = ops.rewrite_rows(rows, counts, ids, ds.vocab, "one_sided", 1.0, "forward")
    b = canonical_triplets(objs, None, None, n_objs, ds.vocab, learned_transitivity=False, triplets=fwd, triplet_counts=counts_h)
    p2i = ds.vocab["pred_name_to_idx"]
    kept = b[0][..., 1][b[2] == 0]
    assert not bool(torch.isin(kept, torch.tensor([p2i[n] for n in ("__below__", "__right of__", "__surrounding__")], device=cuda)).any())
    location = lambda t: int(torch.isin(t[..., 1], torch.tensor([p2i[n] for n in rc.SLOTS], device=cuda)).sum())
    assert location(b[0]) * 2 == location(minimal[3])
    with pytest.raises(RuntimeError, match="triplet_counts\\[0\\] is negative"):
        canonical_triplets(objs, None, None, n_objs, ds.vocab, triplets=rows, triplet_counts=-1 - counts_h)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", rc.CONSISTENCY_CASES, ids=rc.consistency_case_id)
def test_layout_consistency_equals_the_restatement(cuda, case):
    from canonicalsg2im_amd import _lib, ops
    assert hasattr(_lib.lib, "csg_layout_consistency")
    a, b, counted = rc.make_consistency_case(case)
    tf0, ti0 = np.asarray([0.5, 1.0, 2.0 ** -30, 3.0]), np.arange(20, dtype=np.int64)
    want = rc.restate_consistency(a, b, counted, tf0, ti0)
    twice = rc.restate_consistency(a, b, counted, want[4], want[5])
    da, db, dc = (torch.from_numpy(x).to(cuda) for x in (a, b, counted))
    tf, ti = torch.from_numpy(tf0).to(cuda), torch.from_numpy(ti0).to(cuda)
    first = ops.layout_consistency(da, db, dc, tf, ti)
    once = (tf.clone(), ti.clone())
    second = ops.layout_consistency(da, db, dc, tf, ti)
    torch.cuda.synchronize()
    print("%s: per_sample_f %s pairs %s same %s" % (rc.consistency_case_id(case), want[2].tolist(), want[3][:, 19].tolist(),
                                                    want[3][:, 18].tolist()))
    for k, name in enumerate(("iou_ab", "shift", "per_sample_f", "per_sample_i")):
        assert _same_bits(first[k], want[k]), name
        assert _same_bits(second[k], want[k]), name                      # the same bits on every run
    assert _same_bits(once[0], want[4]) and _same_bits(once[1], want[5])
    assert _same_bits(tf, twice[4]) and _same_bits(ti, twice[5])         # two calls accumulate
    if case[2] == "identical":
        iou, per_i = first[0].cpu().numpy(), first[3].cpu().numpy()
        area = (rc._clamp_box(a)[..., 2] * rc._clamp_box(a)[..., 3]) > 0
        assert (iou[area & (counted == 1)] == 1.0).all() and (per_i[:, 18] == per_i[:, 19]).all()
        assert (per_i[:, 0:18:3] == per_i[:, 2:18:3]).all() and (per_i[:, 1:18:3] == per_i[:, 2:18:3]).all()


@pytest.mark.timeout(120)
def test_layout_consistency_refuses_and_captures(cuda):
    from canonicalsg2im_amd import _lib, ops
    buf = torch.zeros(4096, dtype=torch.float64, device=cuda)
    p = _lib.ptr(buf)
    call = _lib.lib.csg_layout_consistency
    for B, O, what in ((0, 4, "bad shape"), (65536, 4, "bad shape"), (1, 0, "bad shape"), (1, 257, "bad shape")):
        assert call(p, p, p, B, O, p, p, p, p, p, p, None) == -1 and what in _lib.last_error()
    for k in range(9):
        ptrs = [None if i == k else p for i in range(9)]
        assert call(ptrs[0], ptrs[1], ptrs[2], 1, 4, *ptrs[3:], None) == -1 and "null operand" in _lib.last_error()
    odd = _lib.ctypes.c_void_p(buf.data_ptr() + 8)
    assert call(odd, p, p, 1, 4, p, p, p, p, p, p, None) == -1 and "16-byte aligned" in _lib.last_error()
    torch.cuda.synchronize()
    assert float(buf.sum()) == 0.0
    a, b, counted = rc.make_consistency_case((3, 65, "moved"))
    da, db, dc = (torch.from_numpy(x).to(cuda) for x in (a, b, counted))
    tf, ti = torch.zeros(4, dtype=torch.float64, device=cuda), torch.zeros(20, dtype=torch.int64, device=cuda)
    ops.layout_consistency(da, db, dc, tf, ti)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.layout_consistency(da, db, dc, tf, ti)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    tf.zero_(), ti.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops.layout_consistency(da, db, dc, tf, ti)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    once = rc.restate_consistency(a, b, counted, np.zeros(4), np.zeros(20, np.int64))
    twice = rc.restate_consistency(a, b, counted, once[4], once[5])
    assert all(_same_bits(outs[k], once[k]) for k in range(4)) and _same_bits(tf, twice[4]) and _same_bits(ti, twice[5])


@pytest.fixture(scope="module")
def run(cuda, tmp_path_factory):
    """The robustness run once, at share 0: two batches of 3 scenes of 3 to 6 objects through scripts.sample."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.scripts import sample
    from canonicalsg2im_amd.sg2im.data.packed_clevr import clevr_vocab
    root = tmp_path_factory.mktemp("rewrite_run")
    out, scenes, ckpt_path = str(root / "out"), str(root / "scenes.json"), str(root / "itr_3.pt")
    opt = T.make_opt(clevr_vocab(), MODEL + ["--batch_size", "3"])
    _, ckpt = _checkpoint(opt, cuda)
    torch.save(ckpt, ckpt_path)
    argv = MODEL + ["--batch_size", "3", "--min_objects", "3", "--max_objects", "6", "--max_samples", "6", "--seed", "4",
                    "--scenes", scenes, "--checkpoint_name", ckpt_path, "--output_dir", out, "--rewrite", "one_sided",
                    "--rewrite_share", "0", "--rewrite_direction", "forward", "--rewrite_seed", "2"]
    sample.main(argv)
    return {"out": out, "scenes": scenes, "ckpt_path": ckpt_path, "ckpt": ckpt, "opt": opt}


def _walk(run, cuda, lt_at_dataset=0, **kw):
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.scripts.train import folder_builder
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    from canonicalsg2im_amd.sg2im.data.loader import file_order_batches
    from canonicalsg2im_amd.split import generate_split
    ds = syn.SynClevrScenes(scenes_json=run["scenes"])
    torch.manual_seed(0)
    sampler = Sampler(run["opt"], cuda, run["ckpt"])
    args = argparse.Namespace(**dict(vars(run["opt"]), learned_transitivity=lt_at_dataset))
    builder = folder_builder(ds, args, sampler, cuda)
    return generate_split(sampler, builder.batches(file_order_batches(len(ds), 3)), None, deprocess="decode_img", **kw)


@pytest.mark.timeout(300)
def test_the_run_writes_its_files_and_the_report_adds_up(run):
    out = run["out"]
    found = sorted(os.path.relpath(os.path.join(d, n), out).replace(os.sep, "/") for d, _, names in os.walk(out) for n in names)
    sets = ("gt_box_gt_mask", "pred_box_pred_mask", "pred_box_pred_mask_rewritten")
    assert found == sorted(["layouts.json", "generalisation.json", "robustness.json"] +
                           ["generation/%s/%d.png" % (s, i) for s in sets for i in range(6)])
    doc = json.load(open(os.path.join(out, "robustness.json")))
    layouts = json.load(open(os.path.join(out, "layouts.json")))
    general = json.load(open(os.path.join(out, "generalisation.json")))
    assert doc["rewrite"] == {"mode": "one_sided", "share": 0.0, "direction": "forward", "seed": 2}
    assert doc["dataset"] == "packed_clevr_syn" and doc["checkpoint"] == run["ckpt_path"] and doc["images"] == 6
    assert doc["clean"] == general["metrics"] and set(general["metrics"]) == {"avg_iou", "total_iou_05", "total_iou_03", "num_boxes"}
    rows = layouts["images"]
    assert all(set(r["rewritten"]) == {"boxes_pred", "iou", "consistency_iou", "shift", "pair_relations", "relation_agreement"}
               for r in rows)
    # share 0: graph B is graph A, so the two layouts are one
    assert doc["rewritten"] == doc["clean"] and doc["relation_agreement"] == general["relation_agreement"]
    assert doc["consistency"] == {"avg_iou": 1.0, "share_above_05": 1.0, "avg_shift": 0.0}
    pr = doc["pair_relations"]
    assert pr["same_pairs"] == pr["pairs"] == sum(len(r["objects"]) * (len(r["objects"]) - 1) for r in rows) and pr["same_share"] == 1.0
    for r in rows:
        rw = r["rewritten"]
        assert rw["boxes_pred"] == r["predicted_boxes"] and rw["iou"] == r["iou"]
        assert rw["consistency_iou"] == [1.0] * len(r["objects"]) and rw["shift"] == [0.0] * len(r["objects"])
        assert rw["pair_relations"]["same_pairs"] == rw["pair_relations"]["pairs"] == len(r["objects"]) * (len(r["objects"]) - 1)
        assert rw["relation_agreement"] == r["relation_agreement"]
    # the report adds up from the rows
    by = doc["by_num_objects"]
    assert sorted(by, key=int) == [str(n) for n in sorted({len(r["objects"]) for r in rows})]
    assert sum(v["images"] for v in by.values()) == 6
    for name in rc.SLOTS:
        for k in ("in_a", "in_b", "in_both"):
            assert sum(v["pair_relations"][name][k] for v in by.values()) == pr[name][k] == sum(
                r["rewritten"]["pair_relations"][name][k] for r in rows)
        assert pr[name]["in_a"] == pr[name]["in_b"] == pr[name]["in_both"] and pr[name]["kept"] in (1.0, None)
    assert sum(pr[name]["in_a"] for name in rc.SLOTS) >= pr["pairs"]             # every pair has a verdict on one axis at least
    assert sum(v["pair_relations"]["pairs"] for v in by.values()) == pr["pairs"]
    assert sum(v["rewritten"]["num_boxes"] for v in by.values()) == doc["rewritten"]["num_boxes"] == sum(len(r["objects"]) for r in rows)
    assert sum(v["relation_agreement"]["tested"] for v in by.values()) == doc["relation_agreement"]["tested"]
    assert sum(v["relation_agreement"]["agreeing"] for v in by.values()) == doc["relation_agreement"]["agreeing"]
    assert layouts["metrics"]["rewritten"]["consistency"] == doc["consistency"]


@pytest.mark.timeout(300)
def test_a_rewritten_graph_moves_the_layout_and_the_walk_is_opt_in(run, cuda):
    from canonicalsg2im_amd.split import Rewrite
    m0, r0 = _walk(run, cuda)
    assert set(m0) == {"avg_iou", "total_iou_05", "total_iou_03", "num_boxes"}             # without `rewrite`: key for key as before
    assert all(set(r) == {"image_id", "objects", "gt_boxes", "predicted_boxes", "iou"} for r in r0)
    m1, r1 = _walk(run, cuda, rewrite=None)
    assert (m1, r1) == (m0, r0)
    layouts = json.load(open(os.path.join(run["out"], "layouts.json")))
    assert [{k: r[k] for k in r0[0]} for r in layouts["images"]] == r0 and {k: layouts["metrics"][k] for k in m0} == m0
    m2, r2 = _walk(run, cuda, rewrite=Rewrite("noise", 1.0, seed=2))
    assert set(m2) == set(m0) | {"rewritten"} and {k: m2[k] for k in m0} == m0
    assert [{k: v for k, v in r.items() if k != "rewritten"} for r in r2] == r0
    rw = m2["rewritten"]
    assert rw["consistency"]["avg_iou"] < 1.0 and rw["consistency"]["avg_shift"] > 0.0
    assert rw["pair_relations"]["same_pairs"] < rw["pair_relations"]["pairs"]
    assert rw["relation_agreement"]["tested"] > 0
    with pytest.raises(ValueError, match="rows that are not ORIGINAL"):
        _walk(run, cuda, lt_at_dataset=1, rewrite=Rewrite("noise", 1.0))
