"""Authored scene graphs on the host (canonicalsg2im_amd/authored.py) against tests/golden/authored_graphs.npz: the
reference's own extract_objs / extract_triplets outputs for the twelve graphs of its scripts/run_model.py
(tests/golden/make_golden_authored.py).  No GPU."""
import copy
import json

import numpy as np
import pytest
import torch

from conftest import load_golden


def fixture_vocab(meta):
    """The fixture's CLEVR vocabulary in the form the package's vocabularies have (synth.make_vocab)."""
    attrs = {a: dict(d) for a, d in meta["attributes"].items()}
    objects = attrs[list(attrs)[0]]
    names = list(meta["pred_idx_to_name"])
    idx_to_name = [None] * (max(objects.values()) + 1)
    for k, v in objects.items():
        idx_to_name[v] = k
    return {"attributes": attrs, "object_name_to_idx": objects, "object_idx_to_name": idx_to_name,
            "pred_idx_to_name": names, "pred_name_to_idx": {n: i for i, n in enumerate(names)}}


@pytest.fixture(scope="module")
def fx():
    meta, arrays = load_golden("authored_graphs")
    return meta, arrays, fixture_vocab(meta)


def test_the_fixture_is_what_the_issue_says(fx):
    meta, arrays, vocab = fx
    assert meta["sizes"] == [3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6, 6] and len(meta["graphs"]) == 12
    assert list(vocab["attributes"]) == ["shape", "color", "material", "size"]
    assert vocab["pred_idx_to_name"][:6] == ["__in_image__", "right", "behind", "front", "left", "__padding__"]
    assert len(vocab["pred_idx_to_name"]) == 12
    # the reference reduced something: the dense 4-object graph authors 6 'front' triplets and keeps 3
    dense4 = arrays["g4_triplets"].numpy()
    assert sum(len(s) for s in meta["graphs"][4]["relationships"]["front"]) == 6
    assert int((dense4[:, 1] == vocab["pred_name_to_idx"]["front"]).sum()) == 3


def test_encode_graphs_equals_the_reference_for_all_twelve_graphs_batched_and_singly(fx):
    from canonicalsg2im_amd.authored import encode_graphs, load_graphs
    meta, arrays, vocab = fx
    graphs = load_graphs(meta["graphs"], vocab)
    pad = vocab["pred_name_to_idx"]["__padding__"]
    objs, trip, counts = encode_graphs(graphs, vocab)
    assert objs.dtype == trip.dtype == counts.dtype == torch.int64
    O = max(meta["sizes"]) + 1
    T = max(arrays["g%d_triplets" % g].shape[0] for g in range(12))
    assert tuple(objs.shape) == (12, O, 4) and tuple(trip.shape) == (12, T, 3) and tuple(counts.shape) == (12,)
    for g in range(12):
        want_o, want_t = arrays["g%d_objs" % g], arrays["g%d_triplets" % g]
        n, t = want_o.shape[0], want_t.shape[0]
        assert int(counts[g]) == n == meta["sizes"][g] + 1
        assert torch.equal(objs[g, :n], want_o), g
        assert torch.equal(objs[g, n - 1], torch.zeros(4, dtype=torch.int64))            # __image__ last of the real rows
        assert int(objs[g, n:].abs().sum()) == 0
        assert torch.equal(trip[g, :t], want_t), (g, trip[g, :t].tolist(), want_t.tolist())
        assert torch.equal(trip[g, t:], torch.tensor([0, pad, 0]).expand(T - t, 3))
        o1, t1, c1 = encode_graphs([graphs[g]], vocab)                                     # singly: no padding at all
        assert torch.equal(o1[0], want_o) and torch.equal(t1[0], want_t) and c1.tolist() == [n]


def test_load_graphs_reads_a_json_file_and_a_single_graph(fx, tmp_path):
    from canonicalsg2im_amd.authored import encode_graphs, load_graphs
    meta, _, vocab = fx
    path = tmp_path / "graphs.json"
    path.write_text(json.dumps(meta["graphs"]))
    a = encode_graphs(load_graphs(str(path), vocab), vocab)
    b = encode_graphs(meta["graphs"], vocab)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert load_graphs(meta["graphs"][0], vocab) == [meta["graphs"][0]]


def test_the_flat_form_round_trips():
    from canonicalsg2im_amd.authored import encode_graphs, load_graphs, triplet_names
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("vg")
    rel = vocab["pred_idx_to_name"][10]
    graphs = [{"objects": ["obj_5", "obj_7", "obj_5"], "relationships": [[0, "__left of__", 1], [2, rel, 0], [1, rel, 2]]},
              {"objects": ["obj_1"], "relationships": []}]
    objs, trip, counts = encode_graphs(load_graphs(graphs, vocab), vocab)
    assert tuple(objs.shape) == (2, 4, 1) and objs[:, :, 0].tolist() == [[5, 7, 5, 0], [1, 0, 0, 0]]
    assert counts.tolist() == [4, 2]
    names = triplet_names(trip, vocab)
    for g, graph in enumerate(graphs):
        n = len(graph["objects"])
        assert names[g] == [list(t) for t in graph["relationships"]] + [[i, "__in_image__", n] for i in range(n)]
        back = [vocab["object_idx_to_name"][int(i)] for i in objs[g, :n, 0]]
        assert back == graph["objects"]
    assert trip[1, 1:].tolist() == [[0, vocab["pred_name_to_idx"]["__padding__"], 0]] * 5


def _ref_graph(fx):
    return copy.deepcopy(fx[0]["graphs"][1])


@pytest.mark.parametrize("name,token", [
    ("unknown attribute value", "pink"), ("missing attribute", "material"), ("unknown predicate", "beside"),
    ("padding predicate", "__padding__"), ("index too large", "3"), ("negative index", "-1"), ("empty objects", "empty"),
    ("wrong list length", "front"), ("flat name in a CLEVR vocabulary", "cube"), ("not a graph", "objects"),
])
def test_malformed_reference_form_raises_with_the_graph_index_and_the_token(fx, name, token):
    from canonicalsg2im_amd.authored import encode_graphs, load_graphs
    _, _, vocab = fx
    good, bad = _ref_graph(fx), _ref_graph(fx)
    if name == "unknown attribute value":
        bad["objects"][1]["color"] = "pink"
    elif name == "missing attribute":
        del bad["objects"][2]["material"]
    elif name == "unknown predicate":
        bad["relationships"]["beside"] = [[], [], []]
    elif name == "padding predicate":
        bad["relationships"]["__padding__"] = [[], [], []]
    elif name == "index too large":
        bad["relationships"]["left"][0] = [3]
    elif name == "negative index":
        bad["relationships"]["left"][0] = [-1]
    elif name == "empty objects":
        bad = {"objects": [], "relationships": {}}
    elif name == "wrong list length":
        bad["relationships"]["front"] = [[], []]
    elif name == "flat name in a CLEVR vocabulary":
        bad["objects"][0] = "cube"
    else:
        bad = ["objects"]
    for fn in (lambda gs: load_graphs(gs, vocab), lambda gs: encode_graphs(gs, vocab)):
        with pytest.raises(ValueError) as e:
            fn([good, good, bad])
        assert "scene graph 2" in str(e.value) and token in str(e.value), str(e.value)


@pytest.mark.parametrize("rels,token", [([[0, "rel_99", 1]], "rel_99"), ([[0, "__left of__", 2]], "2"),
                                        ([[0, "__left of__"]], "__left of__"), ([[True, "__left of__", 1]], "True")])
def test_malformed_flat_form_raises_with_the_graph_index_and_the_token(rels, token):
    from canonicalsg2im_amd.authored import encode_graphs
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("coco")
    with pytest.raises(ValueError) as e:
        encode_graphs([{"objects": ["obj_1", "obj_2"], "relationships": []}, {"objects": ["obj_1", "obj_2"], "relationships": rels}],
                      vocab)
    assert "scene graph 1" in str(e.value) and token in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="scene graph 0.*'zebra'"):
        encode_graphs([{"objects": ["zebra"], "relationships": []}], vocab)


def test_reduction_replays_the_reference_on_a_cycle_and_keeps_short_lists_as_written(fx):
    """The hyper graphs author self-relations ('behind' and 'left' of every object hold the object itself): the reference's
    scalar loops clear a row while reading it, and the fixture pins that.  A list of fewer than three triplets is not
    reduced and keeps the authored order (object-major), which is not (subject, object) order."""
    from canonicalsg2im_amd.authored import encode_graphs
    meta, arrays, vocab = fx
    hyper = meta["graphs"][2]
    assert all(i in hyper["relationships"]["behind"][i] for i in range(3))
    _, trip, _ = encode_graphs([hyper], vocab)
    assert torch.equal(trip[0], arrays["g2_triplets"])
    g = {"objects": hyper["objects"], "relationships": {"left": [[2], [], []], "right": [[], [], [1, 0]]}}
    _, trip, _ = encode_graphs([g], vocab)
    p = vocab["pred_name_to_idx"]
    assert trip[0, :3].tolist() == [[2, p["left"], 0], [1, p["right"], 2], [0, p["right"], 2]]
