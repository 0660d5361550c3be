"""The numpy restatement of the packed Visual Genome canonical graphs (tests/canon_annotated.py) against the outputs of
the reference's own BaseDataset functions and vg_collate_fn (tests/golden/canon_annotated.npz).  Bit-exact."""
import numpy as np

import canon_annotated as ca
from conftest import load_golden


def test_annotated_graphs_match_reference():
    meta, a = load_golden("canon_annotated")
    assert len(meta["cases"]) >= 6
    for ci in range(len(meta["cases"])):
        case, g, vocab = ca.fixture_case(meta, a, ci)
        u = None
        if case["learned_converse"]:
            np.random.seed(case["seed"])
            u = np.random.random_sample(case["draws"])
        trip, tt, counts, conv = ca.canonical_batch(g["objs"], g["boxes"], g["centers"], g["n"], g["rel"], vocab,
                                                    learned_transitivity=bool(case["learned_transitivity"]),
                                                    learned_converse=bool(case["learned_converse"]),
                                                    converse_weights=g.get("weights"), uniforms=u)
        assert np.array_equal(counts, g["counts"]), (ci, counts, g["counts"])
        assert np.array_equal(trip, g["triplets"]), ci
        assert np.array_equal(tt, g["tt"]), ci
        if case["learned_converse"]:
            assert np.array_equal(conv.astype(np.float32), g["conv"]), ci
            assert conv.sum() == case["draws"] and conv[:, :, :-1].sum() > 0


def test_fixture_covers_the_issue_cases():
    """Annotated predicates beyond the location ones, location-predicate rows, self-relations, a sample without
    relationships, transitive self-loops from cycles, both converse / transitivity settings and permuted ids."""
    meta, a = load_golden("canon_annotated")
    flags = {(c["learned_transitivity"], c["learned_converse"]) for c in meta["cases"]}
    assert flags == {(0, 0), (0, 1), (1, 0), (1, 1)}
    permuted = [c for c in meta["cases"] if c["pred_idx_to_name"][:2] != ["__padding__", "__in_image__"]]
    assert permuted and any(c["learned_transitivity"] for c in permuted)
    sizes = [n for c in meta["cases"] for n in c["sizes"]]
    assert min(sizes) == 2 and 100 in sizes and max(sizes) >= 240
    loops = selfrel = locrows = 0
    for ci in range(len(meta["cases"])):
        case, g, vocab = ca.fixture_case(meta, a, ci)
        p2i = vocab["pred_name_to_idx"]
        rel = g["rel"]
        if len(case["sizes"]) > 1:
            assert (rel[1, :, 1] == p2i["__padding__"]).all()                 # no relationships in sample 1
        real = rel[rel[:, :, 1] != p2i["__padding__"]]
        selfrel += int((real[:, 0] == real[:, 2]).sum())
        locrows += int(np.isin(real[:, 1], [p2i[n] for n in ca.AUGMENTED]).sum())
        t, tt = g["triplets"], g["tt"]
        loops += int(((tt == 1) & (t[..., 0] == t[..., 2])).sum())
    assert selfrel > 0 and locrows > 0 and loops > 0
