"""The canonical-graph matrix on the CPU (tests/canon_cases.py): the numpy restatements reproduce what the reference made of
the structured families (tests/golden/canon_structured.npz) bit for bit, every family does what its name says — asserted
from the oracle's adjacency, so that no row of the table pretends — and the table is complete.  No GPU.

The whole file takes 2 to 3 s on one CPU core (48 tests; the largest pieces are the oracle on the 255-object chains and
nests, about 0.1 s each)."""
import itertools

import numpy as np
import pytest

import canon_cases as cc
from canonicalsg2im_amd.synth import make_vocab
from conftest import load_golden
from oracle import canon

ORDER = ("__below__", "__above__", "__left of__", "__right of__")


def _counts(trip, tt, vocab):
    """{predicate name: (original rows, transitive rows)} of one sample's graph."""
    i2n = vocab["pred_idx_to_name"]
    out = {nm: (0, 0) for nm in i2n}
    for p in np.unique(trip[:, 1]) if len(trip) else []:
        rows = trip[:, 1] == p
        out[i2n[p]] = (int((rows & (tt == 0)).sum()), int((rows & (tt == 1)).sum()))
    return out


def _graph(family, rows, seed=0, image="last", **kw):
    vocab = make_vocab("coco")
    objs, boxes, cen = cc.sample(family, rows, seed, image, **kw)
    trip, tt = canon.canonical_graph(objs, boxes, cen, vocab, learned_transitivity=True, include_dummies=(image == "last"))
    return _counts(trip, tt, vocab), (objs, boxes, cen)


# ------------------------------------------------------------------------------------------ 1. the reference's own output
def _golden_cases():
    meta, _ = load_golden("canon_structured")
    return list(range(len(meta["cases"])))


@pytest.mark.parametrize("ci", _golden_cases())
def test_the_restatement_reproduces_the_reference_on_the_structured_families(ci):
    meta, g = load_golden("canon_structured")
    case = meta["cases"][ci]
    vocab = make_vocab(meta["vocab"])
    objs, boxes, cen = cc.sample(case["family"], case["rows"], case["seed"], case["image"], **case["kw"])
    packed = g["c%d_in" % ci].numpy()
    assert np.array_equal(packed[:, 0], objs) and packed[:, 1:5].tobytes() == boxes.tobytes()      # the family is what the
    assert packed[:, 5:].tobytes() == cen.tobytes()                                                # reference was given
    at, conv_at = 0, 0
    for run in case["runs"]:
        if run["refused"]:                   # the reference cannot build it: nothing to compare (the metadata says why)
            assert run["refused"] in ("IndexError", "ValueError")
            continue
        want = g["c%d_rows" % ci].numpy()[at:at + run["count"]].astype(np.int64)
        at += run["count"]
        kw = {}
        if run["learned_converse"]:
            state = np.random.get_state()
            np.random.seed(run["seed"])
            kw = dict(learned_converse=True, converse_weights=g["weights"].numpy(), uniforms=iter(np.random.random_sample(run["draws"])))
            np.random.set_state(state)
        out = canon.canonical_graph(objs, boxes, cen, vocab, bool(run["learned_transitivity"]), bool(case["include_dummies"]), **kw)
        assert np.array_equal(out[0], want[:, :3]) and np.array_equal(out[1], want[:, 3]), (case, run)
        if run["learned_converse"]:
            assert np.array_equal(out[2], g["c%d_conv" % ci].numpy()[conv_at].astype(np.float64))
            assert next(kw["uniforms"], None) is None                        # every recorded draw was consumed
            conv_at += 1


def test_the_golden_file_covers_every_family_and_records_what_the_reference_cannot_build():
    meta, _ = load_golden("canon_structured")
    cases = meta["cases"]
    assert {c["family"] for c in cases} == set(cc.FAMILIES) and {c["image"] for c in cases} == set(cc.IMAGE_POSITIONS)
    assert all(c["rows"] <= 12 and len(c["runs"]) == 4 for c in cases)
    refused = {(c["family"], c["image"], c["include_dummies"]) for c in cases if any(r["refused"] for r in c["runs"])}
    # no location triplet at all, or not exactly one __image__ row under include_dummies: the restatement and the kernels
    # define these (no relation rows; no dummies; the first __image__ row), the older device tests pin sizes 1 and 2
    assert refused == {("identical", "last", 1), ("single", "last", 1), ("only_image", "last", 1), ("random", "absent", 1),
                       ("random", "twice", 1)}


# ------------------------------------------------------------------------------------------ 2. the families
@pytest.mark.parametrize("family", ["chain", "reverse_chain", "shuffled_chain"])
@pytest.mark.parametrize("rows", [65, 256])
def test_a_chain_is_one_total_order_on_both_axes(family, rows):
    n = rows - 1
    counts, _ = _graph(family, rows, seed=3)
    for name in ORDER:                       # two axes, each ordered both ways
        assert counts[name] == (n - 1, (n - 1) * (n - 2) // 2), (name, counts[name])
    assert counts["__inside__"] == counts["__surrounding__"] == (0, 0) and counts["__in_image__"] == (n, 0)
    if rows == 256:                          # the figures of the 255-object chain
        assert sum(c[1] for c in counts.values()) == 128524 and sum(c[0] for c in counts.values()) == 1271


@pytest.mark.parametrize("seed", [2, 5])
@pytest.mark.parametrize("rows", [65, 256])
def test_nested_is_one_total_order_of_inside_and_surrounding(rows, seed):
    n = rows - 1
    counts, _ = _graph("nested", rows, seed=seed)
    assert counts["__inside__"] == counts["__surrounding__"] == (n - 1, (n - 1) * (n - 2) // 2)
    assert all(counts[name] == (0, 0) for name in ORDER)


def test_identical_has_no_location_row_and_single_and_only_image_have_none_either():
    for family, rows in (("identical", 65), ("identical", 256), ("single", 2), ("only_image", 1)):
        counts, _ = _graph(family, rows)
        assert all(counts[name] == (0, 0) for name in canon.AUGMENTED) and counts["__in_image__"] == (rows - 1, 0)


@pytest.mark.parametrize("rows", [65, 129, 256])
def test_grid_has_the_layered_counts(rows):
    n = rows - 1
    k = cc.grid_side(n)
    counts, _ = _graph("grid", rows)
    for names, layer in ((("__left of__", "__right of__"), np.arange(n) % k), (("__above__", "__below__"), np.arange(n) // k)):
        size = np.bincount(layer)
        assert len(size) > 2 and size.max() > 1                                   # k-way ties: layers, not a total order
        neighbours = int((size[:-1] * size[1:]).sum())                            # the minimal graph: adjacent layers, all pairs
        ordered = int((size.sum() ** 2 - (size ** 2).sum()) // 2)                 # the closure: every pair of different layers
        for name in names:
            assert counts[name] == (neighbours, ordered - neighbours), (name, counts[name])


@pytest.mark.parametrize("rows", [129, 256])
def test_two_clusters_have_no_ordered_pair_across_the_word_boundary_until_the_bridge(rows):
    n = rows - 1
    for bridge in (False, True):
        objs, boxes, cen = cc.sample("two_clusters", rows, 0, bridge=bridge)
        adj = canon.location_relations(boxes, cen, objs != 0)
        closure = np.stack([canon.path(a) for a in adj])
        across = closure[:, :64, 64:n].sum(axis=(1, 2)) + closure[:, 64:n, :64].sum(axis=(1, 2))
        inside = closure[:, :64, :64].sum(axis=(1, 2))
        assert list(inside[:4]) == [64 * 63 // 2] * 4                             # a chain inside the first word
        if not bridge:
            assert list(across[:4]) == [0, 0, 0, 0]
            assert across[4] == across[5] == 64 * (n - 64)                        # every pair across: surrounding / inside
        else:
            assert [int(adj[r, :64, 64:n].sum() + adj[r, 64:n, :64].sum()) for r in range(4)] == [1, 1, 1, 1]   # one ordered pair
            assert list(across[:4]) == [64 * (n - 64)] * 4                        # ... whose closure joins the clusters
            assert across[4] == across[5] == 64 * (n - 64) - 1


def test_pivot_last_puts_the_bridge_on_warshalls_last_pivot():
    """With no __image__ row behind it, the object every path across the clusters runs through is row n - 1: a closure that
    stops one pivot early has no ordered pair across, and the graph is that of the plain bridge with two rows renamed."""
    objs, boxes, cen = cc.sample("two_clusters", 129, 0, "absent", bridge=True, pivot_last=True)
    adj = canon.location_relations(boxes, cen, objs != 0)[2]                  # __left of__
    early = np.array(adj)
    for i in range(128):                                                          # path() without its last pivot
        rows = early[:, i].copy()
        rows[i] = False
        early[rows] |= early[i]
    full = canon.path(adj)
    assert full.sum() - early.sum() >= 63 * 64 and not early[:63, 64:128].any() and full[:63, 64:128].all()
    plain = canon.path(canon.location_relations(*cc.sample("two_clusters", 129, 0, "absent", bridge=True)[1:], objs != 0)[2])
    swap = np.arange(129)
    swap[[63, 128]] = 128, 63
    assert np.array_equal(full, plain[np.ix_(swap, swap)])


def test_the_poisoned_padding_rows_would_change_the_result_if_read():
    vocab = make_vocab("coco")
    for row in cc.TABLE:
        if "lds" not in row["paths"] or row["refused"] or len(set(row["sizes"])) == 1 or max(row["sizes"]) > 200:
            continue
        a = cc.inputs(row)
        b = int(np.argmin(row["sizes"]))
        n = int(a["n"][b])
        here = canon.canonical_graph(a["objs"][b, :n], a["boxes"][b, :n], a["centers"][b, :n], vocab, False, False)
        more = canon.canonical_graph(a["objs"][b, :n + 1], a["boxes"][b, :n + 1], a["centers"][b, :n + 1], vocab, False, False)
        if n >= 2 and row["family"] not in ("single", "only_image"):
            assert len(more[0]) > len(here[0]), row["id"]
        assert a["objs"][b, n] != 0                                               # ... and its id is not __image__'s


# ------------------------------------------------------------------------------------------ 3. the table
def _ok(path):
    return [r for r in cc.TABLE if path in r["paths"] and not r["refused"]]


def test_every_path_appears_at_every_size_it_supports():
    for path, limit in cc.LIMIT.items():
        seen = set(itertools.chain.from_iterable(r["sizes"] for r in _ok(path)))
        need = {s for s in cc.SIZES if s <= limit}
        if path == "clevr":
            need = {s for s in (1, 2, 3, 63, 64)}                                 # 63 objects: 64 rows with the __image__ row
        assert need <= seen, (path, sorted(need - seen))
        assert limit in seen and max(seen) == limit


def test_every_refusal_is_one_above_a_passing_row():
    for path, limit in cc.LIMIT.items():
        refused = [r for r in cc.TABLE if path in r["paths"] and r["refused"] == cc.REFUSAL[path]]
        assert refused and all(max(r["sizes"]) == limit + 1 for r in refused), path
        assert any(max(r["sizes"]) == limit for r in _ok(path)), path


def test_every_family_appears_on_every_path_that_takes_boxes():
    for path in cc.BOX_PATHS:
        assert {r["family"] for r in _ok(path)} == set(cc.FAMILIES), path
    for family in ("chain", "reverse_chain", "shuffled_chain", "nested"):
        sizes = set(itertools.chain.from_iterable(r["sizes"] for r in _ok("lds") if r["family"] == family and r["image"] == "last"))
        assert set(cc.CHAIN_SIZES) <= sizes, family


def test_every_flag_combination_and_every_image_position_appears():
    flags = {(r["trans"], r["dummies"], r["conv"], r["permuted"]) for r in _ok("lds")}
    assert flags == set(itertools.product((0, 1), repeat=4))
    assert {r["image"] for r in _ok("lds")} == set(cc.IMAGE_POSITIONS)
    assert {(r["pairs"], r["use_converse"]) for r in _ok("pairs") if 256 in r["sizes"] and 255 in r["sizes"]} >= {
        ("matching", 1), ("star", 0), ("cycle", 0), ("cycle", 1)}
    mixed, back = cc.ROWS["mixed"], cc.ROWS["mixed_reversed"]
    assert mixed["sizes"] == back["sizes"][::-1] and {1, 2, 3, 64, 193, 256} <= set(mixed["sizes"])
    over = cc.ROWS["lds_n_over"]
    assert over["conv"] and over["n_over"][1] == max(over["sizes"]) + 1 and over["n_over"][0] < len(over["sizes"]) - 1


def test_the_annotated_rows_hold_what_the_table_promises():
    row = cc.ROWS["general_vg_all"]
    a = cc.inputs(row)
    p2i = a["vocab"]["pred_name_to_idx"]
    plain = sorted(set(p2i.values()) - {p2i["__padding__"], p2i["__in_image__"]})
    by_size = dict(zip(row["sizes"], a["rel"]))
    chain = by_size[256][by_size[256][:, 1] != p2i["__padding__"]]
    p0 = chain[0, 1]
    links = chain[chain[:, 1] == p0]
    assert {(63, 64), (127, 128), (191, 192), (253, 254)} <= {(s, o) for s, _, o in links.tolist()}    # across every word boundary
    assert len(links) == 255 and len(np.unique(links, axis=0)) == 254                                  # one row given twice
    other = chain[chain[:, 1] != p0]
    assert other[:, [0, 2]].tolist() == [[0, 1], [1, 0]]                                               # a two-cycle
    assert len(set(chain[:, 1].tolist())) == 2 < len(plain)                                            # predicates with no row
    every = by_size[191][by_size[191][:, 1] != p2i["__padding__"]]
    assert sorted(every[:, 1].tolist()) == plain                                                       # every predicate once


def test_the_reversed_batch_is_the_reversed_result():
    """What the device test then holds the kernels to: the restatement has no state to leak, the samples' graphs do not
    depend on their place in the batch."""
    a, b = cc.expected(cc.ROWS["mixed"]), cc.expected(cc.ROWS["mixed_reversed"])
    assert np.array_equal(a["counts"], b["counts"][::-1])
    T = min(a["triplets"].shape[1], b["triplets"].shape[1])
    assert T >= a["counts"].max() and np.array_equal(a["triplets"][:, :T], b["triplets"][::-1, :T])
