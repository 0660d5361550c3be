"""Scene graphs written by a person -> the padded tensors the model takes (host only; no device is touched here).

Two input forms, told apart by the type of "relationships":

  * the reference's form (scripts/run_model.py:19-41), for vocabularies with several attributes (CLEVR):
        {"objects": [{"shape": "cube", "color": "red", "material": "metal", "size": "large"}, ...],
         "relationships": {"right": [[], [0], [1]], "front": [[], [], []]}}
    relationships[pred][o1] lists the SUBJECTS o2 of object o1: every entry is the triplet [o2, pred, o1].  Encoded exactly
    as the reference's extract_objs / extract_triplets do (sg2im/data/clevr_dialog.py:227-233, 289-307): per predicate, in
    the dictionary's order, a list of three or more triplets is replaced by its transitive reduction
    (scripts/graphs_utils.py:74-82 with p_keep = 0: the minimal graph of the closure, rows by (subject, object)); a
    shorter list is kept as written.

  * a flat form for vocabularies with one attribute (COCO, Visual Genome):
        {"objects": ["person", "grass"], "relationships": [[0, "left of", 1]]}
    Every row is the triplet [subject, pred, object], kept as written and in the order written.

In both forms the `__image__` object is appended after the authored objects and one [i, __in_image__, n] triplet per
object follows the authored ones.  A batch is padded as the packed collates pad: object rows of 0, triplet rows of
[0, __padding__, 0].

Everything a graph names is checked here, before any launch: an unknown name, an index out of range or an empty object
list raises ValueError naming the graph's index and the offending token.
"""
import json

import torch

# twelve fixed RGB triples for the box outlines (row o takes DEFAULT_PALETTE[o % 12]); no shuffle, no random stream
DEFAULT_PALETTE = (
    (230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
    (70, 240, 240), (240, 50, 230), (210, 245, 60), (250, 190, 190), (0, 128, 128), (170, 110, 40),
)


def _bad(g, what):
    return ValueError("scene graph %d: %s" % (g, what))


def _index(g, v, n, where):
    if isinstance(v, bool) or not isinstance(v, int) or v < 0 or v >= n:
        raise _bad(g, "%s: object index %r outside [0, %d)" % (where, v, n))
    return v


def _pred_id(g, name, vocab):
    p2i = vocab["pred_name_to_idx"]
    if not isinstance(name, str) or name not in p2i or name == "__padding__":
        raise _bad(g, "unknown predicate %r" % (name,))
    return p2i[name]


def _closure(m):
    """Path matrix (scripts/graphs_utils.py:15-27): row j absorbs row i when m[j][i], for i ascending."""
    p = [list(r) for r in m]
    n = len(p)
    for i in range(n):
        for j in range(n):
            if j != i and p[j][i]:
                p[j] = [a or b for a, b in zip(p[j], p[i])]
    return p


def _minimal(p):
    """The reduction of a closed graph in place (scripts/graphs_utils.py:30-38), in its scalar order: a self-relation
    (an authored cycle) clears its own row while that row is being read, as there."""
    n = len(p)
    for j in range(n):
        for i in range(n):
            if p[i][j]:
                for k in range(n):
                    if p[j][k]:
                        p[i][k] = 0
    return p


def _reduced(rows, pid):
    """reduce_transitive_edges(rows, p_keep=0) (scripts/graphs_utils.py:74-82).  With p_keep = 0 its random matrix decides
    nothing (prob * x > 1 never holds), so none is drawn here."""
    if len(rows) < 3:
        return rows
    n = max(max(s, o) for s, _, o in rows) + 1
    m = [[0] * n for _ in range(n)]
    for s, _, o in rows:
        m[s][o] = 1
    m = _minimal(_closure(m))
    return [[s, pid, o] for s in range(n) for o in range(n) if m[s][o]]


def object_ids(objects, vocab, bad):
    """Authored objects — names (vocabularies with one attribute) or {attribute: name} dictionaries — -> their id rows
    [n][A], in the vocabulary's attribute order and without an `__image__` row.  `bad(what)` makes the exception of an
    unknown or missing name: the caller says which graph or row it was."""
    attrs = vocab["attributes"]
    names = list(attrs.keys())
    rows = []
    for i, obj in enumerate(objects):
        if isinstance(obj, str):
            if len(names) != 1:
                raise bad("object %d is the name %r, but the vocabulary has the attributes %s" % (i, obj, names))
            obj = {names[0]: obj}
        if not isinstance(obj, dict):
            raise bad("object %d: %r is neither a name nor a dictionary of attributes" % (i, obj))
        row = []
        for a in names:
            if a not in obj:
                raise bad("object %d lacks the attribute %r" % (i, a))
            v = obj[a]
            if not isinstance(v, str) or v not in attrs[a] or v == "__image__":
                raise bad("object %d: unknown %s %r" % (i, a, v))
            row.append(attrs[a][v])
        rows.append(row)
    return rows


def object_names(rows, vocab):
    """The other direction of `object_ids`: id rows [n][A] -> the objects as a person writes them, a list of names for a
    vocabulary with one attribute and a list of {attribute: name} otherwise.  An id no name maps to raises ValueError; of
    several names with one id the first in the table's order is taken."""
    attrs = vocab["attributes"]
    names = list(attrs.keys())
    back = {}
    for a in names:
        back[a] = {}
        for name, idx in attrs[a].items():
            back[a].setdefault(int(idx), name)
    out = []
    for i, row in enumerate(rows):
        if len(row) != len(names):
            raise ValueError("object %d has %d ids, the vocabulary has the attributes %s" % (i, len(row), names))
        for a, idx in zip(names, row):
            if int(idx) not in back[a]:
                raise ValueError("object %d: no %s has the id %d" % (i, a, int(idx)))
        named = {a: back[a][int(idx)] for a, idx in zip(names, row)}
        out.append(named[names[0]] if len(names) == 1 else named)
    return out


def object_labels(graphs):
    """Authored graphs -> the labels of their layout pictures, B lists of O `str` or None in the rows of `encode_graphs`: an
    object of the reference's form is named ', '.join(obj.values()), as scripts/run_model.py hands it to
    draw_reversed_item; one of the flat form by its name.  None for the appended `__image__` row and for padding rows."""
    O = max(len(graph["objects"]) for graph in graphs) + 1
    out = []
    for graph in graphs:
        names = [obj if isinstance(obj, str) else ", ".join(obj.values()) for obj in graph["objects"]]
        out.append(names + [None] * (O - len(names)))
    return out


def labels_from_objs(objs_host, vocab):
    """A dataset batch's object ids (B,O,A) on the host -> B lists of O `str` or None: object_idx_to_name[id] for a
    vocabulary with one attribute, otherwise the attributes' names in the vocabulary's attribute order joined by ', '
    (CLEVR: "cube, red, metal, large").  None for rows of id 0 (padding) and for `__image__`."""
    attrs = vocab["attributes"]
    back = []
    for a in attrs:
        names = {}
        for name, idx in attrs[a].items():
            names.setdefault(int(idx), name)
        back.append(names)
    image = int(vocab["object_name_to_idx"]["__image__"])
    single = len(back) == 1
    out = []
    for sample in (objs_host.tolist() if hasattr(objs_host, "tolist") else objs_host):
        row = []
        for ids in sample:
            if ids[0] == 0 or ids[0] == image:
                row.append(None)
            elif single:
                row.append(vocab["object_idx_to_name"][ids[0]])
            else:
                if len(ids) != len(back) or any(i not in names for i, names in zip(ids, back)):
                    raise ValueError("object ids %r name no object of the attributes %s" % (ids, list(attrs)))
                row.append(", ".join(names[i] for i, names in zip(ids, back)))
        out.append(row)
    return out


def _encode_one(g, graph, vocab):
    """-> (object rows [n + 1][A], triplets [[s, p, o], ...]) of graph number g."""
    if not isinstance(graph, dict) or "objects" not in graph or "relationships" not in graph:
        raise _bad(g, "a graph is {\"objects\": [...], \"relationships\": ...}")
    objects, rels = graph["objects"], graph["relationships"]
    if not isinstance(objects, list) or len(objects) == 0:
        raise _bad(g, "empty object list")
    attrs = vocab["attributes"]
    names = list(attrs.keys())
    n = len(objects)
    flat = not isinstance(rels, dict)
    rows = object_ids(objects, vocab, lambda what: _bad(g, what))
    rows.append([attrs[a]["__image__"] for a in names])
    triplets = []
    if flat:
        if not isinstance(rels, list):
            raise _bad(g, "relationships must be a list of [subject, predicate, object] or a dictionary")
        for t in rels:
            if not isinstance(t, (list, tuple)) or len(t) != 3:
                raise _bad(g, "relationship %r is not [subject, predicate, object]" % (t,))
            pid = _pred_id(g, t[1], vocab)
            triplets.append([_index(g, t[0], n, "relationship %r" % (t,)), pid, _index(g, t[2], n, "relationship %r" % (t,))])
    else:
        for name, per_object in rels.items():
            pid = _pred_id(g, name, vocab)
            if not isinstance(per_object, list) or len(per_object) != n:
                raise _bad(g, "relationship %r needs one list of subjects per object (%d)" % (name, n))
            mine = []
            for o1, subjects in enumerate(per_object):
                if not isinstance(subjects, list):
                    raise _bad(g, "relationship %r, object %d: %r is not a list of subjects" % (name, o1, subjects))
                for o2 in subjects:
                    mine.append([_index(g, o2, n, "relationship %r, object %d" % (name, o1)), pid, o1])
            triplets.extend(_reduced(mine, pid))
    if "__in_image__" not in vocab["pred_name_to_idx"]:
        raise _bad(g, "the vocabulary has no predicate '__in_image__'")
    in_image = vocab["pred_name_to_idx"]["__in_image__"]
    triplets.extend([i, in_image, n] for i in range(n))
    return rows, triplets


def load_graphs(path_or_list, vocab):
    """A JSON file (a list of graphs, or one graph) or such a list -> the list of graphs, every one of them checked against
    `vocab` (ValueError with the graph's index and the offending token)."""
    graphs = path_or_list
    if isinstance(path_or_list, (str, bytes)) or hasattr(path_or_list, "__fspath__"):
        with open(path_or_list, "r") as f:
            graphs = json.load(f)
    if isinstance(graphs, dict):
        graphs = [graphs]
    if not isinstance(graphs, list) or len(graphs) == 0:
        raise ValueError("scene graphs: a non-empty list of graphs is needed")
    for g, graph in enumerate(graphs):
        _encode_one(g, graph, vocab)
    return graphs


def encode_graphs(graphs, vocab):
    """-> (objs int64 (B,O,A), triplets int64 (B,T,3), counts int64 (B,)) on the host.  counts[b] is the number of object
    rows of sample b with its `__image__` row, which is the last of them; rows beyond are 0, triplets beyond a sample's own
    are [0, __padding__, 0]."""
    if len(graphs) == 0:
        raise ValueError("scene graphs: a non-empty list of graphs is needed")
    enc = [_encode_one(g, graph, vocab) for g, graph in enumerate(graphs)]
    B, A = len(enc), len(vocab["attributes"])
    O = max(len(r) for r, _ in enc)
    T = max(len(t) for _, t in enc)
    objs = torch.zeros((B, O, A), dtype=torch.int64)
    triplets = torch.zeros((B, T, 3), dtype=torch.int64)
    triplets[:, :, 1] = vocab["pred_name_to_idx"]["__padding__"]
    counts = torch.zeros((B,), dtype=torch.int64)
    for b, (rows, trip) in enumerate(enc):
        objs[b, :len(rows)] = torch.tensor(rows, dtype=torch.int64)
        triplets[b, :len(trip)] = torch.tensor(trip, dtype=torch.int64)
        counts[b] = len(rows)
    return objs, triplets, counts


def triplet_names(triplets, vocab):
    """Encoded triplets (B,T,3) -> per sample the rows [subject, predicate NAME, object] without the padding: what
    scripts/sample.py writes to graphs.json in place of the reference's GraphViz picture."""
    names = vocab["pred_idx_to_name"]
    pad = vocab["pred_name_to_idx"]["__padding__"]
    return [[[int(s), names[int(p)], int(o)] for s, p, o in sample if int(p) != pad] for sample in triplets.tolist()]
