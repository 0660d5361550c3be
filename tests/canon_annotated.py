"""Numpy restatement of the canonical graphs of the packed Visual Genome loader, annotated relationships included
(sg2im/data/packed_vg.py:127-142, vg_collate_fn :154-229): the annotated rows, the location relations reduced per
relation, the __in_image__ dummies, np.unique, then add_learnt_triplets over every non-meta predicate
(sg2im/data/base_dataset.py:89-139).  Builds on oracle/canon.py (location_relations, path, hsu, choice_cdf); pinned by
tests/golden/canon_annotated.npz.  Shared by test_canon_annotated_oracle.py and test_gpu_canon_annotated.py."""
import copy

import numpy as np

from canonicalsg2im_amd.synth import make_vocab
from oracle.canon import AUGMENTED, ORIGINAL_EDGE, TRANSITIVE_EDGE, choice_cdf, hsu, location_relations, path


def canonical_graph(objs0, boxes, centers, rows, vocab, learned_transitivity=False, include_dummies=True,
                    learned_converse=False, converse_weights=None, uniforms=None):
    """One sample: (triplets (T,3), triplet_type (T,), conv_counts (P,P+1) float64).  `rows` (R,3) are the annotated
    relationships in local object indices; `uniforms` an iterator over the numbers of the converse draws."""
    objs0 = np.asarray(objs0)
    O = objs0.shape[0]
    p2i = vocab["pred_name_to_idx"]
    n_rel = len(p2i)
    image_id = vocab["object_name_to_idx"]["__image__"]
    real = (objs0 != image_id) if O > 1 else np.zeros(O, bool)               # base_dataset.py:39-41
    adj = location_relations(boxes, centers, real)
    parts = [np.asarray(rows, np.int64).reshape(-1, 3)]                       # packed_vg.py:127-138
    for r, name in enumerate(AUGMENTED):                                      # base_dataset.py:83-87
        s, o = np.nonzero(hsu(path(adj[r])))
        parts.append(np.stack([s, np.full_like(s, p2i[name]), o], axis=1))
    if include_dummies:                                                       # base_dataset.py:141-151
        img = int(np.nonzero(objs0 == image_id)[0].squeeze())
        others = np.array([i for i in range(O) if i != img], np.int64)
        parts.append(np.stack([others, np.full_like(others, p2i["__in_image__"]), np.full_like(others, img)], axis=1))
    trip = np.unique(np.concatenate(parts, axis=0).astype(np.int64), axis=0)
    meta = {p2i["__padding__"], p2i["__in_image__"]}
    non_meta = sorted(set(p2i.values()) - meta)
    conv_counts = np.zeros((n_rel, n_rel + 1))
    new = []
    for rel in non_meta:                                                      # base_dataset.py:99-109
        rel_t = trip[trip[:, 1] == rel]
        if not len(rel_t):
            continue
        new.extend(rel_t.tolist())
        if learned_converse:                                                  # graphs_utils.py:126-152
            cands = [c for c in non_meta if c != rel]
            cdf = choice_cdf(converse_weights, rel, cands)
            vals = cands + [n_rel]
            for t in rel_t:
                r = vals[int(np.searchsorted(cdf, next(uniforms), side="right"))]
                conv_counts[rel, r] += 1
                if r != n_rel:
                    new.append([int(t[2]), r, int(t[0])])
    extra = []
    if learned_transitivity and new:                                          # :111-120, graphs_utils.py:96-100
        arr = np.asarray(new, np.int64)
        for rel in non_meta:
            rel_t = arr[arr[:, 1] == rel]
            if not len(rel_t):
                continue
            N = int(max(rel_t[:, 0].max(), rel_t[:, 2].max()) + 1)
            g = np.zeros((N, N), bool)
            g[rel_t[:, 0], rel_t[:, 2]] = True
            s, o = np.nonzero(path(g) & ~g)
            extra.append(np.stack([s, np.full_like(s, rel), o], axis=1))
    for rel in sorted(meta):                                                  # :122-124
        new.extend(trip[trip[:, 1] == rel].tolist())
    out = np.unique(np.asarray(new, np.int64).reshape(-1, 3), axis=0)         # :127-128
    ttype = [ORIGINAL_EDGE] * len(out)
    if extra:
        extra = np.concatenate(extra, axis=0).astype(np.int64)
        out = np.concatenate([out, extra], axis=0)
        ttype += [TRANSITIVE_EDGE] * len(extra)
    return out, np.asarray(ttype, np.int64), conv_counts


def canonical_batch(objs0, boxes, centers, n_objs, rel, vocab, learned_transitivity=False, include_dummies=True,
                    learned_converse=False, converse_weights=None, uniforms=None):
    """Padded batch as vg_collate_fn pads it (packed_vg.py:207-212): triplets (B,T,3) with [0, __padding__, 0],
    triplet_type (B,T) with 0, per-sample counts and conv_counts (B,P,P+1).  `rel` (B,R,3): annotated rows, padding rows
    carry __padding__.  The samples consume `uniforms` one after the other."""
    pad = vocab["pred_name_to_idx"]["__padding__"]
    it = iter(uniforms) if uniforms is not None else None
    outs, convs = [], []
    for b in range(len(n_objs)):
        n = int(n_objs[b])
        rows = np.asarray(rel[b]).reshape(-1, 3)
        t, tt, cc = canonical_graph(objs0[b][:n], boxes[b][:n], centers[b][:n], rows[rows[:, 1] != pad], vocab,
                                    learned_transitivity, include_dummies, learned_converse, converse_weights, it)
        outs.append((t, tt))
        convs.append(cc)
    T = max([len(t) for t, _ in outs] + [0])
    B = len(outs)
    trip = np.zeros((B, T, 3), np.int64)
    trip[:, :, 1] = pad
    ttype = np.zeros((B, T), np.int64)
    counts = np.zeros(B, np.int64)
    for b, (t, tt) in enumerate(outs):
        trip[b, :len(t)] = t
        ttype[b, :len(t)] = tt
        counts[b] = len(t)
    return trip, ttype, counts, np.stack(convs)


def fixture_case(meta, arrays, ci):
    """Case ci of tests/golden/canon_annotated.npz as int64 / float arrays, conv_counts dense, and its vocabulary."""
    case = meta["cases"][ci]
    g = {k[len("c%d_" % ci):]: v.numpy() for k, v in arrays.items() if k.startswith("c%d_" % ci)}
    vocab = copy.deepcopy(make_vocab(meta["vocab"]))
    names = case["pred_idx_to_name"]
    vocab["pred_idx_to_name"] = list(names)
    vocab["pred_name_to_idx"] = {nm: i for i, nm in enumerate(names)}
    for k in ("objs", "rel", "triplets", "tt"):
        g[k] = g[k].astype(np.int64)
    if case["learned_converse"]:
        B, P = len(case["sizes"]), len(names)
        conv = np.zeros((B * P, P + 1), np.float32)
        conv[g["conv_rows"]] = g["conv_vals"]
        g["conv"] = conv.reshape(B, P, P + 1)
    return case, g, vocab
