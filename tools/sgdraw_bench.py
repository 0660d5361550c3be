#!/usr/bin/env python
"""Wall time of one `sgdraw.draw_scene_graphs` call ended by a device synchronise: the host layout, one packed upload and
one launch of csg_draw_graph_u8 — launch-and-upload latency, not a kernel time.

    python tools/sgdraw_bench.py host|canonical [--batch 16] [--objects 12] [--calls 20] [--warmup 5]

One mode per process (run them alternately, several rounds); prints one JSON line: the synchronised median, minimum and
maximum per call in milliseconds.  The graphs are seeded flat-form graphs over the synthetic Visual Genome vocabulary:
`--objects` objects and twice as many relationships each.  `host` draws the host-encoded rows in one colour; `canonical`
draws the canonical graph from device tensors (made once, outside the timed window), coloured by type, which adds the
read-back of the triplets to every call.  The bytes are checked against the numpy restatement once, outside the window."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("host", "canonical"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--objects", type=int, default=12)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgdraw_bench needs a HIP device: there is no CPU path")
    import sgdraw_cases as sc
    from canonicalsg2im_amd import authored, sgdraw
    from canonicalsg2im_amd.font5x7 import FONT
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    from canonicalsg2im_amd.synth import make_vocab
    dev = torch.device("cuda:0")
    vocab = make_vocab("vg")
    rng = random.Random(0)
    objects = [n for n in vocab["object_idx_to_name"] if n and not n.startswith("__")]
    preds = [n for n in vocab["pred_idx_to_name"] if n not in ("__in_image__", "__padding__")]
    graphs = []
    for _ in range(a.batch):
        rels = []
        for _ in range(2 * a.objects):
            s, o = rng.sample(range(a.objects), 2)
            rels.append([s, rng.choice(preds), o])
        graphs.append({"objects": [rng.choice(objects) for _ in range(a.objects)], "relationships": rels})
    graphs = authored.load_graphs(graphs, vocab)
    extra = ()
    if a.mode == "canonical":
        objs, rows, counts = authored.encode_graphs(graphs, vocab)
        triplets, _, triplet_type = canonical_triplets(objs.to(dev), None, None, counts, vocab, learned_transitivity=True,
                                                       include_dummies=False, triplets=rows)
        extra = (triplets, triplet_type)
        torch.cuda.synchronize()
    times = []
    for k in range(a.warmup + a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pics = sgdraw.draw_scene_graphs(graphs, vocab, dev, *extra)
        torch.cuda.synchronize()
        if k >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    host = tuple(t.cpu() for t in extra)
    sizes, prims, off, text = sgdraw.layout_batch(graphs, vocab, *host)
    H, W = max(h for _, h in sizes), max(w for w, _ in sizes)
    want = sc.draw_graph(prims, off, text, H, W, sgdraw.DEFAULT_STYLE["background"], FONT)
    for g, (w, h) in enumerate(sizes):
        assert np.array_equal(pics[g].cpu().numpy(), want[g, :, :h, :w]), "picture %d differs from the restatement" % g
    times.sort()
    print(json.dumps({"mode": a.mode, "batch": a.batch, "objects": a.objects, "calls": a.calls,
                      "median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1],
                      "canvas": [H, W], "records": len(prims), "text_bytes": len(text), "bytes": 3 * a.batch * H * W}))


if __name__ == "__main__":
    main()
