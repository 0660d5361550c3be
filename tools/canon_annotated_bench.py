#!/usr/bin/env python3
"""Timing of the general canonical-graph path (annotated relationships, csg_canon_general_*) on the VG vocabulary with
learned transitivity and converse on, at two sizes: B = 32 x 31 objects and B = 48 x 101 objects (the __image__ object
included).  Device time of one canonical_triplets call between CUDA events (median of --reps; the call's two
read-backs included), per-kernel time from the library's event table, and the CPU time of the numpy restatement
(tests/canon_annotated.py, a checker timed here only as the baseline) for the same batch.
Usage (GPU box): python tools/canon_annotated_bench.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _batch(rng, B, n_objs, vocab):
    from canonicalsg2im_amd.synth import annotated_relations
    n = n_objs - 1
    objs = np.zeros((B, n_objs), np.int64)
    objs[:, :n] = rng.integers(1, len(vocab["object_idx_to_name"]), size=(B, n))
    wh = rng.uniform(0.05, 0.6, size=(B, n, 2))
    xy = rng.uniform(0, 1, size=(B, n, 2)) * (1 - wh)
    boxes = -np.ones((B, n_objs, 4), np.float32)
    boxes[:, :n] = np.concatenate([xy, wh], axis=2)
    cen = np.zeros((B, n_objs, 2), np.float32)
    cen[:, :n] = boxes[:, :n, :2] + np.float32(0.5) * boxes[:, :n, 2:]
    rows = [annotated_relations(rng, n, vocab) for _ in range(B)]
    rel = np.zeros((B, max(len(r) for r in rows), 3), np.int64)
    rel[:, :, 1] = vocab["pred_name_to_idx"]["__padding__"]
    for b, r in enumerate(rows):
        rel[b, :len(r)] = r
    return objs, boxes, cen, np.full(B, n_objs, np.int64), rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import canon_annotated as ca
    from canonicalsg2im_amd import _lib
    from canonicalsg2im_amd.sg2im.data import canonical_triplets
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("vg")
    P = len(vocab["pred_name_to_idx"])
    rng = np.random.default_rng(0)
    w = rng.normal(size=(P, P)).astype(np.float32)
    w = np.triu(w) + np.triu(w).T
    out = {}
    for B, n_objs in ((32, 31), (48, 101)):
        objs, boxes, cen, n, rel = _batch(rng, B, n_objs, vocab)
        u = rng.random(2_000_000)
        d = [torch.from_numpy(x).cuda() for x in (objs, boxes, cen)]
        n_t, rel_t = torch.from_numpy(n), torch.from_numpy(rel)

        def call():
            return canonical_triplets(*d, n_t, vocab, learned_transitivity=True, learned_converse=True,
                                      converse_weights=w, uniforms=u, triplets=rel_t)
        for _ in range(3):
            t, _, tt = call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        _lib.prof_reset(); _lib.prof_enable(True)
        call()
        torch.cuda.synchronize()
        prof = _lib.prof_read(); _lib.prof_enable(False)
        kernels = {name: [round(1000.0 * v[0], 1), v[1]] for name, v in prof.items()}     # us, launches per call
        t0 = time.perf_counter()
        to, tto, _, _ = ca.canonical_batch(objs, boxes, cen, n, rel, vocab, True, True, True, w, u)
        cpu_s = time.perf_counter() - t0
        same = bool(np.array_equal(t.cpu().numpy(), to) and np.array_equal(tt.cpu().numpy(), tto))
        out["B%d_O%d" % (B, n_objs)] = {"device_ms_median": round(float(np.median(ms)), 3),
                                        "device_ms_min": round(float(np.min(ms)), 3), "kernel_us_launches": kernels,
                                        "triplets_per_sample_max": int(t.shape[1]),
                                        "restatement_cpu_s_per_batch": round(cpu_s, 3), "bit_exact": same}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
