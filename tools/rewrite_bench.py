#!/usr/bin/env python
"""Time of the robustness run's device steps at its shapes (scripts.sample --dataset packed_clevr_syn --rewrite ...): a batch
of seeded synthetic CLEVR scenes with its minimal canonical graph built on the device.

    python tools/rewrite_bench.py [--batch 10] [--min_objects 15] [--max_objects 30] [--mode one_sided] [--share 0.5]
                                  [--calls 200] [--windows 7] [--warmup 20]

Prints one JSON line.  `select_rewrite_us`: one ops.select_location_rows + one ops.rewrite_rows; `consistency_us`: one
ops.layout_consistency of the ground-truth layout against a perturbed one.  Each is device events around a window of
`--calls` back-to-back calls, divided by the calls — the Python calls, their output allocations and two launches each: issue
cost plus kernel time, launch-bound at these sizes — as the median, minimum and maximum over `--windows` windows.  The
entries have no id in the library's per-kernel timing table, so the kernels' own time is a profiler's to give.  Every
output is checked against the numpy restatement once, outside the windows."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _windows(fn, a):
    for _ in range(a.warmup):
        fn()
    out = []
    for _ in range(a.windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(a.calls):
            fn()
        end.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(end) * 1e3 / a.calls)
    out.sort()
    return {"median": out[len(out) // 2], "min": out[0], "max": out[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--min_objects", type=int, default=15)
    ap.add_argument("--max_objects", type=int, default=30)
    ap.add_argument("--mode", default="one_sided", choices=["one_sided", "noise"])
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rewrite_bench needs a HIP device: there is no CPU path")
    import rewrite_cases as rc
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    dev = torch.device("cuda:0")
    ds = syn.SynClevrScenes(a.min_objects, a.max_objects, a.batch, seed=0)
    args = argparse.Namespace(dataset="packed_clevr_syn", vocab=ds.vocab, learned_transitivity=0, learned_converse=0)
    (batch,) = list(syn.SynClevrBatches(ds, args, None, dev).batches([list(range(a.batch))]))
    _, objs, boxes, triplets, _, ttype, _, ids = batch
    ids = ids.to(dev)
    vocab, table = ds.vocab, ds.vocab["pred_name_to_idx"]
    O = int(objs.shape[1])

    def select_rewrite():
        rows, counts = ops.select_location_rows(triplets, ttype, vocab, num_objs=O)
        return rows, counts, ops.rewrite_rows(rows, counts, ids, vocab, a.mode, a.share, "random", 0)

    rows, counts, out = select_rewrite()
    g = torch.Generator().manual_seed(0)
    moved = (boxes.cpu() + 0.05 * torch.randn(boxes.shape, generator=g)).to(dev)      # a layout near the ground truth
    counted = ((boxes != -1).any(-1) & (objs[..., 0] != vocab["object_name_to_idx"]["__image__"])).to(torch.uint8)
    tf, ti = torch.zeros(4, device=dev, dtype=torch.float64), torch.zeros(20, device=dev, dtype=torch.int64)
    cons = ops.layout_consistency(boxes, moved, counted, tf, ti)
    torch.cuda.synchronize()
    want_rows, want_counts = rc.restate_select(triplets.cpu().numpy(), ttype.cpu().numpy(), table, O)
    want_out = rc.restate_rewrite(want_rows, want_counts, ids.cpu().numpy(), table, a.mode, a.share, "random", 0)
    for got, w in ((rows, want_rows), (counts, want_counts), (out, want_out)):
        assert np.array_equal(got.cpu().numpy(), w), "select / rewrite differ from the restatement"
    want = rc.restate_consistency(boxes.cpu().numpy(), moved.cpu().numpy(), counted.cpu().numpy(), np.zeros(4), np.zeros(20, np.int64))
    for got, w in zip(list(cons) + [tf, ti], want):
        assert np.array_equal(got.cpu().numpy(), w, equal_nan=w.dtype.kind == "f"), "layout_consistency differs from the restatement"
    B, T = triplets.shape[:2]
    print(json.dumps({"batch": int(B), "rows_per_sample": int(T), "objects_rows": O, "mode": a.mode, "share": a.share,
                      "selected_rows": int(want_counts.sum()), "rewritten_rows": int((want_out != want_rows).any(-1).sum()),
                      "pairs": int(want[3][:, 19].sum()), "same_pairs": int(want[3][:, 18].sum()), "calls": a.calls,
                      "windows": a.windows, "select_rewrite_us": _windows(select_rewrite, a),
                      "consistency_us": _windows(lambda: ops.layout_consistency(boxes, moved, counted, tf, ti), a)}))


if __name__ == "__main__":
    main()
