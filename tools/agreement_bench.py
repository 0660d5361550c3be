#!/usr/bin/env python
"""Time of one `ops.relation_agreement` call at the shapes of the large-graph run (scripts.sample --dataset packed_clevr_syn):
a batch of seeded synthetic CLEVR scenes, its canonical graph built on the device, boxes perturbed as a prediction would be.

    python tools/agreement_bench.py [--batch 10] [--min_objects 15] [--max_objects 30] [--learned_transitivity 1]
                                    [--calls 200] [--windows 7] [--warmup 20]

Prints one JSON line.  `call_us`: device events around a window of `--calls` back-to-back calls, divided by the calls — two
launches and the call's three output allocations each, so launch-bound at these sizes — as the median, minimum and maximum
over `--windows` windows.  The entry has no id in the library's per-kernel timing table, so the kernels' own time is a
profiler's to give.  The flags and counts are checked against the numpy restatement once, outside the windows."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--min_objects", type=int, default=15)
    ap.add_argument("--max_objects", type=int, default=30)
    ap.add_argument("--learned_transitivity", type=int, default=1)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("agreement_bench needs a HIP device: there is no CPU path")
    import agreement_cases as ac
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd.sg2im.data import packed_clevr_syn as syn
    dev = torch.device("cuda:0")
    ds = syn.SynClevrScenes(a.min_objects, a.max_objects, a.batch, seed=0)
    args = argparse.Namespace(dataset="packed_clevr_syn", vocab=ds.vocab, learned_transitivity=a.learned_transitivity,
                              learned_converse=0)
    (batch,) = list(syn.SynClevrBatches(ds, args, None, dev).batches([list(range(a.batch))]))
    _, objs, boxes, triplets, _, ttype, _, _ = batch
    g = torch.Generator().manual_seed(0)
    pred = (boxes.cpu() + 0.05 * torch.randn(boxes.shape, generator=g)).to(dev)      # a layout near the ground truth
    vocab = ds.vocab
    P = len(vocab["pred_name_to_idx"])
    totals = torch.zeros((4, P, 2), device=dev, dtype=torch.int64)
    outs = ops.relation_agreement(pred, triplets, ttype, vocab, totals)
    torch.cuda.synchronize()
    want = ac.restate(pred.cpu().numpy(), None, triplets.cpu().numpy(), ttype.cpu().numpy(), vocab["pred_name_to_idx"])
    for got, w in zip(list(outs) + [totals], want):
        assert np.array_equal(got.cpu().numpy(), w), "the device differs from the restatement"
    for _ in range(a.warmup):
        ops.relation_agreement(pred, triplets, ttype, vocab, totals)
    windows = []
    for _ in range(a.windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(a.calls):
            ops.relation_agreement(pred, triplets, ttype, vocab, totals)
        end.record()
        torch.cuda.synchronize()
        windows.append(start.elapsed_time(end) * 1e3 / a.calls)
    windows.sort()
    B, T = triplets.shape[:2]
    print(json.dumps({"batch": int(B), "rows_per_sample": int(T), "objects_rows": int(boxes.shape[1]),
                      "tested": int(want[0].sum()), "agreeing": int(want[1].sum()), "calls": a.calls, "windows": a.windows,
                      "call_us": {"median": windows[len(windows) // 2], "min": windows[0], "max": windows[-1]}}))


if __name__ == "__main__":
    main()
