#!/usr/bin/env python
"""Timing of the box-outline launch (csg_draw_boxes_u8) against the only way to the same picture without it: copy the
uint8 batch to the host and paint there with the numpy restatement of the rule (tests/overlay_cases.py).

    python tools/overlay_bench.py device|host|labels [--batch 16] [--size 256] [--objects 31] [--calls 20] [--warmup 5]

One mode per process (run them alternately, several rounds); prints one JSON line: the synchronised median, minimum and
maximum per call in milliseconds.  All modes start from the same seeded device tensors and the host mode's result is
checked against the device's bytes once, outside the timed window.  `labels` is the outline launch followed by the label
launch (csg_draw_labels_u8: seeded names of 6 to 12 small letters, packed and uploaded inside the timed call, as a caller
pays for them), to be set beside `device`, the outlines alone."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("device", "host", "labels"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--objects", type=int, default=31)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_bench needs a HIP device: there is no CPU path")
    import overlay_cases as oc
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd.authored import DEFAULT_PALETTE
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    B, H, O = a.batch, a.size, a.objects
    img = torch.randint(0, 256, (B, 3, H, H), generator=g, dtype=torch.uint8).to(dev)
    wh = torch.rand((B, O, 2), generator=g) * 0.55 + 0.05
    xy = torch.rand((B, O, 2), generator=g) * (1.0 - wh)
    boxes = torch.cat([xy, wh], dim=2).to(dev)
    objs = torch.randint(1, 100, (B, O + 1, 1), generator=g)
    objs[:, O] = 0                                                        # the __image__ row
    boxes = torch.cat([boxes, torch.tensor([0.0, 0.0, 1.0, 1.0], device=dev).expand(B, 1, 4)], dim=1).contiguous()
    objs = objs.to(dev)
    pal_host = np.asarray(DEFAULT_PALETTE, np.uint8)
    pal = torch.from_numpy(pal_host).to(dev)

    def device_call():
        out = ops.draw_boxes_u8(img, boxes, objs, 0, pal, 2)
        torch.cuda.synchronize()
        return out

    def host_call():
        return oc.draw_boxes(img.cpu().numpy(), boxes.cpu().numpy(), objs.cpu().numpy(), 0, pal_host, 2)

    names = [["".join(chr(97 + int(c)) for c in torch.randint(0, 26, (int(torch.randint(6, 13, (1,), generator=g)),), generator=g))
              for _ in range(O)] + [None] for _ in range(B)]

    def labels_call():
        out = ops.draw_labels_u8(ops.draw_boxes_u8(img, boxes, objs, 0, pal, 2), boxes, objs, 0, pal, names)
        torch.cuda.synchronize()
        return out

    call = {"device": device_call, "host": host_call, "labels": labels_call}[a.mode]
    times = []
    for k in range(a.warmup + a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        if k >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    want = (labels_call() if a.mode == "labels" else device_call()).cpu().numpy()
    got = out.cpu().numpy() if torch.is_tensor(out) else out
    assert np.array_equal(got, want), "the two ways disagree"
    times.sort()
    print(json.dumps({"mode": a.mode, "batch": B, "size": H, "objects": O, "calls": a.calls,
                      "median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1],
                      "bytes": 6 * B * H * H, "painted_bytes": int((want != img.cpu().numpy()).sum())}))


if __name__ == "__main__":
    main()
