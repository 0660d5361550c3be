"""Command-line FID (and Inception score) of folders of pictures, on the device: the reference's
evaluation/fid/fid_score.py with its behaviours kept.

    python -m canonicalsg2im_amd.scripts.quality A B --fid_weights FILE [--dims 2048] [--batch-size 50]
        [--inception_weights FILE --splits 5] [--channel_order bgr|rgb] [--output_dir DIR]

A and B are folders of *.jpg / *.png, or .npz statistics with `mu` and `sigma` (fid_score.py:218-229).  Prints `FID:`; with
--inception_weights also the Inception score of A (a folder).  Writes DIR/quality.json and, for a folder, its statistics as
DIR/stats_A.npz / stats_B.npz.  PIL decodes on the host; everything after the decode runs on the device.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch

_HELP_EPILOG = """behaviours kept from the reference (evaluation/fid/fid_score.py):
  * the remainder of len(files) % batch_size pictures is DROPPED, with the reference's warning (:90-99);
  * the default --channel_order is bgr: the reference reads with cv2.imread and never converts (:111), so its network sees
    blue first.  rgb is what pytorch-fid does.  Numbers of the two orders are not comparable.
--fid_weights is pytorch-fid's pt_inception-2015-12-05-*.pth, --inception_weights torchvision's inception_v3_google-*.pth.
`random` in their place is a seeded stand-in for tests and throughput runs: its numbers mean nothing and every output says
"stand-in".  Loading the real files and the numbers they give are unchecked here."""


def build_parser():
    p = argparse.ArgumentParser(prog="python -m canonicalsg2im_amd.scripts.quality", epilog=_HELP_EPILOG,
                                formatter_class=argparse.RawDescriptionHelpFormatter,
                                description="FID of two sets of pictures (and the Inception score of the first) on the device")
    p.add_argument("A", help="a folder of *.jpg / *.png, or .npz statistics (mu, sigma)")
    p.add_argument("B", help="likewise")
    p.add_argument("--fid_weights", required=True, help="pt_inception-2015-12-05-*.pth, or 'random' (stand-in)")
    p.add_argument("--dims", type=int, default=2048, choices=[64, 192, 768, 2048])
    p.add_argument("--batch-size", type=int, default=50)
    p.add_argument("--inception_weights", default=None, help="inception_v3_google-*.pth, or 'random' (stand-in)")
    p.add_argument("--splits", type=int, default=5)
    p.add_argument("--channel_order", choices=["bgr", "rgb"], default="bgr")
    p.add_argument("--output_dir", default=".")
    return p


def list_files(folder):
    """fid_score.py:225: every *.jpg, then every *.png (sorted here, so that a run can be repeated)."""
    return sorted(glob.glob(os.path.join(folder, "*.jpg"))) + sorted(glob.glob(os.path.join(folder, "*.png")))


def batches(files, batch_size, dev):
    """uint8 (B,H,W,3) device tensors of the reference's batches (:90-99): the remainder is dropped."""
    from PIL import Image
    if not files:
        raise SystemExit("no *.jpg / *.png pictures found")
    if len(files) % batch_size != 0:
        print("Warning: number of images is not a multiple of the batch size. Some samples are going to be ignored.")
    if batch_size > len(files):
        print("Warning: batch size is bigger than the data size. Setting batch size to data size")
        batch_size = len(files)
    for i in range(len(files) // batch_size):
        pics = [np.asarray(Image.open(f).convert("RGB")) for f in files[i * batch_size:(i + 1) * batch_size]]
        if any(p.shape != pics[0].shape for p in pics):
            raise SystemExit("pictures of one batch differ in size (%s): the reference stacks them into one array"
                             % sorted({p.shape for p in pics}))
        yield torch.from_numpy(np.stack(pics)).to(dev)


def main(argv=None):
    args = build_parser().parse_args(argv)
    args.path = [args.A, args.B]
    if not torch.cuda.is_available():
        raise SystemExit("canonicalsg2im_amd needs a HIP device: there is no CPU path")
    from .. import quality
    from ..inception import InceptionV3
    dev = torch.device("cuda", 0)
    for p in args.path:
        if not os.path.exists(p):
            raise SystemExit("Invalid path: %s" % p)
    os.makedirs(args.output_dir, exist_ok=True)
    net = InceptionV3("fid", args.fid_weights).to(dev)
    score_net = InceptionV3("torchvision", args.inception_weights).to(dev) if args.inception_weights else None
    stand_in = net.stand_in or bool(score_net is not None and score_net.stand_in)
    label = "  [stand-in weights: the number means nothing]" if stand_in else ""
    stats, counts, score = [], [], None
    for tag, path in zip("AB", args.path):
        if path.endswith(".npz"):
            stats.append(quality.load_statistics(path))
            counts.append(None)
            continue
        fid = quality.FID(net, dims=args.dims, channel_order=args.channel_order)
        scorer = quality.InceptionScore(score_net, channel_order=args.channel_order) if (score_net is not None and tag == "A") else None
        for pics in batches(list_files(path), args.batch_size, dev):
            fid.update(pics)
            if scorer is not None:
                scorer.update(pics)
        stats.append(fid.statistics())
        counts.append(fid.n)
        quality.save_statistics(os.path.join(args.output_dir, "stats_%s.npz" % tag), *stats[-1])
        if scorer is not None:
            score = scorer.compute(args.splits)
    value = quality.frechet_distance(stats[0][0], stats[0][1], stats[1][0], stats[1][1])
    print("FID: %s%s" % (value, label))
    result = {"fid": value, "dims": args.dims, "batch_size": args.batch_size, "channel_order": args.channel_order,
              "images": counts, "stand_in": stand_in}
    if score is not None:
        print("Inception score (A): %s +- %s%s" % (score[0], score[1], label))
        result["inception_score"] = {"mean": score[0], "std": score[1], "splits": args.splits}
    with open(os.path.join(args.output_dir, "quality.json"), "w") as f:
        json.dump(result, f, indent=1)
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
