"""Turn a packed Visual Genome split file (.h5, as the reference's scripts/preprocess_packed_vg.py writes it) into the .npz
that sg2im/data/packed_vg.py of this package reads with numpy alone.

    python tools/vg_h5_to_npz.py datasets/vg/train.h5 [-o datasets/vg/train.npz]

Needs h5py, which is imported inside main(): run it where h5py exists.  Every dataset of the file is copied under its own
name, image_paths as fixed-width bytes (no pickling).  NOT TESTED beyond its argument handling (--help, a missing file):
h5py is not installed where this package is built and tested."""
import argparse
import os
import sys

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("h5", help="the split file to read")
    ap.add_argument("-o", "--output", help="the .npz to write (default: the input's name with .npz)")
    a = ap.parse_args(argv)
    if not os.path.isfile(a.h5):
        ap.error("%s: no such file" % a.h5)
    import h5py
    out = a.output or os.path.splitext(a.h5)[0] + ".npz"
    with h5py.File(a.h5, "r") as f:
        arrays = {k: np.asarray(v) for k, v in f.items()}
    if "image_paths" in arrays:
        arrays["image_paths"] = np.asarray([p if isinstance(p, bytes) else str(p).encode() for p in arrays["image_paths"].tolist()])
    np.savez(out, **arrays)
    print("%s: %s" % (out, ", ".join("%s %s" % (k, v.shape) for k, v in arrays.items())))


if __name__ == "__main__":
    main(sys.argv[1:])
