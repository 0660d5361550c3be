"""Device-side pieces of the reference's data pipeline (sg2im/data/*): the canonical graph construction of the packed
datasets — the O(O^3) numpy/python step that feeds the hot path — and the folder datasets that feed it pictures: the three
packed ones, the default `coco` with its sampled-pair graph, `vg` with its annotated-only graph and `clevr` with the renderer's
relations reduced to their minimal graphs; and `packed_clevr_syn`, synthetic CLEVR scenes without pictures, for the large-graph run."""
from .base_dataset import (ANTI_SYMMETRIC_EDGE, ORIGINAL_EDGE, SYMMETRIC_EDGE, TRANSITIVE_EDGE,  # noqa: F401
                           annotated_triplets, augmented_relations, canonical_triplets, clevr_triplets, meta_relations,
                           register_augmented_relations)

FOLDER_DATASETS = {        # --dataset -> (the module of this package that holds it, the module's build_*_dataset)
    "clevr": ("clevr", "build_clevr_dialog_dataset"),
    "coco": ("coco", "build_coco_pairs_dataset"),
    "packed_coco": ("packed_coco", "build_coco_dataset"),
    "packed_clevr": ("packed_clevr", "build_clevr_dataset"),
    "packed_clevr_syn": ("packed_clevr_syn", "build_clevr_syn_dataset"),      # no folder: scenes drawn from a seed
    "packed_vg": ("packed_vg", "build_vg_dataset"),
    "vg": ("vg", "build_vg_unpacked_dataset"),
}


def build_folder_dataset(args, split):
    """build_*_dataset(args, split) of the folder dataset --dataset names: the dataset (its `builder_class` makes its
    batches), or None when --dataset names none or its files are not there.  The module is imported here, on first use."""
    if args.dataset not in FOLDER_DATASETS:
        return None
    import importlib
    module, build = FOLDER_DATASETS[args.dataset]
    return getattr(importlib.import_module("." + module, __name__), build)(args, split)


def looked_for(args, split):
    """What `build_folder_dataset(args, split)` looks for, for the message of a caller that cannot go on without the folder:
    the image directory of the split (the dataset module's own `split_image_dir`; Visual Genome also needs its split file)."""
    if args.dataset not in FOLDER_DATASETS:
        return "a folder dataset (--dataset %s names none: %s)" % (args.dataset, ", ".join(sorted(FOLDER_DATASETS)))
    import importlib
    module = importlib.import_module("." + FOLDER_DATASETS[args.dataset][0], __name__)
    where = module.split_image_dir(args, split)
    if args.dataset == "packed_vg":
        import os
        where = "%s with %s (.h5 or .npz)" % (where, getattr(args, "%s_h5" % split) or os.path.join(args.dataroot, "vg", "%s.h5" % split))
    if args.dataset == "vg":
        where = "%s with %s (.h5 or .npz)" % (where, module.split_path(args, split))
    return where
