"""Device-side pieces of the reference's data pipeline (sg2im/data/*): the canonical graph construction of the packed
datasets — the O(O^3) numpy/python step that feeds the hot path — and the folder datasets that feed it pictures: the three
packed ones and the default `coco` with its sampled-pair graph."""
from .base_dataset import (ANTI_SYMMETRIC_EDGE, ORIGINAL_EDGE, SYMMETRIC_EDGE, TRANSITIVE_EDGE,  # noqa: F401
                           augmented_relations, canonical_triplets, meta_relations, register_augmented_relations)

FOLDER_DATASETS = {        # --dataset -> (the module of this package that holds it, the module's build_*_dataset)
    "coco": ("coco", "build_coco_pairs_dataset"),
    "packed_coco": ("packed_coco", "build_coco_dataset"),
    "packed_clevr": ("packed_clevr", "build_clevr_dataset"),
    "packed_vg": ("packed_vg", "build_vg_dataset"),
}


def build_folder_dataset(args, split):
    """build_*_dataset(args, split) of the folder dataset --dataset names: the dataset (its `builder_class` makes its
    batches), or None when --dataset names none or its files are not there.  The module is imported here, on first use."""
    if args.dataset not in FOLDER_DATASETS:
        return None
    import importlib
    module, build = FOLDER_DATASETS[args.dataset]
    return getattr(importlib.import_module("." + module, __name__), build)(args, split)
