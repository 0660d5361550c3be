#!/usr/bin/env python3
"""Generate tests/golden/quality.npz by running the REFERENCE's own `calculate_frechet_distance`
(evaluation/fid/fid_score.py:136-190) and `InceptionScore.compute_score` (evaluation/inception.py:35-49) on the CPU.

Runs only where a checkout of the reference and scipy are at hand; nothing of the reference travels: the output is one
`.npz` of the numbers the reference returned for the seeded inputs of tests/inception_cases.py.  Usage:
    python tests/golden/make_golden_quality.py REFERENCE_ROOT

cv2 and torchvision are absent here: stub modules stand in for them (the two functions never touch either), with
`torchvision.models.inception.InceptionA/C/E` as empty classes for the `class FIDInception*(…)` statements.  The
`InceptionScore` object is built with `__new__` and given `preds` — the substitution precedent of make_golden_coco.py: its
constructor would download a network.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "evaluation")):
    raise SystemExit("usage: make_golden_quality.py REFERENCE_ROOT  (the reference's checkout: it holds evaluation/)")
sys.path.insert(0, os.path.abspath(sys.argv[1]))
sys.path.insert(0, os.path.dirname(HERE))         # tests/: the seeded inputs are made by tests/inception_cases.py


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Empty:
    def __init__(self, *a, **k):
        pass


_mod("cv2")
tv = _mod("torchvision")
tv.models = _mod("torchvision.models", inception_v3=_Empty)
tv.models.inception = _mod("torchvision.models.inception", InceptionA=_Empty, InceptionC=_Empty, InceptionE=_Empty,
                           inception_v3=_Empty)
_mod("torchvision.models.utils", load_state_dict_from_url=_Empty)

from evaluation.fid.fid_score import calculate_frechet_distance  # noqa: E402  (reference)
from evaluation.inception import InceptionScore  # noqa: E402  (reference)

import inception_cases as cases  # noqa: E402  (ours: inputs only)


def main():
    out = {}
    for k, (D, N) in enumerate(cases.FRECHET_CASES):
        mu1, s1, mu2, s2 = cases.frechet_inputs(D, N, seed=k)
        out["frechet_%d_%d" % (D, N)] = np.float64(calculate_frechet_distance(mu1, s1, mu2, s2))
    for N, splits in cases.SCORE_CASES:
        obj = InceptionScore.__new__(InceptionScore)
        obj.preds = cases.score_probabilities(N)
        mean, std = obj.compute_score(splits=splits)
        out["score_%d_%d" % (N, splits)] = np.array([mean, std], np.float64)
    np.savez(os.path.join(HERE, "quality.npz"), **out)
    for k, v in out.items():
        print(k, v)


if __name__ == "__main__":
    main()
