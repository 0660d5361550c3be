"""The normalisation matrix on the CPU (tests/norm_cases.py): `norm_ref64` against torch autograd in float64, the table's
coverage of every path, entry point and kernel corner, and the cap on what a row may mask at LeakyReLU kinks."""
import pytest
import torch

import norm_cases as nc
from norm_cases import CASES, case_ids

RUN = [c for c in CASES if not c["refuse"]]


def _small(c):
    return nc.shrunk(c)


@pytest.mark.parametrize("c", RUN, ids=case_ids(RUN))
def test_ref64_against_torch_autograd(c):
    """Every row (a shrunken twin of the large ones): norm_ref64's outputs, gradients and running statistics agree with
    torch's own operators and autograd in float64 to 1e-10 of each tensor's scale; what is not asked for is None."""
    t = _small(c)
    d = nc.make_data(t)
    nc.mask_kinks(t, d)
    ref, _ = nc.reference(t, d)
    twin = nc.torch_twin(t, d, torch.float64)
    assert set(ref) == set(twin), sorted(set(ref) ^ set(twin))
    for name, r in ref.items():
        if r is None:
            assert twin[name] is None, name
            continue
        assert twin[name] is not None, name
        assert tuple(r.shape) == tuple(twin[name].shape), name
        scale = float(r.abs().max())
        err = float((r - twin[name]).abs().max())
        assert err <= 1e-10 * scale + 1e-300, "%s %s: %.3e of scale %.3e" % (c["name"], name, err, scale)


@pytest.mark.parametrize("c", RUN, ids=case_ids(RUN))
def test_masking_cap(c):
    """At most 0.1 % of a row's incoming gradient is masked (per modulation), judged on the fp64 reference alone."""
    d = nc.make_data(c)
    frac = nc.mask_kinks(c, d)
    assert frac <= nc.MASK_CAP, "%s masks %.4f %% of its gradient" % (c["name"], 100 * frac)
    if all(s == 1.0 for s in c["slopes"]):
        assert frac == 0.0


def _rows(**kw):
    return [c for c in CASES if all((v(c[k]) if callable(v) else c[k] == v) for k, v in kw.items())]


def test_table_covers_every_path_entry_point_and_corner():
    from canonicalsg2im_amd import ops
    names = case_ids()
    assert len(set(names)) == len(names)
    run = [c for c in CASES if not c["refuse"]]
    # every path, directly and through the modules, on one rank and in the N-replica form
    for path in nc.PATHS:
        assert _rows(path=path, via="ops", multi=False, refuse=None), path
        assert _rows(path=path, multi=True), path + " N-replica"
        assert [c for c in run if c["via"] in ("spade", "pair", "block0") and c["path"] == path], path + " module"
    entries = {e for c in run for e in c["calls"]}
    assert entries == {"norm_act", "norm_act_pair", "spade_joined", "spade_fused"}, entries
    assert {c["via"] for c in run} >= {"ops", "affine2d", "affine1d", "affine_sync", "spade", "pair", "block0"}
    for via in ("spade", "pair"):
        assert _rows(via=via, training=True) and _rows(via=via, training=False), via
    # both invstd forms, the variance below eps and the constant channel in both
    assert _rows(multi=True, sigma=lambda s: s * s < 1e-5, const=None) and _rows(multi=True, const=lambda v: v is not None)
    assert _rows(multi=False, const=lambda v: v is not None)
    # _NormAct's options
    na = lambda **kw: _rows(path="_NormAct", via="ops", **kw)
    for instance in (False, True):
        for training in (False, True):
            assert na(instance=instance, training=training), (instance, training)
        for mod in ("none", "gb"):
            assert na(instance=instance, mod=mod), (instance, mod)
    for slope in (1.0, 0.2, 0.0):
        assert na(slopes=(slope,), mod="gb") and na(slopes=(slope,), mod="none"), slope
    assert na(running=(False,), instance=False) and na(momentum=lambda m: m != 0.1)
    assert na(need="g") and na(xfmt="cl") and na(xfmt="slice")
    # the kernels' corners
    for C in (4, 12, 20, 1024, 1040, 2048):
        assert na(C=C), C
    assert [c for c in na() if c["C"] > 1024 and c["C"] % 1024] and [c for c in na() if c["C"] >= 2048]
    P = lambda c: c["H"] * c["W"] * (1 if c["instance"] else c["B"])
    assert [c for c in na() if P(c) < 32 and ops._chunks(P(c)) == 1]
    empty = [c for c in na() if -(-P(c) // ops._chunks(P(c))) * (ops._chunks(P(c)) - 1) >= P(c)]
    assert empty and any(P(c) == 40000 for c in empty), "no row with empty trailing chunks"
    assert na(instance=True, H=129, W=129)
    assert na(instance=False, mean_term=True, offset=lambda m: m >= 100 * 1.7)
    assert na(instance=True, H=129, mean_term=True, offset=lambda m: m >= 100 * 1.7)
    assert all(c["offset"] / c["sigma"] >= 100 for c in CASES if c["mean_term"])
    # affine norms: (N, C), (N, C, L), (N, C, H, W); N = 1 (count 1) and N = 3
    aff = _rows(mod="affine", refuse=None)
    assert {len(c["shape"]) if c["shape"] else 4 for c in aff} == {2, 3, 4}
    assert [c for c in aff if c["B"] * c["H"] * c["W"] == 1] and [c for c in aff if c["B"] == 3]
    assert {c["via"] for c in aff} == {"affine2d", "affine1d", "affine_sync"}
    # _NormActPair
    pr = _rows(path="_NormActPair", via="ops")
    assert [c for c in pr if c["slopes"][0] != c["slopes"][1]] and [c for c in pr if c["running"] != (True, True)]
    # _SpadeJoined
    sj = _rows(path="_SpadeJoined", via="ops", multi=False)
    assert {(c["H"], c["W"]) for c in sj} == {(8, 8), (16, 16)}
    assert [c for c in sj if c["C"] % 8 == 4] and [c for c in sj if c["C"] == 64] and [c for c in sj if c["C"] == 1024]
    assert [c for c in sj if c["in_slope"] is None] and [c for c in sj if c["in_slope"] is not None]
    assert [c for c in sj if c["need"] not in ("xawb",)]
    # _SpadeFused: every launch the stage / item rule can give, computed from the rule
    sf = [c for c in _rows(path="_SpadeFused", refuse=None)]
    for c in sf:
        assert c["launch"] == tuple(nc.joint_rule(c, k) for k in range(c["K"])), c["name"]
        assert c["C"] % 32 == 0 and c["H"] % 4 == 0 and c["W"] % 4 == 0 and c["W"] >= 32 and c["H"] >= 16, c["name"]
    one = [c for c in sf if c["via"] == "ops" and not c["multi"]]
    for K in (1, 2):
        for launch in ("pair", "joint"):
            assert [c for c in one if c["K"] == K and c["launch"] == (launch,) * K], (K, launch)
    mixed = [c for c in one if c["K"] == 2 and set(c["launch"]) == {"pair", "joint"}]
    assert mixed and all(sorted(c["nh"]) == [120, 128] and c["slopes"][0] != c["slopes"][1] for c in mixed)
    big = lambda c: nc.joint_items(c) >= 2 * nc.MI355X_CUS
    assert [c for c in one if big(c) and c["knobs"].get("SPADE_JOINT") is False and c["launch"] == ("pair",)]
    assert [c for c in one if big(c) and not c["persistent"] and c["launch"] == ("pair",)]
    assert [c for c in sf if c["multi"] and big(c) and c["K"] == 1] and [c for c in sf if c["multi"] and big(c) and c["K"] == 2]
    assert {c["C"] for c in one} >= {32, 96, 128} and [c for c in one if (c["H"], c["W"]) == (16, 32)]
    assert [c for c in one if "x" not in c["need"]] and [c for c in one if "w" not in c["need"]]
    assert [c for c in one if 0.0 in c["slopes"]]
    # refusals
    assert len(_rows(refuse=lambda r: r is not None)) >= 3
    # nothing near 2^31 elements
    assert all(c["B"] * max(c["C"] * 2, (c["nh"] or (0,))[0]) * c["H"] * c["W"] < 2 ** 27 for c in CASES)
