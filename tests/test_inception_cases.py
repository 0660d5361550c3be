"""CPU checks of the Inception / FID / Inception-score feature: the case tables and the restatement of
tests/inception_cases.py against torch itself, the package's host side (state-dict keys, BatchNorm folding, tap tables,
refusals) and the host formulas against tests/golden/quality.npz (the reference's own functions, make_golden_quality.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "quality.npz")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    from canonicalsg2im_amd import inception, ops, quality
    return inception, ops, quality


def pool3_rule(x, kind, stride, pad):
    """csg_pool3's arithmetic restated in fp32 numpy: taps inside the picture row by row, left to right; max from -inf; the
    averages from 0, one addition per tap in that order, ONE division by 9 (kind 1) or by the taps inside (kind 2)."""
    x = x.numpy()
    B, C, H, W = x.shape
    OH, OW = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    y = np.zeros((B, C, OH, OW), np.float32)
    for oy in range(OH):
        for ox in range(OW):
            acc = np.full((B, C), -np.inf if kind == 0 else 0.0, np.float32)
            inside = 0
            for dy in range(3):
                for dx in range(3):
                    iy, ix = oy * stride - pad + dy, ox * stride - pad + dx
                    if 0 <= iy < H and 0 <= ix < W:
                        acc = np.maximum(acc, x[:, :, iy, ix]) if kind == 0 else (acc + x[:, :, iy, ix]).astype(np.float32)
                        inside += 1
            y[:, :, oy, ox] = acc if kind == 0 else (acc / np.float32(9 if kind == 1 else inside)).astype(np.float32)
    return torch.from_numpy(y)


def torch_pool(x, kind, stride, pad):
    if kind == 0:
        return F.max_pool2d(x, 3, stride, pad)
    return F.avg_pool2d(x, 3, stride, pad, count_include_pad=kind == 1)


@pytest.mark.parametrize("side", [1, 2, 5])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_pool_rule_is_torchs_own_pool_bit_for_bit(side, kind):
    x = torch.randn(2, 4, side, side, generator=torch.Generator().manual_seed(side))
    for stride, pad in ((1, 1), (2, 0)):
        if side + 2 * pad < 3:
            continue
        assert torch.equal(pool3_rule(x, kind, stride, pad), torch_pool(x, kind, stride, pad)), (side, kind, stride, pad)


def test_state_dict_keys_are_torchvisions(pkg):
    inception = pkg[0]
    shapes = cases.conv_shapes()
    assert len(shapes) == 94
    for variant in ("torchvision", "fid"):
        sd = cases.seeded_state_dict(variant)
        assert len(sd) == 94 * 5 + 2
        net = inception.InceptionV3(variant, sd)
        own = net.state_dict()
        assert set(own) == set(sd) == set(inception.state_dict_keys(variant))
        assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in sd.items()}
        assert own["fc.weight"].shape[0] == (1000 if variant == "torchvision" else 1008)
        for k in ("Conv2d_1a_3x3.conv.weight", "Conv2d_1a_3x3.bn.running_var", "Mixed_7c.branch3x3dbl_3b.bn.bias", "fc.bias"):
            assert k in own and torch.equal(own[k], sd[k])
        # strict: torchvision's extras are the only keys ignored
        extra = dict(sd)
        extra["AuxLogits.fc.weight"] = torch.zeros(3)
        extra["Mixed_5b.branch1x1.bn.num_batches_tracked"] = torch.tensor(0)
        net.load_state_dict(extra)
        with pytest.raises(RuntimeError):
            net.load_state_dict({k: v for k, v in sd.items() if k != "Mixed_6e.branch7x7dbl_5.conv.weight"})
        with pytest.raises(RuntimeError):
            net.load_state_dict(dict(sd, **{"Mixed_8a.conv.weight": torch.zeros(1)}))
    # every channel count but the picture's 3 is a multiple of 4
    assert all(co % 4 == 0 and (ci % 4 == 0 or name == "Conv2d_1a_3x3") for name, (co, ci, _, _) in shapes.items())
    assert [tuple(t[1:5]) for t in inception.layer_table()] == [(ci, co, kh, kw) for (co, ci, kh, kw) in shapes.values()]
    assert [t.name for t in inception.layer_table()] == list(shapes)


def test_constructor_refusals(pkg, monkeypatch):
    inception, _, quality = pkg
    for variant in ("torchvision", "fid"):
        monkeypatch.delenv(inception.WEIGHT_ENV[variant], raising=False)
        with pytest.raises(RuntimeError, match=r"inception_v3_google-\*\.pth.*pt_inception-2015-12-05-\*\.pth"):
            inception.InceptionV3(variant)
    net = inception.InceptionV3("fid", "random")
    assert net.stand_in and not net.training
    with pytest.raises(RuntimeError, match="eval mode only"):
        net.train()
    with pytest.raises(RuntimeError, match="forward only"):
        net(torch.zeros(1, 3, 75, 75, requires_grad=True))
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(1, 3, 75, 75))
    with pytest.raises(ValueError):
        quality.InceptionScore(net)
    with pytest.raises(ValueError):
        quality.FID(inception.InceptionV3("torchvision", "random"))
    assert quality.FID(net, dims=192).stand_in


def test_folded_batchnorm_is_unfolded_batchnorm_in_fp64(pkg):
    inception = pkg[0]
    g = torch.Generator().manual_seed(5)
    w = torch.randn(8, 4, 3, 3, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(8, generator=g, dtype=torch.float64) + 0.5, torch.randn(8, generator=g, dtype=torch.float64)
    mean, var = torch.randn(8, generator=g, dtype=torch.float64), torch.rand(8, generator=g, dtype=torch.float64) + 0.1
    x = torch.randn(2, 4, 6, 6, generator=g, dtype=torch.float64)
    want = F.batch_norm(F.conv2d(x, w, None, 1, 1), mean, var, gamma, beta, False, 0.0, 1e-3)
    wf, bf = inception.fold_batchnorm(w.float(), gamma, beta, mean, var)
    assert wf.dtype == torch.float64 and bf.dtype == torch.float64
    got = F.conv2d(x, inception.fold_batchnorm(w, gamma, beta, mean, var)[0], bf, 1, 1)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_tap_tables_of_rectangular_and_split_filters(pkg):
    ops = pkg[1]
    for KH, KW, ph, pw in ((1, 7, 0, 3), (7, 1, 3, 0), (1, 3, 0, 1), (3, 1, 1, 0)):
        d, OH, OW = ops.conv2d_taps_desc(2, 5, 5, 8, 12, KH, KW, 1, ph, pw, 0, KH * KW)
        assert (OH, OW) == (5, 5) and d.ntaps == d.wtaps == KH * KW
        assert [(d.tap_dy[t], d.tap_dx[t], d.tap_w[t]) for t in range(d.ntaps)] == \
            [(ky - ph, kx - pw, ky * KW + kx) for ky in range(KH) for kx in range(KW)]
    # 5x5: 16 + 9 taps over one weight of 25, every tap once, the second launch accumulates
    a = ops.conv2d_taps_desc(1, 3, 3, 4, 4, 5, 5, 1, 2, 2, 0, 16)[0]
    b = ops.conv2d_taps_desc(1, 3, 3, 4, 4, 5, 5, 1, 2, 2, 16, 9, accumulate=1)[0]
    taps = [(d.tap_dy[t], d.tap_dx[t], d.tap_w[t]) for d in (a, b) for t in range(d.ntaps)]
    assert taps == [(ky - 2, kx - 2, ky * 5 + kx) for ky in range(5) for kx in range(5)]
    assert a.wtaps == b.wtaps == 25 and (a.accumulate, b.accumulate) == (0, 1)
    with pytest.raises(RuntimeError):
        ops.conv2d_taps_desc(1, 3, 3, 4, 4, 5, 5, 1, 2, 2, 0, 25)


def test_restatement_variants_differ_only_in_the_pools():
    """At a 1x1 map every 3x3 pad-1 pool sees one tap: avg over 9 divides it by 9, avg-inside and max return it."""
    x = torch.rand(1, 2048, 1, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    sd = cases.seeded_state_dict("fid")
    fid, tv = cases.Net(sd, "fid"), cases.Net(sd, "torchvision")
    a, b = fid.block("Mixed_7c", x), tv.block("Mixed_7c", x)
    assert torch.equal(a[:, :1856], b[:, :1856]) and not torch.equal(a[:, 1856:], b[:, 1856:])
    assert tuple(a.shape) == (1, 2048, 1, 1)
    for name, cin in cases.BLOCK_CASES:
        y = fid.block(name, torch.rand(1, cin, 5, 5, dtype=torch.float64))
        assert y.shape[1] == {"Mixed_5b": 256, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_7a": 1280}.get(name, 2048)


@pytest.mark.parametrize("D,N", cases.FRECHET_CASES)
def test_frechet_distance_against_the_reference(pkg, D, N, tmp_path):
    """Full rank: 1e-12 (measured 1.0e-15 .. 2.7e-15; three decades for another LAPACK).  Rank-deficient (N <= D): 1e-7
    (measured 5.0e-9, 6.6e-9) — there the reference's sqrtm returns a complex matrix whose imaginary parts reach 2.5e-6 and
    its own number is only that good."""
    quality = pkg[2]
    k = cases.FRECHET_CASES.index((D, N))
    mu1, s1, mu2, s2 = cases.frechet_inputs(D, N, seed=k)
    want = float(np.load(GOLDEN)["frechet_%d_%d" % (D, N)])
    got = quality.frechet_distance(mu1, s1, mu2, s2)
    rel = abs(got - want) / abs(want)
    print("frechet D=%d N=%d: %.17g vs %.17g, rel %.2e" % (D, N, got, want, rel))
    assert rel <= (1e-12 if (D, N) in cases.FRECHET_FULL else 1e-7)
    # the .npz round trip (fid_score.py:218-222)
    path = str(tmp_path / "stats.npz")
    quality.save_statistics(path, mu1, s1)
    m, s = quality.load_statistics(path)
    assert np.array_equal(m, mu1) and np.array_equal(s, s1)
    assert quality.frechet_distance(m, s, mu2, s2) == got


def test_frechet_distance_of_identical_statistics_is_rounding(pkg):
    quality = pkg[2]
    mu, s, _, _ = cases.frechet_inputs(64, 200, seed=0)
    assert abs(quality.frechet_distance(mu, s, mu, s)) <= 1e-10 * np.trace(s)


@pytest.mark.parametrize("N,splits", cases.SCORE_CASES)
def test_score_formula_against_the_reference(N, splits):
    want = np.load(GOLDEN)["score_%d_%d" % (N, splits)]
    mean, std = cases.score_formula(cases.score_probabilities(N), splits)
    assert abs(mean - want[0]) <= 1e-12 * want[0] and abs(std - want[1]) <= 1e-12 * want[0]
