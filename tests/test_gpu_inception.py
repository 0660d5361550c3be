"""Device tests of the Inception / FID / Inception-score feature (csrc/inception.hip, canonicalsg2im_amd/inception.py,
quality.py) against the CPU restatement of tests/inception_cases.py.  Everything runs the seeded weights of that file: the
real weight files have never been loaded.

Kernels with a bit-exact host counterpart (pools, identity resize) are held to equality.  Everything that sums in fp32 is
judged like the project's other fp32 paths (tests/fp64_band.py): against the fp64 restatement, the device's relative L2
error must be <= 3 x the error of the SAME restatement evaluated in fp32 by torch on the CPU + 1e-4, and the max-norm error
likewise (ReLU outputs are continuous: no gate-flip allowance)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_cases as cases
from conftest import ROOT
from fp64_band import errors

pytestmark = pytest.mark.gpu

K_L2, FLOOR = 3.0, 1e-4                     # fp64_band.Band's constants
GOLDEN = os.path.join(ROOT, "tests", "golden", "quality.npz")
_TABLE = []
REPORT = os.environ.get("INCEPTION_ERRORS_REPORT")          # a file that receives the table too (profiles/inception_errors.txt)


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def judge(name, hip, ref32, ref64):
    h_l2, h_mx = errors(hip, ref64)
    r_l2, r_mx = errors(ref32, ref64)
    _TABLE.append("%-44s %10.2e %10.2e %10.2e %10.2e" % (name, h_l2, r_l2, h_mx, r_mx))
    print(_TABLE[-1])
    assert h_l2 <= K_L2 * r_l2 + FLOOR and h_mx <= K_L2 * r_mx + FLOOR, \
        "%s: hip l2 %.2e (fp32 ref %.2e), hip max %.2e (fp32 ref %.2e)" % (name, h_l2, r_l2, h_mx, r_mx)
    return h_l2, h_mx


@pytest.fixture(scope="module", autouse=True)
def dump_table():
    yield
    if _TABLE and REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(REPORT)), exist_ok=True)
        with open(REPORT, "w") as f:
            f.write("%-44s %10s %10s %10s %10s\n" % ("output (error vs the fp64 restatement)", "hip l2", "fp32ref l2", "hip max",
                                                      "fp32ref max"))
            f.write("\n".join(_TABLE) + "\n")


def to_dev(x, cuda):
    """CPU (B,C,H,W) -> device tensor with NHWC memory."""
    from canonicalsg2im_amd import ops
    return ops.nhwc(x.float().to(cuda))


@functools.lru_cache(maxsize=None)
def state(variant):
    return cases.seeded_state_dict(variant)


@functools.lru_cache(maxsize=None)
def device_net(variant):
    from canonicalsg2im_amd import inception
    return inception.InceptionV3(variant, state(variant)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def host_net(variant, dtype):
    return cases.Net(state(variant), variant, dtype)


# ------------------------------------------------------------------------------------------------ csg_pool3
@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("side", [1, 2, 3, 7, 8])
def test_pool3_is_torchs_pool_bit_for_bit_and_writes_only_its_slice(cuda, side, C):
    """The order: taps inside the picture row by row, left to right, one fp32 addition each from 0, one division at the end
    (by 9, or by the number of taps inside) — torch's host avg_pool2d; max from -inf."""
    from canonicalsg2im_amd import ops
    x = torch.randn(2, C, side, side, generator=torch.Generator().manual_seed(side * 100 + C))
    xd = to_dev(x, cuda)
    for stride, pad in ((1, 1), (2, 0)):
        if side + 2 * pad < 3:
            with pytest.raises(RuntimeError):
                ops.pool3(xd, ops.POOL_MAX, stride, pad)
            continue
        for kind in (ops.POOL_MAX, ops.POOL_AVG9, ops.POOL_AVG_INSIDE):
            want = F.max_pool2d(x, 3, stride, pad) if kind == ops.POOL_MAX else \
                F.avg_pool2d(x, 3, stride, pad, count_include_pad=kind == ops.POOL_AVG9)
            assert torch.equal(ops.pool3(xd, kind, stride, pad).cpu(), want), (kind, stride, pad)
            wide = torch.full((2, C + 12, want.shape[2], want.shape[3]), 7.5, device=cuda)
            wide = ops.nhwc(wide)
            ops.pool3(xd, kind, stride, pad, out=wide, out_off=4)
            got = wide.cpu()
            assert torch.equal(got[:, 4:4 + C], want)
            assert bool((got[:, :4] == 7.5).all()) and bool((got[:, 4 + C:] == 7.5).all())


def test_spatial_mean(cuda):
    from canonicalsg2im_amd import ops
    for (B, C, H, W) in ((2, 64, 1, 1), (3, 68, 5, 7), (1, 192, 35, 35)):
        x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C))
        judge("spatial_mean %dx%dx%dx%d" % (B, C, H, W), ops.spatial_mean(to_dev(x, cuda)), x.mean((2, 3)), x.double().mean((2, 3)))


# ------------------------------------------------------------------------------------------------ convolutions
def conv_case(cuda, name, B, Cin, Cout, H, W, KH, KW, stride, pad, seed=0, slice_off=None, w=None, x=None, bias=True):
    from canonicalsg2im_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g) if x is None else x
    w = torch.randn(Cout, Cin, KH, KW, generator=g) * (2.0 / (Cin * KH * KW)) ** 0.5 if w is None else w
    b = 0.3 * torch.randn(Cout, generator=g) if bias else None
    ref64 = F.relu(F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride, pad))
    ref32 = F.relu(F.conv2d(x, w, b, stride, pad))
    pc = (-Cin) % 4
    xp, wp = F.pad(x, (0, 0, 0, 0, 0, pc)), F.pad(w, (0, 0, 0, 0, 0, pc))
    wd = wp.permute(0, 2, 3, 1).contiguous().to(cuda)
    bd = None if b is None else b.to(cuda)
    if slice_off is None:
        y = ops.conv2d_forward(to_dev(xp, cuda), wd, bd, KH, KW, stride, pad, ops.ACT_LEAKY, 0.0)
    else:
        wide = ops.nhwc(torch.full((B, Cout + slice_off + 8) + tuple(ref64.shape[2:]), -3.25, device=cuda))
        ops.conv2d_forward(to_dev(xp, cuda), wd, bd, KH, KW, stride, pad, ops.ACT_LEAKY, 0.0, out=wide, out_off=slice_off)
        got = wide.cpu()
        assert bool((got[:, :slice_off] == -3.25).all()) and bool((got[:, slice_off + Cout:] == -3.25).all()), name
        y = got[:, slice_off:slice_off + Cout]
    assert tuple(y.shape) == tuple(ref64.shape), name
    judge(name, y, ref32, ref64)
    return y.cpu()


def test_rectangular_convolutions(cuda):
    # (1,7) and (7,1) on W or H of 5: the taps leave both edges; (1,3) and (3,1) on a 1x1 map: only the centre tap is inside
    conv_case(cuda, "conv 1x7 on 5x5", 2, 16, 24, 5, 5, 1, 7, 1, (0, 3), seed=1)
    conv_case(cuda, "conv 7x1 on 5x5", 2, 16, 24, 5, 5, 7, 1, 1, (3, 0), seed=2, slice_off=8)
    conv_case(cuda, "conv 1x7 on 7x5 (H != W)", 2, 16, 24, 7, 5, 1, 7, 1, (0, 3), seed=3)
    conv_case(cuda, "conv 1x3 on 1x1", 2, 384, 384, 1, 1, 1, 3, 1, (0, 1), seed=4, slice_off=320)
    conv_case(cuda, "conv 3x1 on 1x1", 2, 384, 384, 1, 1, 3, 1, 1, (1, 0), seed=5)


def test_strided_and_padded_input_convolutions(cuda):
    conv_case(cuda, "conv 3x3 s2 on 7 -> 3", 2, 32, 32, 7, 7, 3, 3, 2, (0, 0), seed=6)
    conv_case(cuda, "conv 3x3 s2 on 8 -> 3", 2, 32, 32, 8, 8, 3, 3, 2, (0, 0), seed=7, slice_off=4)
    conv_case(cuda, "conv 3x3 s2 Cin=3 padded to 4", 2, 3, 32, 9, 9, 3, 3, 2, (0, 0), seed=8)


def test_five_by_five_is_the_sum_of_two_launches_with_relu_on_the_sum(cuda):
    conv_case(cuda, "conv 5x5 on 3x3", 2, 48, 64, 3, 3, 5, 5, 1, (2, 2), seed=9)
    conv_case(cuda, "conv 5x5 on 35x35", 2, 48, 64, 35, 35, 5, 5, 1, (2, 2), seed=10, slice_off=64)
    # taps 0..15 weigh +1, taps 16..24 weigh -3, x = 1: at the centre of a 3x3 map the first launch sees taps 6, 7, 8, 11,
    # 12, 13 (+6 Cin) and the second 16, 17, 18 (-9 Cin): the first partial is positive, the sum negative
    Cin, Cout = 4, 4
    w = torch.ones(Cout, Cin, 25)
    w[:, :, 16:] = -3.0
    w = w.view(Cout, Cin, 5, 5)
    x = torch.ones(1, Cin, 3, 3)
    first = F.conv2d(x, torch.where(w > 0, w, torch.zeros(())), None, 1, 2)
    total = F.conv2d(x, w, None, 1, 2)
    assert float(first[0, 0, 1, 1]) == 6 * Cin and float(total[0, 0, 1, 1]) == -3 * Cin
    y = conv_case(cuda, "conv 5x5 partial > 0, sum < 0", 1, Cin, Cout, 3, 3, 5, 5, 1, (2, 2), w=w, x=x, bias=False)
    assert float(y[0, 0, 1, 1]) == 0.0 and torch.equal(y, F.relu(total))
    assert float(F.relu(first)[0, 0, 1, 1]) > 0           # what a ReLU on the first partial would have left there


def test_forward_only_entry_refuses_gradients(cuda):
    from canonicalsg2im_amd import ops
    x = to_dev(torch.randn(1, 4, 3, 3), cuda).requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward only"):
        ops.conv2d_forward(x, torch.zeros(4, 1, 3, 4, device=cuda), None, 1, 3, 1, (0, 1))


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("src", [(64, 64), (256, 256), (480, 320), (299, 299)])
def test_resize_bilinear(cuda, src):
    """Against F.interpolate in fp64.  Bound: the source coordinate is formed in fp32 as torch forms it; its rounding error
    is at most 2 ulp of a coordinate below 512 (2 x 3.1e-5), which moves a value by at most that times the largest step
    between neighbouring pixels (<= 1 here), times |a|; the four products and three sums add < 1e-6."""
    from canonicalsg2im_amd import ops
    H, W = src
    g = torch.Generator().manual_seed(H + W)
    u8 = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    f32 = torch.rand(2, 3, H, W, generator=g)
    for a, b, rev in ((1.0, 0.0, False), (2.0, -1.0, False), (2.0, -1.0, True)):
        for kind, x_dev, x64 in (("u8", u8.to(cuda), (u8.float() / 255).double().permute(0, 3, 1, 2)),
                                 ("f32", to_dev(f32, cuda), f32.double())):
            want = F.interpolate(x64.flip(1) if rev else x64, size=(299, 299), mode="bilinear", align_corners=False) * a + b
            got = ops.resize_bilinear(x_dev, (299, 299), a, b, reverse=rev).cpu()
            assert tuple(got.shape) == (2, 4, 299, 299) and bool((got[:, 3] == 0).all())
            err = float((got[:, :3].double() - want).abs().max())
            print("resize %s %dx%d a=%g rev=%d: max err %.2e" % (kind, H, W, a, rev, err))
            assert err <= abs(a) * 2 * 2.0 ** -15 + 1e-6
            if src == (299, 299) and a == 1.0:
                assert torch.equal(got[:, :3], x64.float())            # identity: bit for bit


# ------------------------------------------------------------------------------------------------ feature statistics
@pytest.mark.parametrize("n,D", [(1, 64), (7, 64), (50, 192), (3, 2048)])
def test_feat_stats_two_updates(cuda, n, D):
    """Gate 1e-12 of max|sigma|: fp64 eps 1.1e-16 x N <= 200 terms x the one-pass amplification (mu^2 + sigma^2) / sigma^2 = 4
    for uniform [0,1) features ~ 1e-13."""
    from canonicalsg2im_amd import ops
    g = torch.Generator().manual_seed(n * D)
    parts = [torch.rand(n, D, generator=g), torch.rand(n, D, generator=g)]
    total = torch.zeros(D, device=cuda, dtype=torch.float64)
    outer = torch.zeros(D, D, device=cuda, dtype=torch.float64)
    for p in parts:
        ops.feat_stats(p.to(cuda), total, outer)
    mu, sigma = ops.feat_stats_finalize(total, outer, 2 * n)
    act = torch.cat(parts).double().numpy()
    want_mu, want_sigma = np.mean(act, axis=0), np.cov(act, rowvar=False)
    sigma = sigma.cpu().numpy()
    err = np.abs(sigma - want_sigma).max() / np.abs(want_sigma).max()
    print("feat_stats n=2x%d D=%d: sigma err %.2e of max|sigma|" % (n, D, err))
    assert err <= 1e-12
    assert np.abs(mu.cpu().numpy() - want_mu).max() <= 1e-14
    assert np.array_equal(sigma, sigma.T)


def test_feat_stats_of_one_row_is_numpys_nan_covariance(cuda):
    from canonicalsg2im_amd import ops
    x = torch.rand(1, 64, generator=torch.Generator().manual_seed(3))
    total = torch.zeros(64, device=cuda, dtype=torch.float64)
    outer = torch.zeros(64, 64, device=cuda, dtype=torch.float64)
    ops.feat_stats(x.to(cuda), total, outer)
    mu, sigma = ops.feat_stats_finalize(total, outer, 1)
    assert torch.equal(mu.cpu(), x[0].double()) and bool(torch.isnan(sigma).all())
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert np.isnan(np.cov(x.double().numpy(), rowvar=False)).all()


# ------------------------------------------------------------------------------------------------ Inception score
@pytest.mark.parametrize("N,splits", cases.SCORE_CASES)
def test_inception_score_kernel(cuda, N, splits):
    from canonicalsg2im_amd import ops
    probs = cases.score_probabilities(N)
    out = ops.inception_score(torch.from_numpy(probs).to(cuda), splits).cpu().numpy()
    mean, std = cases.score_formula(probs, splits)
    want = np.load(GOLDEN)["score_%d_%d" % (N, splits)]
    print("score N=%d splits=%d: %.15g +- %.15g (formula %.15g +- %.15g)" % (N, splits, out[0], out[1], mean, std))
    assert out.shape == (2 + splits,)
    assert abs(out[0] - mean) <= 1e-12 * mean and abs(out[1] - std) <= 1e-12 * mean
    assert abs(out[0] - want[0]) <= 1e-12 * want[0] and abs(out[1] - want[1]) <= 1e-12 * want[0]


def test_softmax_rows(cuda):
    from canonicalsg2im_amd import ops
    logits = torch.randn(5, 1000, generator=torch.Generator().manual_seed(8)) * 3
    got = ops.softmax_rows(logits.to(cuda)).cpu()
    assert got.dtype == torch.float64
    want = F.softmax(logits.double(), dim=1)
    # fp32: exp to ~2 ulp, a 1000-term sum, one division
    assert float(((got - want).abs() / want).max()) <= 2e-6
    assert torch.equal(got, got.float().double())           # fp32 values, widened


# ------------------------------------------------------------------------------------------------ blocks and the whole net
@pytest.mark.parametrize("variant", ["torchvision", "fid"])
def test_every_block_type_at_5x5(cuda, variant):
    net = device_net(variant)
    for name, cin in cases.BLOCK_CASES:
        x = torch.rand(2, cin, 5, 5, generator=torch.Generator().manual_seed(cin)) * 2
        y = net.run_block(name, to_dev(x, cuda))
        judge("%s %s 5x5" % (variant, name), y, host_net(variant, torch.float32).block(name, x),
              host_net(variant, torch.float64).block(name, x))


@functools.lru_cache(maxsize=None)
def whole_net_75(variant):
    """(x, fp32 restatement, fp64 restatement) on a 75x75 input: maps 37 -> 35 -> 17 -> 15 -> 7 -> 3 -> 1."""
    x = torch.randn(2, 3, 75, 75, generator=torch.Generator().manual_seed(75))
    return x, host_net(variant, torch.float32)(x), host_net(variant, torch.float64)(x)


def test_whole_network_on_75x75_fid_every_dims(cuda):
    net = device_net("fid")
    x, r32, r64 = whole_net_75("fid")
    outs = net(x.to(cuda), dims=cases.DIMS)
    for d, y in zip(cases.DIMS, outs):
        assert tuple(y.shape) == (2, d)
        judge("fid 75x75 dims=%d" % d, y, r32[d], r64[d])
    assert torch.equal(net(x.to(cuda), dims=768), outs[2]) and torch.equal(net(x.to(cuda)), outs[3])


def test_whole_network_on_75x75_torchvision_logits(cuda):
    net = device_net("torchvision")
    x, r32, r64 = whole_net_75("torchvision")
    y = net(x.to(cuda))
    assert tuple(y.shape) == (2, 1000)
    judge("torchvision 75x75 logits", y, r32, r64)


@pytest.mark.parametrize("variant", ["torchvision", "fid"])
def test_one_299_pass_through_the_resize(cuda, variant):
    from canonicalsg2im_amd import inception
    pic = cases.pictures(1, 64, seed=5)
    src = pic if variant == "fid" else (pic.float() / 255).permute(0, 3, 1, 2).contiguous()
    x_dev = inception.prepare(src.to(cuda) if variant == "fid" else to_dev(src, cuda), variant)
    assert tuple(x_dev.shape) == (1, 4, 299, 299)
    y = device_net(variant)(x_dev)
    r32 = host_net(variant, torch.float32)(cases.prepare(src, variant, dtype=torch.float32))
    r64 = host_net(variant, torch.float64)(cases.prepare(src, variant))
    if variant == "fid":
        r32, r64 = r32[2048], r64[2048]
    judge("%s 299x299 from 64x64" % variant, y, r32, r64)


# ------------------------------------------------------------------------------------------------ FID, Inception score
SIDE = (75, 75)            # the end-to-end tests resize to 75 x 75: the fp64 restatement of 24 pictures stays within seconds


def test_fid_end_to_end(cuda):
    """FID(A, B) of 2 x 12 seeded 64x64 uint8 pictures at dims 768 against the restatement pipeline (fp64 net -> numpy
    statistics -> the fixture-checked host formula).  Tolerance: the MEASURED feature error, propagated through
    d^2 = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 |A1 A2^T|_* with A_i = centred features / sqrt(N - 1) (tr sqrtm(S1 S2) is the
    nuclear norm of A1 A2^T, which is 1-Lipschitz in the nuclear norm, <= sqrt(rank) x Frobenius), plus the host
    formula's own 1e-7 on rank-deficient statistics."""
    from canonicalsg2im_amd import quality
    net = device_net("fid")
    sets = [cases.pictures(12, 64, seed=s) for s in (1, 2)]
    stats, stats64, d_mu, d_a, a_norm = [], [], [], [], []
    for pics in sets:
        fid = quality.FID(net, dims=768, size=SIDE)
        parts = [fid.features(pics[:5].to(cuda)), fid.features(pics[5:].to(cuda))]
        for f in parts:
            fid.update_features(f)
        assert fid.n == 12
        stats.append(fid.statistics())
        f64 = host_net("fid", torch.float64)(cases.prepare(pics, "fid", SIDE))[768].numpy()
        f_dev = torch.cat(parts).double().cpu().numpy()
        stats64.append((np.mean(f64, axis=0), np.cov(f64, rowvar=False)))
        d_mu.append(np.linalg.norm(f_dev.mean(0) - f64.mean(0)))
        d_a.append(np.linalg.norm((f_dev - f_dev.mean(0)) - (f64 - f64.mean(0))) / np.sqrt(11))
        a_norm.append(np.linalg.norm(f64 - f64.mean(0)) / np.sqrt(11))
        # the device statistics are np.mean / np.cov of the device's own features
        assert np.abs(stats[-1][1] - np.cov(f_dev, rowvar=False)).max() <= 1e-12 * np.abs(stats[-1][1]).max()
    (m1, s1), (m2, s2) = stats
    same = quality.frechet_distance(m1, s1, m1, s1)
    got = quality.frechet_distance(m1, s1, m2, s2)
    want = quality.frechet_distance(*stats64[0], *stats64[1])
    dm = np.linalg.norm(stats64[0][0] - stats64[1][0])
    tol = 2 * dm * (d_mu[0] + d_mu[1]) + (d_mu[0] + d_mu[1]) ** 2
    tol += sum(2 * a * d + d * d for a, d in zip(a_norm, d_a))
    tol += 2 * np.sqrt(12) * (d_a[0] * a_norm[1] + a_norm[0] * d_a[1] + d_a[0] * d_a[1])
    tol += 1e-7 * abs(want)
    print("FID(A,A) = %.3e (tr sigma %.3e); FID(A,B) = %.9g, restatement %.9g, |diff| %.2e, propagated tolerance %.2e"
          % (same, np.trace(s1), got, want, abs(got - want), tol))
    # identical statistics: tr S + tr S - 2 sum sqrt(lambda_i(S S)) leaves the eigenvalue route's rounding.  S S has rank 11
    # here; each of its D - 11 zero eigenvalues comes back as noise of at most eps |S|^2 and contributes up to sqrt(eps) |S|
    # to the sum, so |FID(A, A)| <= 2 D sqrt(eps) tr S (|S|_2 <= tr S) = 5.2e-5 here.  Measured on the device's statistics:
    # -1.3e-6 (D = 768, N = 12, tr S = 3.2).
    assert abs(same) <= 2 * 768 * np.sqrt(np.finfo(np.float64).eps) * np.trace(s1)
    assert want > 100 * tol, "the two sets are too alike for this check to mean anything"
    assert abs(got - want) <= tol


def test_inception_score_end_to_end(cuda):
    """The score of 12 pictures against the restatement pipeline.  Tolerance from the MEASURED logit error e (+ 2e-6 for the
    fp32 softmax): every log-probability moves by at most 2e, so KL_i moves by at most 4e + (exp(2e) - 1) x sum_j p |log(p /
    py)|, and the score exp(mean KL) by that factor."""
    from canonicalsg2im_amd import quality
    net = device_net("torchvision")
    pics = cases.pictures(12, 64, seed=3)
    imgs = (pics.float() / 255).permute(0, 3, 1, 2).contiguous() * 2 - 1          # a generator's output range
    score = quality.InceptionScore(net, size=SIDE)
    score.update(to_dev(imgs[:7], cuda))
    score.update(to_dev(imgs[7:], cuda))
    assert score.n == 12
    logits64 = host_net("torchvision", torch.float64)(cases.prepare(imgs, "torchvision", SIDE))
    p64 = F.softmax(logits64, dim=1).numpy()
    from canonicalsg2im_amd import inception
    logits_dev = torch.cat([net(inception.prepare(to_dev(part, cuda), "torchvision", SIDE))
                            for part in (imgs[:7], imgs[7:])]).double().cpu()          # the same two launches as update's
    e = float((logits_dev - logits64).abs().max()) + 2e-6
    for splits in (1, 5):
        mean, std = score.compute(splits)
        want_mean, want_std = cases.score_formula(p64, splits)
        per = 12 // splits
        worst = 0.0
        for k in range(splits):
            part = p64[k * per:(k + 1) * per]
            py = part.mean(0)
            worst = max(worst, float(np.abs(part * np.log(part / py)).sum(1).max()))
        dlog = 4 * e + np.expm1(2 * e) * worst
        tol = want_mean * np.expm1(dlog) * 1.0000001
        print("score splits=%d: %.9g +- %.3g, restatement %.9g +- %.3g, logit error %.2e, tolerance %.2e"
              % (splits, mean, std, want_mean, want_std, e, tol))
        assert abs(mean - want_mean) <= tol and abs(std - want_std) <= 2 * tol
    score.clean()
    assert score.n == 0


def test_check_model_gains_the_two_keys_only_when_asked(cuda):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.evaluate import Evaluator
    from canonicalsg2im_amd.synth import BatchConfig, make_batch, make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
                             "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "2",
                             "--use_img_disc", "1"])
    torch.manual_seed(0)
    tr = T.Trainer(opt, cuda)
    val = [[None if t is None else t.to(cuda) for t in make_batch(vocab, BatchConfig(2, 64, 2, 5, "packed"), seed=s)]
           for s in (11, 12, 13)]
    ev = Evaluator(tr)
    plain, _, _ = ev.check_model(val, use_gt=True)
    assert not any(k.startswith("inception") for k in plain)
    from canonicalsg2im_amd import inception
    net = inception.InceptionV3("torchvision", "random").to(cuda)
    scored, _, _ = ev.check_model(val, use_gt=True, inception=net)
    assert set(scored) - set(plain) == {"inception_mean", "inception_std", "inception_stand_in"}
    assert float(scored["inception_mean"]) >= 1.0 and float(scored["inception_std"]) >= 0.0
    assert tr.model.training


# ------------------------------------------------------------------------------------------------ scripts.quality
def test_quality_script(cuda, tmp_path, capsys):
    from PIL import Image
    from canonicalsg2im_amd.scripts import quality as script
    folders = []
    for k, n in ((0, 7), (1, 6)):
        d = tmp_path / ("set%d" % k)
        d.mkdir()
        for i, pic in enumerate(cases.pictures(n, 32, seed=20 + k).numpy()):
            Image.fromarray(pic).save(str(d / ("%03d.png" % i)))
        folders.append(str(d))
    out = tmp_path / "out"
    common = ["--fid_weights", "random", "--dims", "64", "--batch-size", "3", "--output_dir", str(out)]
    res = script.main(folders + common)
    text = capsys.readouterr().out
    assert "FID:" in text and "Warning: number of images is not a multiple of the batch size" in text
    assert "stand-in" in text and res["stand_in"] and res["images"] == [6, 6] and res["channel_order"] == "bgr"
    import json
    assert json.load(open(str(out / "quality.json")))["fid"] == res["fid"]
    # the .npz round trip: statistics saved by the first run give the same number
    res2 = script.main([str(out / "stats_A.npz"), folders[1]] + common)
    assert res2["fid"] == res["fid"]
    # the channel order changes the result
    res3 = script.main(folders + common + ["--channel_order", "rgb"])
    assert res3["fid"] != res["fid"]
    # with --inception_weights the Inception score of A is printed too
    res4 = script.main(folders + common + ["--inception_weights", "random", "--splits", "2"])
    assert "Inception score" in capsys.readouterr().out and res4["inception_score"]["mean"] >= 1.0
