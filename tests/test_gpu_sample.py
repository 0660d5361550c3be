"""The sampler on a real MI355X (canonicalsg2im_amd/sample.py): the uint8 deprocess against torch's fp32 host arithmetic
byte for byte, the inference forms of the SPADE launches against each other bit for bit, the eval statistics against
float64, the whole eval-mode generator against the float64 oracle, and the absence of side effects.

The deprocess restatement (`deprocess_host`) is the reference's sg2im/data/utils.py:36-65 written out.  T.Normalize(mean,
std) computes `tensor.sub_(mean).div_(std)` with mean and std as fp32 tensors, so imagenet_deprocess is, per channel c,
    t = (x - 0) / fp32(1 / IMAGENET_STD[c])            (:38)
    t = (t - fp32(-IMAGENET_MEAN[c])) / 1              (:39)
    t = (t - t.min()) / (t.max() - t.min())            (:31-33, rescale, over the whole image)
    u = byte(clamp(t * 255, 0, 255))                   (:62)
— i.e. (x - mean) / std is NOT what runs: the division by 1 / std comes first and is a division, not a multiplication.
"""
import os
import subprocess
import sys
from unittest import mock

import pytest
import torch

from conftest import ROOT, assert_close

pytestmark = pytest.mark.gpu

IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]
FULL = ["--image_size", "256,256", "--no_vgg_loss", "--use_img_disc", "0", "--batch_size", "4", "--gpu_ids", "0"]


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def deprocess_host(imgs, rescale):
    """deprocess_batch(imgs, rescale, imagenet_deprocess) of sg2im/data/utils.py:36-65 on fp32 CPU tensors."""
    std1 = torch.as_tensor([1.0 / s for s in IMAGENET_STD], dtype=torch.float32).view(3, 1, 1)      # INV_IMAGENET_STD
    mean2 = torch.as_tensor([-m for m in IMAGENET_MEAN], dtype=torch.float32).view(3, 1, 1)         # INV_IMAGENET_MEAN
    out = []
    for i in range(imgs.size(0)):
        t = imgs[i].cpu().clone()
        t = t.sub_(torch.zeros(3, 1, 1)).div_(std1)                 # T.Normalize(mean=[0, 0, 0], std=INV_IMAGENET_STD)
        t = t.sub_(mean2).div_(torch.ones(3, 1, 1))                 # T.Normalize(mean=INV_IMAGENET_MEAN, std=[1, 1, 1])
        if rescale:
            lo, hi = t.min(), t.max()
            t = t.sub(lo).div(hi - lo)
        out.append(t[None].mul(255).clamp(0, 255).byte())
    return torch.cat(out, dim=0)


# --------------------------------------------------------------------------------------------- 1. deprocess
@pytest.mark.timeout(600)
@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_deprocess_u8_equals_the_host_arithmetic_byte_for_byte(cuda, B, H, rescale):
    from canonicalsg2im_amd import ops
    g = torch.Generator().manual_seed(100 * B + H + int(rescale))
    x = torch.randn((B, 3, H, H), generator=g) * 1.5                 # tanh images stay in [-1, 1]; these go beyond +-3
    x[0, :, :4, :4] = torch.tensor([-7.5, 0.0, 6.25]).view(3, 1, 1)
    assert float(x.abs().max()) > 3.0
    want = deprocess_host(x, rescale)
    assert torch.equal(want, deprocess_host(x, rescale)), "the host restatement itself is not deterministic"
    padded = torch.zeros((B, H, H, 4))                                # conv_img's output: 3 channels in 4-float pixels
    padded[..., :3] = x.permute(0, 2, 3, 1)
    padded[..., 3] = 99.0                                             # the pad must not enter the min / max
    forms = {"4-padded": padded.to(cuda).permute(0, 3, 1, 2)[:, :3],
             "channels-last": x.to(cuda).contiguous(memory_format=torch.channels_last)}
    for name, img in forms.items():
        got = ops.deprocess_u8(img, rescale)
        again = ops.deprocess_u8(img, rescale)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 3, H, H) and got.is_contiguous()
        differing = int((got.cpu() != want).sum())
        print("deprocess_u8 B=%d H=%d rescale=%s %s: %d differing bytes of %d" % (B, H, rescale, name, differing, want.numel()))
        assert differing == 0, "%s: %d bytes differ from the fp32 host arithmetic" % (name, differing)
        assert torch.equal(got, again), name + ": a second run differs"


@pytest.mark.timeout(300)
def test_deprocess_u8_of_a_constant_image_is_what_torch_gives_on_the_host(cuda):
    """hi == lo: (t - lo) / (hi - lo) is 0 / 0 = NaN for every element, and byte() of a NaN is undefined in C++.  The
    kernel writes what torch's host kernels produce here — this test asks torch rather than stating a value — and an
    image holding a NaN (min and max propagate it) goes the same way.  Other images of the batch are not affected."""
    from canonicalsg2im_amd import ops
    x = torch.randn((3, 3, 64, 64), generator=torch.Generator().manual_seed(5))
    # image 1: constant AFTER the two Normalize steps — per channel the x whose t is exactly T, for the first T where all
    # three channels round to it
    std1 = torch.as_tensor([1.0 / s for s in IMAGENET_STD], dtype=torch.float32)
    mean2 = torch.as_tensor([-m for m in IMAGENET_MEAN], dtype=torch.float32)
    for T in torch.linspace(0.25, 0.75, 4097):
        xc = (T + mean2) * std1
        if bool(((xc / std1 - mean2) == T).all()):
            break
    else:
        raise AssertionError("no constant image found")
    x[1] = xc.view(3, 1, 1)
    x[2, 1, 7, 9] = float("nan")
    want = deprocess_host(x, True)
    got = ops.deprocess_u8(x.to(cuda).contiguous(memory_format=torch.channels_last), True).cpu()
    assert torch.equal(got, want), int((got != want).sum())
    assert len(want[1].unique()) == 1 and len(want[2].unique()) == 1 and len(want[0].unique()) > 100


# --------------------------------------------------------------------------------------------- 2. gamma_out = NULL
@pytest.mark.timeout(600)
@pytest.mark.parametrize("B", [4, 16])
@pytest.mark.parametrize("C,HW", [(256, 64), (64, 128)])
def test_spade_infer_is_bit_identical_to_the_forms_that_write_gamma(cuda, C, HW, B):
    """128 -> C at HW x HW (both F(4x4,3x3) maps): spade_infer's y on a NaN-prefilled output equals, bit for bit and given
    the same (mean, invstd), (a) the joint launch WITH a gamma buffer, (b) the gamma / beta launch pair, (c) the plain
    gamma || beta convolution followed by csg_norm_apply_fwd.
    Batch 4: these launches have ONE (region, gamma + beta block) item per CU, and the joint launch exists from two per CU
    up (csg_wino4_conv_spade_supported says no, the library refuses the call): spade_infer runs the pair there, and (a) is
    that refusal.  Batch 16 has four items per CU: there spade_infer IS the joint launch with gamma_out = NULL."""
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    nh, slope = 128, 0.2
    g = torch.Generator().manual_seed(C + HW)
    r = lambda *s: torch.randn(*s, generator=g)
    x = ops.nhwc((r(B, C, HW, HW) * 1.3 + 0.2).to(cuda))
    actv = ops.nhwc(r(B, nh, HW, HW).relu().to(cuda))
    w = (r(2 * C, nh, 3, 3) * 0.03).to(cuda).contiguous(memory_format=torch.channels_last)
    b = (r(2 * C) * 0.1).to(cuda)
    rm, rv = (r(C) * 0.3).to(cuda), (torch.rand(C, generator=g) + 0.5).to(cuda)
    (mean, invstd), = ops.norm_eval_stats([(rm, rv)], 1e-5)
    nan = lambda: torch.full_like(x, float("nan"))
    d = ops._wino_desc(B, HW, HW, nh, C)
    d.y_cs = C
    joint = B >= 16
    assert lib.csg_wino4_conv_spade_supported(d) == int(joint) and ops.wino_variant(B, HW, HW, nh, 2 * C) == 4
    up = ops.wino_pack(w, False, None, 4)

    y = nan()
    out, = ops.spade_infer(x, [(actv, w, b, rm, rv, slope, None)], 1e-5, outs=[y])
    assert out is y
    # (a) the same launch, gamma written
    ya, ga = nan(), nan()
    rc = lib.csg_wino4_conv_spade(d, ptr(actv), ptr(up), ptr(b), ptr(x), ptr(ga), C, ptr(mean), ptr(invstd), slope, ptr(ya),
                                  stream())
    assert rc == (0 if joint else -2), rc                 # CSG_E_UNSUPPORTED: nothing was launched
    # (b) the launch pair
    yb, gb = nan(), nan()
    check(lib.csg_wino4_conv_part(d, ptr(actv), ptr(up), 0, 2 * C // 32, ptr(b), None, None, 0, None, None, 1.0, ptr(gb),
                                  stream()), "gamma")
    check(lib.csg_wino4_conv_part(d, ptr(actv), ptr(up), C // 32, 2 * C // 32, ptr(b[C:]), ptr(x), ptr(gb), C, ptr(mean),
                                  ptr(invstd), slope, ptr(yb), stream()), "beta")
    # (c) plain convolution, then the apply pass
    yc = nan()
    with torch.no_grad():
        gbmap = ops.nhwc(ops.conv2d(actv, w, b, 1, 1))
    check(lib.csg_norm_apply_fwd(ptr(x), ptr(mean), ptr(invstd), ptr(gbmap), slope, 1, B * HW * HW, C, ptr(yc), None, 1.0, None,
                                 stream()), "apply")
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
    for name, other in (("joint launch with gamma", ya), ("launch pair", yb), ("convolution + apply pass", yc))[0 if joint else 1:]:
        n = int((y != other).sum())
        print("C=%d %dx%d  spade_infer vs %s: %d differing elements, max |diff| %.3e" % (
            C, HW, HW, name, n, float((y - other).abs().max())))
    if joint:
        assert torch.equal(y, ya), "joint launch with a gamma buffer"
        assert torch.equal(ga, gb)
    else:
        assert torch.isnan(ya).all() and torch.isnan(ga).all()
    assert torch.equal(y, yb), "launch pair"
    assert torch.equal(y, yc), "plain convolution + csg_norm_apply_fwd"
    assert torch.equal(gb, gbmap[:, :C])
    # and the whole thing is the eval-mode modulation (fp64 on the host, the convolution's tolerance)
    gb64 = torch.nn.functional.conv2d(actv.double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)
    xh = (x.double().cpu() - rm.double().cpu().view(1, C, 1, 1)) / torch.sqrt(rv.double().cpu().view(1, C, 1, 1) + 1e-5)
    ref = torch.nn.functional.leaky_relu(xh * (1 + gb64[:, :C]) + gb64[:, C:], slope)
    assert_close(y, ref, 1e-4, 1e-4 * float(ref.abs().max()), "spade_infer vs fp64")


# --------------------------------------------------------------------------------------------- 3. eval statistics
@pytest.mark.timeout(300)
def test_norm_eval_stats_multi_is_within_two_ulp_of_float64(cuda):
    from canonicalsg2im_amd import ops
    g = torch.Generator().manual_seed(9)
    pairs = []
    for C in (32, 1024, 1040, 64, 512):
        rv = torch.rand(C, generator=g) * 4 + 1e-3
        rv[::7] = torch.rand(len(rv[::7]), generator=g) * 1e-6          # variances far below eps as well
        pairs.append(((torch.randn(C, generator=g) * 3).to(cuda), rv.to(cuda)))
    eps = 1e-5
    out = ops.norm_eval_stats(pairs, eps)
    torch.cuda.synchronize()
    assert len(out) == len(pairs)
    worst = 0.0
    for (rm, rv), (mean, invstd) in zip(pairs, out):
        assert mean.data_ptr() % 16 == 0 and invstd.data_ptr() % 16 == 0
        assert torch.equal(mean, rm)
        # fp32 var + fp32 eps is what F.batch_norm adds; the float64 reference takes that sum as given
        ref = 1.0 / torch.sqrt((rv + torch.tensor(eps, dtype=torch.float32, device=cuda)).double().cpu())
        ref32 = ref.float()
        ulp = (torch.nextafter(ref32, torch.full_like(ref32, float("inf"))) - ref32).double()
        err = ((invstd.double().cpu() - ref).abs() / ulp).max()
        worst = max(worst, float(err))
    print("norm_eval_stats: worst error %.3f ulp" % worst)
    assert worst <= 2.0, worst


# --------------------------------------------------------------------------------------------- 4. whole generator
def _oracle_eval_image64(ts, batch, boxes_from, masks_from, mask_noise=None):
    """MetaGeneratorModel.forward(test_mode=True) (sg2im/meta_models.py:25-51) of the oracle in float64, eval mode: running
    statistics, no power iteration, painter's compositing when masks reach the generator."""
    import oracle.functional as OF
    from oracle.fp64 import batch_to64, state_to64
    sg, g = state_to64(ts.sg), state_to64(ts.g)
    b64 = batch_to64(batch)
    objs, boxes, triplets, tt, masks = b64[1], b64[2], b64[3], b64[5], b64[6]
    vocab = ts.opt.vocab
    with torch.no_grad():
        # (without the mask net's entries the helper skips its training-mode mask branch)
        obj_vecs, boxes_pred, _ = OF.sg2layout_forward({k: v for k, v in sg.items() if not k.startswith("mask_net.")}, vocab,
                                                       objs, triplets, tt)
        use_boxes = boxes if boxes_from == "gt" else boxes_pred
        use_masks = None
        if masks_from == "gt":
            use_masks = masks
        elif masks_from == "pred":
            B, O = objs.shape[0], objs.shape[1]
            noise = mask_noise.double().repeat((B, O, 1)).view(B, O, -1)
            scores = OF.mask_net(sg, "mask_net.", torch.cat([obj_vecs, noise], dim=-1), training=False)
            use_masks = scores.view(B, O, scores.shape[2], scores.shape[3]).sigmoid()
        painter = lambda vecs, bx, mk, H, W=None, test_mode=False: _ORIG_M2L(vecs, bx, mk, H, W, test_mode=True)
        with mock.patch.object(OF, "masks_to_layout", painter):
            img = OF.generator_forward(g, vocab, ts.opt.image_size[0], objs, use_boxes, training=False,
                                       num_upsampling_layers=ts.opt.num_upsampling_layers, layout_masks=use_masks)
    return img, boxes_pred


def _orig_m2l():
    import oracle.functional as OF
    return OF.masks_to_layout


_ORIG_M2L = None


def _trained(cuda, argv, cfg, seed):
    """A trainer after ONE step (running statistics and u / v off their initial values), its checkpoint, a fresh batch."""
    global _ORIG_M2L
    import oracle
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_batch, make_vocab
    _ORIG_M2L = _ORIG_M2L or _orig_m2l()
    vocab = make_vocab("coco")
    opt = T.make_opt(vocab, argv)
    torch.manual_seed(seed)
    tr = T.Trainer(opt, cuda)
    if tr.model.has_graph and getattr(tr.model.sg_to_layout.module, "mask_net", None) is not None:
        tr.model.sg_to_layout.module.mask_noise = torch.randn((1, opt.mask_noise_dim), generator=torch.Generator().manual_seed(1))
    tr.step([None if t is None else t.to(cuda) for t in make_batch(vocab, cfg, seed=seed + 1)])
    torch.cuda.synchronize()
    ckpt = {"model_state": {k: v.detach().clone() for k, v in tr.checkpoint_dict()["model_state"].items()}}
    ts = T.oracle_state_from(tr, oracle)
    noise = tr.model.sg_to_layout.module.mask_noise
    del tr
    torch.cuda.empty_cache()
    return opt, vocab, ckpt, ts, make_batch(vocab, cfg, seed=seed + 2), noise


def _image_rule(img, ref64, tag):
    """The project's image rule: rtol 1e-4 + 1e-4 absolute, and <= 2e-5 in relative L2."""
    d = img.detach().double().cpu() - ref64
    rel_l2 = float(d.norm() / ref64.norm())
    print("%s: max |diff| %.3e, relative L2 %.3e (mean |pixel| %.3f)" % (tag, float(d.abs().max()), rel_l2,
                                                                          float(ref64.abs().mean())))
    assert_close(img, ref64, 1e-4, 1e-4, tag)
    assert rel_l2 <= 2e-5, "%s: relative L2 distance %.3e > 2e-5" % (tag, rel_l2)


def _sd_equal(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), "state_dict entry %s changed" % k


@pytest.mark.timeout(2400)
def test_generator_at_full_width_matches_the_float64_oracle_and_replays_bit_identically(cuda, tmp_path):
    """ngf 64, 256 x 256, batch 4, COCO-shaped batch, after one training step: Sampler.generate(uint8=False) against the
    oracle's float64 eval-mode forward of the same weights — with the ground-truth boxes and with the predicted ones —
    through the eager walk (first call), the capturing call and a pure replay, which must all be the same bits; the same
    call in a fresh process with CSG_GRAPHS=0 gives those bits too; no entry of the model's state_dict changes."""
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.synth import BatchConfig
    opt, vocab, ckpt, ts, batch, _ = _trained(cuda, FULL, BatchConfig(4, 256, 1, 30, "random"), seed=0)
    s = Sampler(opt, cuda, ckpt)
    dev = [None if t is None else t.to(cuda) for t in batch]
    objs, boxes, triplets, tt = dev[1], dev[2], dev[3], dev[5]
    before = {k: v.detach().clone() for k, v in s.model.state_dict().items()}
    assert torch.is_grad_enabled()
    images = {}
    for boxes_from in ("gt", "pred"):
        kw = {"boxes_gt": boxes} if boxes_from == "gt" else {}
        runs = [s.generate(objs, triplets, tt, uint8=False, **kw) for _ in range(3)]
        torch.cuda.synchronize()
        assert torch.is_grad_enabled()
        ref64, boxes64 = _oracle_eval_image64(ts, batch, boxes_from, None)
        img = runs[0][0]
        assert tuple(img.shape) == (4, 3, 256, 256) and img.dtype == torch.float32 and img.stride(1) == 1
        _image_rule(img, ref64, "generate(boxes %s)" % boxes_from)
        assert_close(runs[0][1], boxes64, 1e-4, 1e-5, "boxes_pred")
        assert runs[0][2] is None
        assert torch.equal(runs[1][0], img), "the second call differs from the first"
        assert torch.equal(runs[2][0], img), "the third call (a replay) differs from the first"
        images[boxes_from] = img.cpu()
    # one key serves both cases: the very first call walked eagerly, the second captured, every later one replayed
    assert s.replays == 5 and s.eager_calls == 1, (s.replays, s.eager_calls)
    _sd_equal(before, {k: v for k, v in s.model.state_dict().items()})
    # uint8: the same image through the device deprocess, byte for byte what the host makes of the fp32 image
    u8 = s.generate(objs, triplets, tt, boxes_gt=boxes)[0]
    assert u8.dtype == torch.uint8 and torch.equal(u8.cpu(), deprocess_host(images["gt"], True))
    # a fresh process without replay
    torch.save({"ckpt": ckpt, "argv": FULL, "batch": batch}, tmp_path / "job.pt")
    for graphs in ("0", "1"):
        out = tmp_path / ("img_%s.pt" % graphs)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path / "job.pt"), str(out)], cwd=ROOT,
                           env=dict(os.environ, CSG_GRAPHS=graphs, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        got = torch.load(out)
        assert got["replays"] == (0 if graphs == "0" else 2), got["replays"]
        assert torch.equal(got["img"], images["gt"]), "fresh process with CSG_GRAPHS=%s differs" % graphs


@pytest.mark.timeout(1800)
def test_generator_with_masks_paints_the_layout_and_matches_the_float64_oracle(cuda):
    """ngf 64 at 64 x 64 with --mask_size 16: the ground-truth masks reach the generator through painter's compositing
    (ops.layout_paint); eager walk, capture and replay agree bit for bit and with the float64 oracle."""
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.synth import BatchConfig
    argv = ["--image_size", "64,64", "--no_vgg_loss", "--use_img_disc", "0", "--batch_size", "4", "--gpu_ids", "0",
            "--mask_size", "16"]
    opt, vocab, ckpt, ts, batch, noise = _trained(cuda, argv, BatchConfig(4, 64, 3, 8, "random", mask_size=16), seed=3)
    s = Sampler(opt, cuda, ckpt)
    s.model.sg_to_layout.module.mask_noise = noise
    dev = [None if t is None else t.to(cuda) for t in batch]
    before = {k: v.detach().clone() for k, v in s.model.state_dict().items()}
    runs = [s.generate(dev[1], dev[3], dev[5], boxes_gt=dev[2], masks_gt=dev[6], uint8=False) for _ in range(3)]
    torch.cuda.synchronize()
    ref64, _ = _oracle_eval_image64(ts, batch, "gt", "gt")
    _image_rule(runs[0][0], ref64, "generate(masks, painter)")
    assert torch.equal(runs[1][0], runs[0][0]) and torch.equal(runs[2][0], runs[0][0])
    assert s.replays == 2 and s.eager_calls == 1
    # the predicted masks come back in eval mode (running statistics of the mask net)
    import oracle.functional as OF
    from oracle.fp64 import batch_to64, state_to64
    sg = state_to64(ts.sg)
    b64 = batch_to64(batch)
    with torch.no_grad():
        vecs = OF.sg2layout_forward({k: v for k, v in sg.items() if not k.startswith("mask_net.")}, vocab, b64[1], b64[3], b64[5])[0]
        B, O = b64[1].shape[:2]
        scores = OF.mask_net(sg, "mask_net.", torch.cat([vecs, noise.double().repeat((B, O, 1)).view(B, O, -1)], dim=-1),
                             training=False)
    assert_close(runs[0][2], scores.view(B, O, 16, 16).sigmoid(), 1e-4, 1e-5, "masks_pred")
    _sd_equal(before, {k: v for k, v in s.model.state_dict().items()})


# --------------------------------------------------------------------------------------------- 5. no side effects
_SIDE = ["--image_size", "64,64", "--ngf", "32", "--ndf", "16", "--no_vgg_loss", "--use_img_disc", "1", "--batch_size", "4",
         "--gpu_ids", "0"]


def _side_effect_child(out, with_sampler):
    """Three trainer steps (eager, capturing, replayed) — after three sampler calls in the same process, or without."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.synth import BatchConfig, make_batch, make_vocab
    cuda = torch.device("cuda:0")
    vocab = make_vocab("coco")
    opt = T.make_opt(vocab, _SIDE)
    cfg = BatchConfig(4, 64, 3, 8, "random")
    torch.manual_seed(0)
    tr = T.Trainer(opt, cuda)
    if with_sampler:
        rng = torch.random.get_rng_state()
        s = Sampler(opt, cuda, tr.checkpoint_dict())
        torch.random.set_rng_state(rng)
        b = [None if t is None else t.to(cuda) for t in make_batch(vocab, cfg, seed=50)]
        for _ in range(3):
            s.generate(b[1], b[3], b[5], boxes_gt=b[2])
        assert s.replays == 2
    rows = []
    for it in range(3):
        G, D = tr.step([None if t is None else t.to(cuda) for t in make_batch(vocab, cfg, seed=60 + it)])
        rows.append(({k: v.cpu() for k, v in G.items()}, {k: v.cpu() for k, v in D.items()}))
    torch.cuda.synchronize()
    torch.save({"rows": rows, "replays": tr.graphs.replays if tr.graphs is not None else -1}, out)


@pytest.mark.timeout(1200)
def test_a_trainer_step_after_sampling_matches_a_fresh_process_bit_for_bit(cuda, tmp_path):
    outs = {}
    for tag in ("plain", "sampled"):
        out = tmp_path / (tag + ".pt")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side-effects", tag, str(out)], cwd=ROOT,
                           env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=500)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[tag] = torch.load(out)
    assert outs["plain"]["replays"] == outs["sampled"]["replays"] == 2
    for it, ((Ga, Da), (Gb, Db)) in enumerate(zip(outs["plain"]["rows"], outs["sampled"]["rows"])):
        for a, b in ((Ga, Gb), (Da, Db)):
            assert set(a) == set(b)
            for k in a:
                assert torch.equal(a[k], b[k]), "step %d, %s: %r vs %r" % (it, k, a[k], b[k])


# --------------------------------------------------------------------------------------------- 6. additivity
@pytest.mark.timeout(300)
def test_spade_forward_in_eval_mode_still_takes_its_three_passes(cuda):
    """SPADE.forward in eval mode on a 32-wide map, nothing set: the launches are those of the three-pass path it has
    always taken (mlp_shared, the materialised gamma || beta map, norm_act(training=False)) — not the inference forms."""
    from canonicalsg2im_amd import _lib, ops
    from canonicalsg2im_amd.spade.models.networks.normalization import SPADE
    torch.manual_seed(4)
    sp = SPADE("spadesyncbatch3x3", 64, 32).to(cuda).eval()
    with torch.no_grad():
        sp.param_free_norm.running_mean.normal_()
        sp.param_free_norm.running_var.uniform_(0.5, 2.0)
    x, seg = ops.nhwc(torch.randn(4, 64, 32, 32, device=cuda)), ops.nhwc(torch.randn(4, 32, 32, 32, device=cuda))
    assert not sp.fusable(x) and not sp.joinable(x)

    def launches(fn):
        with torch.no_grad():
            fn()                                       # (weight layouts and packs of a first call)
            torch.cuda.synchronize()
            _lib.prof_enable(1)
            _lib.prof_reset()
            try:
                y = fn()
                torch.cuda.synchronize()
                table = {k: v[1] for k, v in _lib.prof_read().items()}
            finally:
                _lib.prof_enable(0)
                _lib.prof_reset()
        return y, table

    def three_passes():
        sh, pn = sp.mlp_shared[0], sp.param_free_norm
        actv = ops.conv2d(seg, sh.weight, sh.bias, 1, 1, sh.act, sh.slope)
        gb = ops.conv2d(actv, torch.cat([sp.mlp_gamma.weight, sp.mlp_beta.weight]), torch.cat([sp.mlp_gamma.bias, sp.mlp_beta.bias]),
                        1, 1)
        return ops.norm_act(x, gb, pn.running_mean, pn.running_var, training=False, slope=0.2, eps=pn.eps)

    y, table = launches(lambda: sp(x, seg, fused_slope=0.2))
    y3, table3 = launches(three_passes)
    print("SPADE.forward (eval) launches:", table)
    assert table == table3, (table, table3)
    assert table.get("norm_apply_fwd") == 1 and "norm_eval_stats" not in table and "deprocess_u8" not in table
    assert {k: v for k, v in table.items() if k != "wino_pack"} == {"wino4_conv": 1, "wino_conv": 1, "norm_apply_fwd": 1} \
        or sum(v for k, v in table.items() if k != "wino_pack") == 3, table
    assert torch.equal(y, y3)


def _replay_child(job, out):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.synth import make_vocab
    cuda = torch.device("cuda:0")
    job = torch.load(job)
    opt = T.make_opt(make_vocab("coco"), job["argv"])
    s = Sampler(opt, cuda, job["ckpt"])
    b = [None if t is None else t.to(cuda) for t in job["batch"]]
    for _ in range(3):
        img = s.generate(b[1], b[3], b[5], boxes_gt=b[2], uint8=False)[0]
    torch.cuda.synchronize()
    torch.save({"img": img.cpu(), "replays": s.replays}, out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--side-effects":
        _side_effect_child(sys.argv[3], sys.argv[2] == "sampled")
    else:
        _replay_child(sys.argv[1], sys.argv[2])
