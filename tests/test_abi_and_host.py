"""CPU-side checks (no GPU, no compute calls): the C-ABI library loads and exports every symbol
declared in include/csg_hip.h, the host logic (descriptors, flags, synthetic batches, state_dict
surface) behaves like the reference, and nothing in the product imports the oracle."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from canonicalsg2im_amd import _lib
    return _lib


def test_library_exports_every_declared_symbol(built):
    hdr = open(os.path.join(ROOT, "include", "csg_hip.h")).read()
    declared = set(re.findall(r"\b(csg_[a-z0-9_]+)\s*\(", hdr))
    declared.discard("csg_conv_desc")
    assert len(declared) >= 30
    assert declared == set(built.SIGNATURES.keys()), declared ^ set(built.SIGNATURES.keys())
    for name in declared:
        assert getattr(built.lib, name) is not None
    assert built.lib.csg_version() >= 100
    assert built.lib.csg_prof_num_kernels() > 10


def test_shipped_kernels_keep_their_state_in_registers(built):
    """The compiler's own resource report of the build (`__graft_entry__.kernel_resources`: -Rpass-analysis=kernel-resource-usage
    remarks kept beside each object): every kernel the library ships holds its state in registers.  Scratch in one of
    the MFMA loops does not fail a parity test — it turns a 0.4 ms launch into a 12 ms one (round 6 did exactly that to
    k_wino4_conv_v<*, false> with a lambda the compiler stopped inlining; rounds 3 and 5 met it twice in DESIGN's notes)."""
    import __graft_entry__ as ge
    res = ge.kernel_resources()
    assert len(res) >= 100, len(res)
    allowed = {
        # conv_img's forward (64 -> 3, 0.13 ms per launch): nine dwords per lane, known and bounded
        "k_few_fwdILi3ELi3ELi3E": 36, "k_few_fwdILi3ELi3ELi4E": 36,
    }
    bad = {}
    for name, r in res.items():
        limit = max([v for k, v in allowed.items() if k in name] + [0])
        if r.get("scratch", 0) > limit:
            bad[name] = (r["scratch"], limit, r["source"])
    assert not bad, bad
    # the three MFMA loops sit where DESIGN.md says they do: three waves per SIMD for the F(4x4,3x3) convolution (<= 170
    # registers), two for the weight gradient and the direct / F(2x2,3x3) kernels
    w4 = [r for n, r in res.items() if "k_wino4_conv_v" in n]
    assert len(w4) == 3 and all(r["vgprs"] <= 170 and r["occupancy"] >= 3 for r in w4), w4
    ww = [r for n, r in res.items() if "k_wino4_wgrad" in n]
    assert len(ww) == 1 and all(r["vgprs"] <= 256 and r["occupancy"] >= 2 for r in ww), ww


def test_library_reads_only_the_family_switches_from_the_environment():
    """Kernel choices are made by ops.plan_conv; the library itself reads no tuning knob, only the switches that turn a
    kernel family off (A/B runs and the bit-identity test of the persistent F(4x4,3x3) form)."""
    csrc = os.path.join(ROOT, "canonicalsg2im_amd", "csrc")
    names = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            names |= set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', open(os.path.join(csrc, f)).read()))
    assert names == {"CSG_WINO4", "CSG_WINO34", "CSG_WINO4_PERSIST"}, names
    # the settled A/B switches are gone from the package, Python and HIP alike (their results: profiles/README.md)
    retired = re.compile("CSG_SN_BATCHED|CSG_POOL_FANOUT|CSG_HINGE_FUSED|CSG_PREPACK")
    for dirpath, _, files in os.walk(os.path.join(ROOT, "canonicalsg2im_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                assert not retired.search(open(os.path.join(dirpath, f), errors="replace").read()), os.path.join(dirpath, f)


def _call_args(text, start):
    """The top-level arguments of the call whose opening parenthesis is at text[start]."""
    args, depth, cur = [], 0, ""
    for ch in text[start:]:
        if ch == "(":
            depth += 1
            if depth == 1:
                continue
        elif ch == ")":
            depth -= 1
            if depth == 0:
                return args + [cur.strip()]
        if ch == "," and depth == 1:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    raise AssertionError("unbalanced call")


def test_dynamic_lds_limits_are_raised_in_one_place():
    """Above 48 KB of dynamic LDS a kernel's limit has to be raised before the launch: csg::lds_limit (csg_common.h) is the
    one place that does it, per kernel and device, checked.  A file that launches with dynamic LDS and never calls it
    says so here, with the arithmetic beside its launches — a new kernel file has to decide on purpose."""
    csrc = os.path.join(ROOT, "canonicalsg2im_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    assert len(text) >= 30
    assert [f for f, t in text.items() if "hipFuncSetAttribute" in t] == ["csg_common.h"]
    assert [f for f, t in text.items() if "attr_set" in t] == []
    never_above_48k = {"gemm.hip",       # 32 KB, and exactly 48 KB for the 64-wide tile
                       "norm.hip"}       # 16 KB
    launches = 0
    for f, t in text.items():
        # a macro that hands its arguments on to CSG_LAUNCH (FEW_DISPATCH) is a launch too: same argument positions
        macros = ["CSG_LAUNCH"] + re.findall(r"#define (\w+)\(KERNEL, \.\.\.\)", t)
        dynamic = []
        for m in re.finditer(r"\b(%s)\(" % "|".join(macros), t):
            if t[:m.start()].endswith("#define "):
                continue
            args = _call_args(t, m.end() - 1)
            if "__VA_ARGS__" in args:
                continue                                       # inside such a macro's body: its uses are checked
            assert len(args) >= 6, (f, args)
            launches += 1
            if args[3] != "0":
                dynamic.append(args[3])
        if dynamic and "lds_limit<" not in t:
            assert f in never_above_48k, (f, dynamic)
        else:
            assert f not in never_above_48k, f
    assert launches >= 100, launches


def test_conv_descriptor_struct_matches_header(built):
    import ctypes
    hdr = open(os.path.join(ROOT, "include", "csg_hip.h")).read()
    body = hdr[hdr.index("typedef struct csg_conv_desc {"):hdr.index("} csg_conv_desc;")]
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)(?:\[CSG_MAX_TAPS\])?\s*[,;]", body.split("{", 1)[1])
    assert names == [f[0] for f in built.ConvDesc._fields_]
    assert ctypes.sizeof(built.ConvDesc) == 4 * (20 + 3 * 16 + 4)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "canonicalsg2im_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import oracle|from oracle)", src, re.M), os.path.join(dirpath, f)


def test_ops_refuse_cpu_tensors(built):
    from canonicalsg2im_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.conv2d(torch.randn(1, 4, 4, 4), torch.randn(4, 4, 3, 3), None, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.real_object_mask(torch.zeros(1, 2, 1, dtype=torch.int64), 0)


def test_backward_data_descriptors_cover_every_input_pixel_once(built):
    """Parity classes of the stride-2 transposed convolution: each input pixel belongs to exactly one
    launch and each (ky,kx) tap is used by exactly one parity class."""
    from canonicalsg2im_amd.ops import _desc_forward, _descs_backward_data
    for (IH, K, s, p) in ((9, 4, 2, 2), (8, 4, 2, 2), (7, 3, 1, 1), (6, 4, 1, 2), (5, 1, 1, 0)):
        d, OH, OW = _desc_forward(2, IH, IH, 8, 12, K, K, s, p)
        assert OH == (IH + 2 * p - K) // s + 1
        descs = _descs_backward_data(2, IH, IH, 8, 12, K, K, s, p, OH, OW)
        seen = torch.zeros(IH, IH, dtype=torch.int32)
        taps = []
        for bd in descs:
            for gy in range(bd.OHg):
                for gx in range(bd.OWg):
                    seen[gy * bd.os + bd.ooy, gx * bd.os + bd.oox] += 1
            for t in range(bd.ntaps):
                taps.append(bd.tap_w[t])
                ky = bd.tap_w[t] // K
                # dY row of grid row j is j + tap_dy: must satisfy iy = s*oy - p + ky
                assert s * (0 + bd.tap_dy[t]) - p + ky == bd.ooy
        assert int(seen.min()) == 1 and int(seen.max()) == 1
        assert sorted(taps) == list(range(K * K))


def test_flags_match_reference_defaults():
    from canonicalsg2im_amd.scripts.args import make_opt
    from canonicalsg2im_amd.synth import make_vocab
    opt = make_opt(make_vocab("clevr"), ["--no_vgg_loss"])
    assert opt.image_size == (256, 256) and opt.embedding_dim == 32 and opt.gconv_dim == 128
    assert opt.gconv_hidden_dim == 512 and opt.gconv_num_layers == 5 and opt.ngf == 64 and opt.ndf == 64
    assert opt.norm_G == 'spectralspadesyncbatch3x3' and opt.norm_D == 'spectralinstance'
    assert opt.num_D == 2 and opt.n_layers_D == 4 and opt.beta1 == 0.5 and opt.learning_rate == 1e-4
    assert opt.semantic_nc == 4 * 32 and opt.gpu_ids == [0]
    with pytest.raises(AssertionError):
        make_opt(make_vocab("coco"), ["--batch_size", "3", "--gpu_ids", "0,1"])


def test_synthetic_batch_follows_collate_contract():
    from canonicalsg2im_amd.synth import BASELINE_CONFIGS, BatchConfig, make_batch, make_vocab, shard_batch
    vocab = make_vocab("coco")
    b = make_batch(vocab, BatchConfig(4, 64, 3, 8, "packed"), seed=1)
    imgs, objs, boxes, triplets, conv, tt, masks, ids = b
    assert imgs.shape == (4, 3, 64, 64) and imgs.dtype == torch.float32
    assert objs.dtype == torch.int64 and objs.shape[2] == 1 and boxes.shape[:2] == objs.shape[:2]
    assert triplets.dtype == torch.int64 and triplets.shape[2] == 3 and tt.shape == triplets.shape[:2]
    pad = objs[..., 0] == 0
    assert torch.all(boxes[pad] == -1) and torch.all(boxes[~pad] >= 0)
    padt = triplets[..., 1] == 0
    assert torch.all(triplets[padt] == 0)
    n_obj = (~pad).sum(1)
    assert torch.all(triplets[..., 0].max(1).values < n_obj) and torch.all(triplets[..., 2].max(1).values < n_obj)
    b2 = make_batch(vocab, BatchConfig(4, 64, 3, 8, "packed"), seed=1)
    assert all(torch.equal(x, y) for x, y in zip(b[:6], b2[:6]))
    s0, s1 = shard_batch(b, 0, 2), shard_batch(b, 1, 2)
    assert torch.equal(torch.cat([s0[1], s1[1]]), objs)
    with pytest.raises(ValueError):
        shard_batch(b, 0, 3)
    clevr = make_batch(make_vocab("clevr"), BatchConfig(2, 64, 4, 6, "closure"), seed=2)
    assert clevr[1].shape[2] == 4 and set(clevr[5].unique().tolist()) <= {0, 1}
    assert set(BASELINE_CONFIGS) == {"C1", "C2", "C3", "C4", "C5"}


def test_module_surface_and_state_dict_keys(built):
    """Constructors, attribute names and checkpoint keys of the drop-in modules."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sg2im.model import get_conv_converse
    from canonicalsg2im_amd.synth import make_vocab
    from conftest import load_golden
    meta, a = load_golden("train_step")
    opt = T.make_opt(make_vocab(meta["vocab"]), meta["argv"])
    tr = T.Trainer(opt, torch.device("cpu"))
    sg, g, d = T.split_state(tr)
    for mine, want in ((sg, meta["shapes"]["sg"]), (g, meta["shapes"]["g"]), (d, meta["shapes"]["d"])):
        keys = {k for k in mine if not any(u in k for u in ("repr_net", "image_encoder"))}
        assert keys == set(want), keys ^ set(want)
        for k in want:
            assert list(mine[k].shape) == want[k][0], k
    full = tr.model.state_dict()
    assert "sg_to_layout.module.trans_candidates_weights" in full
    assert "layout_to_image_model.module.up_3.norm_s.param_free_norm.running_var" in full
    assert any("image_encoder.cnn" in k for k in full) and any("repr_net.0.weight" in k for k in full)
    m = tr.model.sg_to_layout.module
    assert all(c.predicates_transitive_weights is m.trans_candidates_weights for c in m.gconvs)   # ONE parameter
    assert get_conv_converse(tr.model).shape == (8, 8)
    assert get_conv_converse(full).shape == (8, 8)
    groups = tr.optimizer.param_groups
    assert groups[0]["lr"] == opt.learning_rate and groups[1]["lr"] == 1e-2 and len(groups[1]["params"]) == 1
    assert tr.discriminator.optimizer_d_img.param_groups[0]["betas"] == (0.5, 0.999)


def test_out_of_scope_components_fail_loudly(built, monkeypatch):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sg2im.layout import masks_to_layout
    from canonicalsg2im_amd.spade.models.networks import VGGLoss
    from canonicalsg2im_amd.synth import make_vocab
    monkeypatch.delenv("CSG_VGG19_WEIGHTS", raising=False)
    monkeypatch.delenv("CSG_VGG19_RANDOM", raising=False)
    with pytest.raises(RuntimeError, match="CSG_VGG19_WEIGHTS"):     # no pretrained weights, no silent random features
        VGGLoss([0])
    vgg = VGGLoss([0], weights="random").vgg                          # reference VGG19 keys (architecture.py:101-110)
    assert list(vgg.state_dict())[:6] == ["slice1.0.weight", "slice1.0.bias", "slice2.2.weight", "slice2.2.bias",
                                          "slice2.5.weight", "slice2.5.bias"]
    assert len(vgg.state_dict()) == 26 and "slice5.28.weight" in vgg.state_dict()
    with pytest.raises(RuntimeError, match="no CPU path"):          # compositing is a HIP kernel too: no CPU fallback
        masks_to_layout(torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1, 2, 2), 8, test_mode=True)
    from canonicalsg2im_amd.sg2im.layers import build_mlp
    mlp = build_mlp([6, 12, 4], batch_norm='batch')                   # reference keys: Linear 0, BatchNorm1d 1, Linear 3
    assert set(mlp.state_dict()) == {"0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var",
                                     "1.num_batches_tracked", "3.weight", "3.bias"}
    with pytest.raises(RuntimeError, match="CSG_VGG19_WEIGHTS"):     # default flags keep the VGG loss on
        T.Trainer(T.make_opt(make_vocab("tiny"), ["--image_size", "64,64", "--ngf", "4"]), torch.device("cpu"))
    tr = T.Trainer(T.make_opt(make_vocab("tiny"), ["--no_vgg_loss", "--image_size", "64,64", "--ngf", "4"]),
                   torch.device("cpu"))         # default use_img_disc=0: object + mask discriminators exist
    keys = set(tr.discriminator.obj_discriminator.state_dict())
    assert {"discriminator.cnn.0.0.weight", "discriminator.cnn.0.1.running_mean", "discriminator.cnn.0.6.bias",
            "discriminator.cnn.2.weight", "discriminator.real_classifier.weight",
            "discriminator.obj_classifier.bias"} <= keys
    assert "discriminator_1.model1.0.0.weight_orig" in tr.discriminator.mask_discriminator.state_dict()
    assert tr.discriminator.optimizer_d_obj.param_groups[0]["lr"] == 1e-4


def test_reference_command_lines_parse():
    """Every flag of the reference's scripts/args.py is accepted (README recipes parse unchanged)."""
    from canonicalsg2im_amd.scripts.args import build_parser
    p = build_parser()
    clevr = ("--dataset packed_clevr --batch_size 48 --image_size 256,256 --learned_transitivity 1 --use_img_disc 1 "
             "--loader_num_workers 8 --include_dummies 1 --output_dir out --checkpoint_every 5000 --print_every 100").split()
    a = p.parse_args(clevr)
    assert a.dataset == "packed_clevr" and a.batch_size == 48 and a.use_img_disc == 1 and a.loader_num_workers == 8
    coco = "--dataset coco --max_objects 1000 --image_size 256,256 --no_flip --shuffle_val 0 --timing 1".split()
    b = p.parse_args(coco)
    assert b.no_flip is True and b.shuffle_val is False and b.timing is True and b.use_img_disc == 0


def test_dropin_aliases_resolve_the_reference_import_paths(built):
    """after `dropin.install()` the reference trainer's imports (scripts/train.py:18-24)
    resolve to the HIP-backed modules — the SAME module objects, not second copies.  Run in a child process so
    that the aliases do not leak into this test session."""
    import subprocess
    import sys
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import canonicalsg2im_amd.dropin as dropin; dropin.install(scripts=True)\n"
        "from sg2im.meta_models import MetaGeneratorModel, MetaDiscriminatorModel\n"
        "from sg2im.model import get_conv_converse\n"
        "from sg2im.pix2pix_model import Pix2PixModel\n"
        "from sg2im.layout import boxes_to_layout, masks_to_layout\n"
        "from spade.models.networks.sync_batchnorm import DataParallelWithCallback\n"
        "from spade.models.networks import SPADEGenerator, MultiscaleDiscriminator, GANLoss\n"
        "from scripts.graphs_utils import calc_log_p\n"
        "import canonicalsg2im_amd.sg2im.meta_models as real\n"
        "assert MetaGeneratorModel is real.MetaGeneratorModel\n"
        "assert sys.modules['sg2im.meta_models'] is real\n"
        "assert SPADEGenerator.__module__ == 'canonicalsg2im_amd.spade.models.networks.generator'\n"
        "print('ALIASES_OK')\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALIASES_OK" in out.stdout, out.stderr[-2000:]


def test_weight_epoch_advances_where_tensor_versions_do_not(built):
    """Caches derived from trainable weights (the PatchGAN's permuted first-layer weight) are keyed on
    ops.weight_epoch(): the fused multi-tensor Adam updates parameters without bumping `_version`, so the key must
    advance on every optimiser step of ANY optimiser (torch's global post-step hook)."""
    from canonicalsg2im_amd import ops
    p = torch.nn.Parameter(torch.randn(4, 4))
    p.grad = torch.randn(4, 4)
    for kw in ({"fused": True}, {"foreach": True}, {}):
        opt = torch.optim.Adam([p], lr=1e-3, **kw)
        e0, v0 = ops.weight_epoch(), p._version
        before = p.detach().clone()
        opt.step()
        assert not torch.equal(before, p.detach())
        assert ops.weight_epoch() == e0 + 1, kw
        if kw.get("fused"):
            assert p._version == v0          # the reason the epoch exists; if torch changes this, the key still works
    sgd = torch.optim.SGD([p], lr=0.1)
    e0 = ops.weight_epoch()
    sgd.step()
    assert ops.weight_epoch() == e0 + 1


def test_spade_gamma_beta_parameters_share_one_allocation(built):
    """normalization._joined: the two parameters become the halves of one tensor (no torch.cat per call), gradients
    reach both, an optimiser step shows through the joined tensor, `module.to(...)` separates them and the next call
    joins them again; state_dict keys and values are untouched."""
    from canonicalsg2im_amd.spade.models.networks import normalization as N

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.randn(3, 4, 3, 3).contiguous(memory_format=torch.channels_last))
            self.b = torch.nn.Parameter(torch.randn(3, 4, 3, 3).contiguous(memory_format=torch.channels_last))
            self.ba = torch.nn.Parameter(torch.randn(3))
            self.bb = torch.nn.Parameter(torch.randn(3))

    m = M()
    a0, b0 = m.a.detach().clone(), m.b.detach().clone()
    opt = torch.optim.Adam(m.parameters(), lr=0.1)
    w = N._joined(m, "_jw", m.a, m.b)
    bias = N._joined(m, "_jb", m.ba, m.bb)
    assert w.shape == (6, 4, 3, 3) and torch.equal(w[:3], a0) and torch.equal(w[3:], b0)
    assert w.is_contiguous(memory_format=torch.channels_last) and bias.shape == (6,)
    assert m.a.data_ptr() == w.data_ptr() and m.b.data_ptr() == w.data_ptr() + 3 * w.stride(0) * 4
    ((w * torch.arange(6.0).view(6, 1, 1, 1)).sum() + (bias * torch.arange(6.0)).sum()).backward()
    assert m.a.grad.unique().tolist() == [0.0, 1.0, 2.0] and m.b.grad.unique().tolist() == [3.0, 4.0, 5.0]
    assert m.bb.grad.tolist() == [3.0, 4.0, 5.0]
    opt.step()
    w2 = N._joined(m, "_jw", m.a, m.b)
    assert w2.data_ptr() == w.data_ptr() and not torch.equal(w2[3:], b0) and torch.equal(w2[3:], m.b.detach())
    assert set(m.state_dict().keys()) == {"a", "b", "ba", "bb"}
    m2 = M()
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2.b, m.b)
    m.double()                                            # separates the parameters; the next call re-joins them
    w3 = N._joined(m, "_jw", m.a, m.b)
    assert w3.dtype == torch.float64 and m.a.data_ptr() == w3.data_ptr() and torch.equal(w3[3:], m.b.detach())


def test_data_parallel_wrapper_refuses_several_devices_without_a_process_group():
    """The reference's `--gpu_ids 0,1,2,3` in ONE process (replicate.py:50-67) would run the whole batch on one device here:
    the wrapper refuses at its first forward instead of doing so silently; one device id (or none) is the normal form."""
    import pytest
    from canonicalsg2im_amd.spade.models.networks.sync_batchnorm import DataParallelWithCallback
    lin = torch.nn.Linear(3, 2)
    x = torch.randn(4, 3)
    for ids in (None, [], [0]):
        assert torch.equal(DataParallelWithCallback(lin, device_ids=ids)(x), lin(x))
    dp = DataParallelWithCallback(lin, device_ids=[0, 1, 2, 3])
    assert dp.module is lin and dp.device_ids == [0, 1, 2, 3]          # constructing is fine (checkpoint tools do it)
    with pytest.raises(RuntimeError, match="one process per GPU"):
        dp(x)


def test_side_streams_are_a_no_op_off_the_gpu():
    """canonicalsg2im_amd/streams.py only engages for HIP tensors outside a capture; on the CPU the modules take their plain
    sequential path (there is no CPU product path, but module construction / host logic tests run here)."""
    from canonicalsg2im_amd import streams
    assert streams.usable(torch.zeros(2)) is False
    assert streams.usable(None) is False
