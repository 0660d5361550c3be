"""Host side of the sampler (canonicalsg2im_amd/sample.py, scripts/sample.py): checkpoint handling, the command line, the
refusal of CPU tensors, and an import that stays free of PIL.  No GPU, no kernel launch."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _sampler(extra=()):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import Sampler
    from canonicalsg2im_amd.synth import make_vocab
    opt = T.make_opt(make_vocab("tiny"), TINY + list(extra))
    return Sampler(opt, "cpu")


def test_sampler_holds_a_generator_and_nothing_else(built):
    s = _sampler()
    assert not s.model.training and all(not m.training for m in s.model.modules())
    names = [n for n, _ in s.model.named_children()]
    assert sorted(names) == ["layout_to_image_model", "sg_to_layout"], names


def test_reference_style_checkpoint_loads_strictly(built):
    """What the reference's save_checkpoint writes (scripts/train.py:488-520): `model_state` beside a `gans_model_state`
    whose keys carry DataParallel's `module.` prefix, discriminator and optimiser entries.  Only `model_state` is read."""
    src, dst = _sampler(), _sampler()
    with torch.no_grad():
        for p in src.model.parameters():
            p.add_(0.25)
    ckpt = {"model_state": {k: v.clone() for k, v in src.model.state_dict().items()},
            "gans_model_state": {"module.netD.whatever": torch.zeros(3)}, "d_img_state": {}, "optim_state": {},
            "counters": {"t": 7, "epoch": 0}}
    dst.load(ckpt)
    for (k, a), (_, b) in zip(src.model.state_dict().items(), dst.model.state_dict().items()):
        assert torch.equal(a, b), k
    assert not dst.model.training
    # a generator saved from inside a DataParallel wrapper: every key carries `module.`
    wrapped = {"model_state": {"module." + k: v for k, v in ckpt["model_state"].items()}}
    _sampler().load(wrapped)
    with pytest.raises(KeyError):
        _sampler().load({"gans_model_state": {}})


def test_strict_load_refuses_another_mask_size(built):
    ckpt = {"model_state": _sampler().model.state_dict()}
    with pytest.raises(RuntimeError, match="mask_net"):
        _sampler(["--mask_size", "16"]).load(ckpt)
    with pytest.raises(RuntimeError, match="mask_net"):
        _sampler().load({"model_state": _sampler(["--mask_size", "16"]).model.state_dict()})


def test_generate_refuses_cpu_tensors(built):
    s = _sampler()
    objs = torch.zeros((1, 3, 1), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.generate(objs, torch.zeros((1, 2, 3), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int64))


def test_command_line_parses_the_reference_flags_and_its_own(built, tmp_path):
    from canonicalsg2im_amd.scripts import sample as cli
    a = cli.parse_args(["--dataset", "packed_coco", "--image_size", "128,128", "--batch_size", "8", "--num_samples", "20",
                        "--output_dir", str(tmp_path), "--ngf", "32", "--mask_size", "16"])
    assert (a.num_samples, a.batch_size, a.image_size, a.output_dir, a.ngf, a.mask_size) == (20, 8, (128, 128), str(tmp_path),
                                                                                              32, 16)
    assert cli.parse_args([]).num_samples == 16 and cli.parse_args([]).checkpoint_name == "checkpoint"
    ck = tmp_path / "itr_1.pt"
    ck.write_bytes(b"")
    assert cli.parse_args(["--checkpoint_name", str(ck)]).checkpoint_name == str(ck)
    with pytest.raises(SystemExit):
        cli.parse_args(["--checkpoint_name", str(tmp_path / "absent.pt")])
    with pytest.raises(SystemExit):
        cli.parse_args(["--num_samples", "0"])


def test_importing_the_sampler_does_not_import_pil(built):
    code = ("import sys; import canonicalsg2im_amd.sample, canonicalsg2im_amd.scripts.sample; "
            "bad = [m for m in sys.modules if m == 'PIL' or m.startswith('PIL.')]; assert not bad, bad")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
