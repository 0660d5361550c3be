"""CPU tests of bench.py's own logic: the parity gate (`_parity`) on synthetic tensors and the `--gpus N` self-launch.

The gate's verdict on the HIP step must follow the HIP side only (losses vs the fp32 oracle, image vs the fp64 evaluation);
the fp32 oracle's distance from its own fp64 evaluation is reported and held to a sanity bound that fp32 noise cannot reach
(round 5's driver run failed on exactly that: a correct HIP step, an oracle 2.6e-5 in relative L2 from fp64, limit 2e-5)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _case(hip_noise=2e-6, oracle_noise=2.6e-5, loss_rel=1e-6, seed=0):
    """A tanh-like image with a few saturated pixels; `*_noise` = relative-L2 distance of that evaluation from the truth."""
    g = torch.Generator().manual_seed(seed)
    truth = torch.tanh(0.6 * torch.randn(2, 3, 64, 64, generator=g, dtype=torch.float64))

    def noisy(rel):
        n = torch.randn(truth.shape, generator=g, dtype=torch.float64)
        return (truth + n * (rel * truth.norm() / n.norm())).float()

    Go = {"total_loss": torch.tensor(3.25), "bbox_pred": torch.tensor(0.125), "bbox_pred_all": torch.linspace(0.1, 0.9, 8)}
    Do = {"total_img_loss": torch.tensor(1.5), "ac_loss_real": torch.tensor(2.0)}
    G0 = {k: (v.clone() if k == "bbox_pred_all" else float(v) * (1 + loss_rel)) for k, v in Go.items()}
    D0 = {k: float(v) * (1 - loss_rel) for k, v in Do.items()}
    return (G0, D0, noisy(hip_noise)), Go, Do, noisy(oracle_noise), truth


def test_good_hip_noisy_oracle_passes():
    """Round 5's driver record, restated: HIP 2e-6 from fp64, fp32 oracle 2.6e-5 from fp64 -> the step is accepted."""
    step, Go, Do, img_o, truth = _case()
    r = bench._parity(step, Go, Do, img_o, "t", img64=truth)
    assert r["ok"] and r["hip_ok"] and r["oracle_sane"]
    assert r["imgs_pred"]["judged_against"] == "fp64 oracle"
    assert r["imgs_pred"]["fp32_oracle_vs_fp64"]["rel_l2"] > 2e-5          # the number that used to fail the run
    assert r["imgs_pred"]["fp32_oracle_vs_fp64"]["sane"]
    # 3x the worst fp32 noise measured on the oracle still is not "broken"
    step, Go, Do, img_o, truth = _case(oracle_noise=8e-5)
    assert bench._parity(step, Go, Do, img_o, "t", img64=truth)["ok"]


def test_bad_hip_image_fails_whatever_the_oracle_does():
    step, Go, Do, img_o, truth = _case(hip_noise=1e-3, oracle_noise=1e-6)
    r = bench._parity(step, Go, Do, img_o, "t", img64=truth)
    assert not r["ok"] and not r["hip_ok"] and r["oracle_sane"]
    # a single pixel off by 1e-3 (relative L2 stays tiny) is caught by the per-pixel rule
    step, Go, Do, img_o, truth = _case(hip_noise=1e-7)
    step[2][0, 0, 3, 3] += 1e-3
    r = bench._parity(step, Go, Do, img_o, "t", img64=truth)
    assert not r["hip_ok"] and r["imgs_pred"]["pixels_over_rtol_plus_atol"] == 1
    # relative L2 alone: every pixel inside rtol + atol, the image as a whole 3e-5 away
    step, Go, Do, img_o, truth = _case(hip_noise=3e-5)
    r = bench._parity(step, Go, Do, img_o, "t", img64=truth)
    assert not r["hip_ok"] and r["imgs_pred"]["rel_l2"] > 2e-5


def test_bad_loss_or_bbox_fails():
    step, Go, Do, img_o, truth = _case(loss_rel=3e-4)
    r = bench._parity(step, Go, Do, img_o, "t", img64=truth)
    assert not r["ok"] and not r["hip_ok"] and r["max_rel"] > 1e-4
    step, Go, Do, img_o, truth = _case()
    step[0]["bbox_pred_all"][2] += 1e-3
    r = bench._parity(step, Go, Do, img_o, "t", img64=truth)
    assert not r["ok"] and not r["bbox_pred_all_ok"]
    step, Go, Do, img_o, truth = _case()
    del step[1]["ac_loss_real"]                                            # a loss the HIP step did not report
    Do2 = dict(Do)
    with pytest.raises(KeyError):
        bench._parity(step, Go, Do2, img_o, "t", img64=truth)


def test_broken_oracle_is_flagged_as_the_oracle():
    """An oracle whose fp32 evaluation is orders of magnitude from its fp64 one fails the run, and the record says which side."""
    step, Go, Do, img_o, truth = _case(oracle_noise=5e-3)
    r = bench._parity(step, Go, Do, img_o, "t", img64=truth)
    assert not r["ok"] and r["hip_ok"] and not r["oracle_sane"]
    assert not r["imgs_pred"]["fp32_oracle_vs_fp64"]["sane"]


def test_without_fp64_the_fp32_oracle_is_the_yardstick():
    step, Go, Do, img_o, truth = _case(hip_noise=2e-6, oracle_noise=0.0)
    r = bench._parity(step, Go, Do, img_o, "t")
    assert r["ok"] and r["imgs_pred"]["judged_against"] == "fp32 oracle" and r["oracle_sane"]
    step, Go, Do, img_o, truth = _case(hip_noise=1e-3, oracle_noise=0.0)
    assert not bench._parity(step, Go, Do, img_o, "t")["ok"]


def test_later_step_index_is_a_constant():
    """The checked step does not follow --warmup: bench.py names a fixed index."""
    assert bench.PARITY_LATER_STEP == 4
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "done[0] == PARITY_LATER_STEP" in src


def test_gpus_n_without_a_launcher_starts_n_ranks(monkeypatch):
    """`python bench.py --gpus 2 ...` with no torchrun environment: one torch.distributed.run child with 2 ranks of this
    file and the same arguments, before torch is imported in the parent; its status is the parent's status."""
    import subprocess
    seen = {}

    def fake_call(cmd, env=None, cwd=None):
        seen.update(cmd=cmd, env=env, cwd=cwd)
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "2" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "2", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_world_size_must_equal_gpus(monkeypatch):
    """Under a launcher whose world differs from --gpus the run refuses to print a line (n_gpus would lie)."""
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "--gpus 4 but WORLD_SIZE=1" in str(e.value.code)


# ------------------------------------------------------------------ --dump-outputs
class _StandInTrainer:
    """The attributes step_outputs reads, on CPU modules."""
    def __init__(self):
        torch.manual_seed(0)
        self.model = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 5))
        self.discriminator = torch.nn.Conv2d(3, 2, 3)            # 56 parameters: fewer than the sample
        self.last_model_out = (torch.rand(2, 3, 8, 8), torch.rand(2, 4, 4), None)


def test_step_outputs_are_what_the_step_returns_as_float_arrays():
    import numpy as np
    tr = _StandInTrainer()
    G = {"total_loss": torch.tensor(3.25), "bbox_pred_all": torch.linspace(0.1, 0.9, 8)}
    D = {"total_img_loss": torch.tensor(1.5), "count": torch.tensor(7)}
    a = bench.step_outputs(tr, G, D, sample=100)
    assert set(a) == {"G_total_loss", "G_bbox_pred_all", "D_total_img_loss", "D_count", "imgs_pred", "boxes_pred",
                      "weights_generator_sample", "weights_discriminator_sample"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["D_count"].dtype == np.float64 and float(a["D_count"]) == 7.0
    assert float(a["G_total_loss"]) == 3.25 and np.array_equal(a["G_bbox_pred_all"], G["bbox_pred_all"].numpy())
    assert np.array_equal(a["imgs_pred"], tr.last_model_out[0].numpy())
    # the weight sample: `sample` distinct entries of the flattened parameters, the same ones every time
    flat = torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]).numpy()
    s = a["weights_generator_sample"]
    assert s.shape == (100,) and np.isin(s, flat).all() and len(np.unique(s)) == 100
    assert np.array_equal(s, bench.step_outputs(tr, G, D, sample=100)["weights_generator_sample"])
    # a network smaller than the sample is written whole
    assert a["weights_discriminator_sample"].size == sum(p.numel() for p in tr.discriminator.parameters())
    # an optimiser step shows in the sample
    with torch.no_grad():
        for p in tr.model.parameters():
            p.add_(1e-3)
    assert not np.array_equal(s, bench.step_outputs(tr, G, D, sample=100)["weights_generator_sample"])


def test_write_outputs_round_trip_and_limits(tmp_path):
    import numpy as np
    arrays = {"x": np.arange(6, dtype=np.float32).reshape(2, 3), "y": np.float64(2.5) * np.ones(4)}
    assert bench.write_outputs(str(tmp_path / "d"), arrays) == 6 * 4 + 4 * 8
    for k, v in arrays.items():
        r = np.load(str(tmp_path / "d" / (k + ".npy")))
        assert r.dtype == v.dtype and np.array_equal(r, v)
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), arrays, limit=50)
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "int"), {"i": np.arange(3)})
    assert not (tmp_path / "big").exists() and not (tmp_path / "int").exists()
    assert bench.DUMP_LIMIT_BYTES == 64 << 20


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.steps == 3 and a.dump_outputs == "out"


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full"])
    assert bench.parse().full is True


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_dump_outputs_repeat_run_to_run_and_follow_steps(tmp_path):
    """Two runs with the same arguments write the same arrays, bit for bit; one more timed step changes the weights."""
    import json
    import subprocess
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--batch", "2", "--image_size", "64",
            "--ngf", "8", "--ndf", "8", "--no_cpu_baseline", "--no_vgg_variant", "--no_prof", "--no_gen_metric"]
    dumps = {}
    for tag, steps in (("a", 2), ("b", 2), ("c", 3)):
        out = subprocess.run(base + ["--steps", str(steps), "--dump-outputs", str(tmp_path / tag)], cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and json.loads(lines[0])["steps"] == steps
        dumps[tag] = {f[:-4]: np.load(str(tmp_path / tag / f)) for f in sorted(os.listdir(str(tmp_path / tag)))}
    a, b, c = dumps["a"], dumps["b"], dumps["c"]
    assert {"G_total_loss", "D_total_img_loss", "G_bbox_pred_all", "imgs_pred", "weights_generator_sample",
            "weights_discriminator_sample"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert a["imgs_pred"].shape == (2, 3, 64, 64)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])]
    assert set(a) == set(c) and not np.array_equal(a["weights_generator_sample"], c["weights_generator_sample"])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_times_the_same_steps_as_a_full_run(tmp_path):
    """Without --full the line holds the headline only; --full adds the legs after the timed region (tables, CPU baseline,
    oracle parity), and both runs time the same steps: their dumped outputs are identical, bit for bit."""
    import json
    import subprocess
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
            "--image_size", "64", "--ngf", "8", "--ndf", "8", "--no_vgg_variant"]
    lines, dumps = {}, {}
    for tag, extra in (("plain", []), ("full", ["--full"])):
        out = subprocess.run(base + extra + ["--dump-outputs", str(tmp_path / tag)], cwd=ROOT, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        found = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(found) == 1
        lines[tag] = json.loads(found[0])
        dumps[tag] = {f[:-4]: np.load(str(tmp_path / tag / f)) for f in sorted(os.listdir(str(tmp_path / tag)))}
    plain, full = lines["plain"], lines["full"]
    headline = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "losses_finite"}
    assert headline <= set(plain) and headline <= set(full)
    assert plain["metric"] == full["metric"] and plain["unit"] == full["unit"] == "img/s" and plain["dtype"] == "f32"
    legs = {"cpu_baseline", "parity_b16", "parity_later_step", "kernels", "hbm_kernels", "roofline", "roofline_step"}
    assert not legs & set(plain), legs & set(plain)
    assert {"cpu_baseline", "parity_b16", "parity_later_step", "kernels"} <= set(full)
    assert full["parity_b16"]["ok"] and full[full["parity_later_step"]]["ok"]
    assert ("hip_graphs" in plain) == ("hip_graphs" in full)
    if "hip_graphs" in plain:
        assert "eager_ms_per_step" in full["hip_graphs"] and "eager_ms_per_step" not in plain["hip_graphs"]
        assert {k: v for k, v in plain["hip_graphs"].items() if k != "note"} == \
               {k: v for k, v in full["hip_graphs"].items() if k not in ("note", "eager_ms_per_step")}
    a, b = dumps["plain"], dumps["full"]
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])]
