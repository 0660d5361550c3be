"""Validation (canonicalsg2im_amd/evaluate.py, csrc/metrics.hip) — what can be checked without a GPU: the box-IoU fixture
recorded from the reference is self-consistent, the library exports the entry point, the modules import and refuse the CPU,
and the command lines parse what they should."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def fixture():
    return load_golden("box_iou")


def test_fixture_aggregates_are_float64_sums_of_its_per_object_values(fixture):
    meta, z = fixture
    assert meta["per_sample"] == ["sum_iou", "over05", "over03", "counted"]
    seeded = np.zeros(4)
    for name in meta["batches"]:
        iou, counted = z[name + "_iou"].numpy(), z[name + "_counted"].numpy().astype(bool)
        o05, o03, per = z[name + "_over05"].numpy(), z[name + "_over03"].numpy(), z[name + "_per_sample"].numpy()
        assert iou.dtype == np.float32 and per.dtype == np.float64 and per.shape == (iou.shape[0], 4)
        assert z[name + "_pred"].shape == z[name + "_gt"].shape == iou.shape + (4,)
        assert not iou[~counted].any() and not o05[~counted].any() and not o03[~counted].any()
        # the thresholds are those of the fp32 comparison the reference makes; NaN fails both
        with np.errstate(invalid="ignore"):
            assert np.array_equal(o05.astype(bool), counted & (iou > np.float32(0.5)))
            assert np.array_equal(o03.astype(bool), counted & (iou > np.float32(0.3)))
        for b in range(iou.shape[0]):
            want = np.array([iou[b][counted[b]].astype(np.float64).sum(), o05[b].sum(), o03[b].sum(), counted[b].sum()])
            assert np.array_equal(np.isnan(want), np.isnan(per[b]))
            assert np.allclose(per[b], want, rtol=1e-12, atol=0, equal_nan=True), (name, b, per[b], want)
        # the reference's mask: any ground-truth value != -1, and objs[.,0] != __image__
        gt, objs = z[name + "_gt"].numpy(), z[name + "_objs"].numpy()
        assert np.array_equal(counted, (gt != -1).any(-1) & (objs[..., 0] != meta["image_id"][name]))
        if name != "hand":
            seeded += per.sum(0)
    s = meta["seeded"]
    assert (s["counted"], s["over05"], s["over03"], s["nan"]) == (702, 32, 119, 0)
    assert seeded[3] == 702 and seeded[1] == 32 and seeded[2] == 119
    assert abs(seeded[0] - s["sum_iou"]) <= 1e-12 * s["sum_iou"]


def test_fixture_hand_rows_hold_the_cases_the_seeded_batches_lack(fixture):
    meta, z = fixture
    iou, counted = z["hand_iou"][0], z["hand_counted"][0]
    assert iou[0] == 1.0 and iou[1] == 0.0 and iou[2] == 0.0 and torch.isnan(iou[3]) and iou[4] == 0.25
    assert counted.tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 1]
    assert float(z["hand_pred"][0].min()) < 0.0 and float(z["hand_pred"][0].max()) > 1.0       # clamped by the metric
    objs = z["hand_objs"][0, :, 0]
    assert int(objs[5]) == meta["image_id"]["hand"] != 0 and int(objs[7]) == 0 and counted[7] == 1   # not remove_dummy_objects
    assert torch.isnan(z["hand_per_sample"][:, 0]).all() and z["hand_per_sample"][0, 3] == 7
    assert torch.equal(z["hand_iou"][1].flip(0).nan_to_num(-1.0), iou.nan_to_num(-1.0))


def test_library_exports_box_iou_at_revision_111():
    from canonicalsg2im_amd import _lib
    assert "csg_box_iou" in _lib.SIGNATURES and hasattr(_lib.lib, "csg_box_iou")
    assert _lib.lib.csg_version() >= 111
    names = [_lib.lib.csg_prof_kernel_name(k).decode() for k in range(_lib.lib.csg_prof_num_kernels())]
    assert "box_iou" in names
    # limits are refused before anything is launched (no device needed): B = 0, and null operands
    assert _lib.lib.csg_box_iou(None, None, None, 0, 4, 1, 0, None, None, None, None, None) == -1
    assert "csg_box_iou" in _lib.last_error()
    assert _lib.lib.csg_box_iou(None, None, None, 2, 4, 1, 0, None, None, None, None, None) == -1


def test_metrics_source_is_compiled_without_contraction():
    import __graft_entry__ as g
    assert "metrics.hip" in g.SOURCES and "-ffp-contract=off" in g.EXTRA_FLAGS["metrics.hip"]


def test_evaluator_imports_and_refuses_the_cpu():
    import types
    import canonicalsg2im_amd.evaluate as E
    from canonicalsg2im_amd import ops
    tr = types.SimpleNamespace(device=torch.device("cpu"), opt=None, model=None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        E.Evaluator(tr)
    z = torch.zeros(1, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.box_iou(z, z, torch.zeros(1, 2, 1, dtype=torch.int64), 0, torch.zeros(4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="totals"):
        ops.box_iou(z, z, torch.zeros(1, 2, 1, dtype=torch.int64), 0, torch.zeros(4))


def test_fetch_returns_every_tensor_from_one_buffer():
    from canonicalsg2im_amd.evaluate import _fetch
    g = torch.Generator().manual_seed(0)
    src = {"a": torch.randn(3, 5, generator=g), "b": torch.arange(7, dtype=torch.uint8), "c": torch.randn(2, dtype=torch.float64, generator=g),
           "d": torch.arange(3, dtype=torch.int64), "e": torch.empty(0, 4)}
    out = _fetch(src)
    assert list(out) == list(src)
    for k in src:
        assert out[k].dtype == src[k].dtype and torch.equal(out[k], src[k]), k
    base = out["a"].untyped_storage().data_ptr()
    assert all(out[k].untyped_storage().data_ptr() == base for k in "abcd")


def test_command_lines_accept_and_reject_what_they_should(tmp_path):
    from canonicalsg2im_amd.scripts import evaluate as ev, train as tr
    assert tr.build_parser().parse_args([]).val_every == 0
    assert tr.build_parser().parse_args(["--val_every", "50"]).val_every == 50
    with pytest.raises(SystemExit):
        tr.build_parser().parse_args(["--val_every", "often"])
    with pytest.raises(SystemExit):
        tr.main(["--val_every", "-1"])
    ck = tmp_path / "itr_1.pt"
    ck.write_bytes(b"")
    args = ev.parse_args(["--checkpoint_name", str(ck), "--output_dir", str(tmp_path), "--num_val_samples", "32",
                          "--batch_size", "16", "--use_img_disc", "1"])
    assert args.num_val_samples == 32 and args.output_dir == str(tmp_path) and args.checkpoint_name == str(ck)
    assert ev.parse_args(["--checkpoint_name", str(ck)]).num_val_samples == 1024          # the reference's default
    for bad in ([], ["--checkpoint_name", str(tmp_path / "missing.pt")], ["--checkpoint_name", str(ck), "--num_val_samples", "0"],
                ["--checkpoint_name", str(ck), "--val_every", "3"]):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    # validation seeds lie above every training seed
    assert ev.VAL_SEED_BASE == 2 ** 40


def test_log_line_carries_the_three_metrics(capsys):
    from canonicalsg2im_amd.scripts.evaluate import log_results
    log_results({"bbox_pred": torch.tensor(0.5), "avg_iou": torch.tensor(0.125, dtype=torch.float64),
                 "total_iou_05": torch.tensor(0.0), "total_iou_03": torch.tensor(0.25)}, 7, "GT VAL")
    line = capsys.readouterr().out.strip()
    assert line.startswith("Iter: 7, GT VAL avg_iou: 0.1250 total_iou_03: 0.2500 total_iou_05: 0.0000") and "bbox_pred 0.5000" in line
    assert json.dumps({"x": 1})          # (json is what write_outputs uses; nothing else is needed on the host)
