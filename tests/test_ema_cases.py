"""Host-side checks of the weight EMA (no GPU): the case table of tests/ema_cases.py is well-formed, its float64 restatement
agrees with an fp32 evaluation of the stated sequence within its own bound, the warm-up rule gives the hand-worked values,
the planning entry and the flags refuse what they should, and a trainer with the EMA off writes today's checkpoint keys.

`WeightEMA` itself is NOT constructible on the CPU (its table is made by ops.EmaTable, which refuses host tensors as every
op does): that `WeightEMA.state_dict()` has the model's keys is checked in tests/test_gpu_ema.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ema_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "2"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from canonicalsg2im_amd import _lib
    return _lib


def test_table_is_well_formed(built):
    from canonicalsg2im_amd import ops
    hdr = open(os.path.join(ROOT, "include", "csg_hip.h")).read()
    C = ec.chunk()
    assert C == int(re.search(r"#define CSG_EMA_CHUNK (\d+)", hdr).group(1)) and C % 1024 == 0
    assert (ops.EMA_AVERAGE, ops.EMA_COPY) == (ec.AVERAGE, ec.COPY)
    assert hasattr(built.lib, "csg_ema_apply") and hasattr(built.lib, "csg_ema_table_plan")
    rows = ec.table()
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names) and len(rows) >= 40
    singles = {r["items"][0][0] for r in rows if len(r["items"]) == 1}
    assert singles == {0, 1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3}
    for kind in (ec.AVERAGE, ec.COPY):
        assert {r["items"][0][0] for r in rows if len(r["items"]) == 1 and r["items"][0][1] == kind} == singles
    two = [r for r in rows if len(r["items"]) == 2 and r["items"][0][2] == "normal"]
    assert all({it[1] for it in r["items"]} == {ec.AVERAGE, ec.COPY} for r in two)
    decays = {r["decay"] for r in two}
    assert {0.0, 1.0, 0.5, 0.999, 0.9999} <= decays
    assert {ec.warmup_decay(0.9999, n) for n in (1, 2, 90, 100000)} <= decays
    many = [r for r in rows if len(r["items"]) == 300]
    assert len(many) == 3 and {r["decay"] for r in many} == {0.999, 0.5, 1.0}
    for r in many:
        kinds = [it[1] for it in r["items"]]
        sizes = [it[0] for it in r["items"]]
        assert 100 < sum(kinds) < 200 and min(sizes) == 0 and max(sizes) > C and len(set(sizes)) > 30
        assert sum(1 for s in sizes if s % 4) > 150                     # most slots need padding
    assert any(any(n % 4 for n, _, _ in r["items"][:-1]) and len(r["items"]) > 3 for r in rows)
    assert any(len(r["items"]) == 3 and r["items"][1][0] == 0 and r["items"][0][0] and r["items"][2][0] for r in rows)
    special = [r for r in rows if r["items"][0][2] == "special"]
    assert {r["decay"] for r in special} >= {0.0, 1.0, 0.5, 0.999, 0.9999}
    s = ec.SPECIALS
    assert np.isnan(s).sum() == 3 and np.isinf(s).sum() == 2 and (s == 0).sum() == 2 and np.signbit(s[s == 0]).sum() == 1
    sub = np.abs(s[np.isfinite(s) & (s != 0)]) < np.finfo(np.float32).tiny
    assert sub.sum() == 2 and np.nanmax(np.abs(s[np.isfinite(s)])) == np.finfo(np.float32).max
    for r in special:                      # every pair (p, e) occurs, in the 16-byte body and in a 3-float tail
        (p, e, _), _ = ec.make(r)
        pairs = set(zip(p.view(np.uint32).tolist(), e.view(np.uint32).tolist()))
        assert len(pairs) == len(s) ** 2 and p.size % 4 == 3
    # data is reproducible and has the sizes the row states
    for r in rows[:6] + many[:1]:
        a, b = ec.make(r), ec.make(r)
        assert [x[0].size for x in a] == [it[0] for it in r["items"]]
        assert all(np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and
                   np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(a, b))


def test_layout_and_plan(built):
    """Slots start at multiples of 4 floats and do not overlap; the planning entry counts chunks per item, gives empty items
    none, and refuses misaligned or null addresses and unknown kinds — on the host, nothing is launched."""
    from canonicalsg2im_amd import ops
    C = ec.chunk()
    numels = [3, 5, 0, 1, 4, C - 1, C, C + 1, 2 * C + 3, 0]
    offs, total = ops.ema_layout(numels)
    assert all(o % 4 == 0 for o in offs) and total % 4 == 0
    assert all(offs[i] + numels[i] <= offs[i + 1] < offs[i] + numels[i] + 4 for i in range(len(offs) - 1))
    assert total == offs[-1] + numels[-1]
    arr = (built.EmaItem * len(numels))()
    for i, n in enumerate(numels):
        arr[i].src, arr[i].dst, arr[i].numel, arr[i].kind = 0x10000 + 16 * i, 0x900000 + 4 * offs[i], n, i % 2
    chunks = built.lib.csg_ema_table_plan(arr, len(numels))
    per = [-(-n // C) for n in numels]
    assert chunks == sum(per) and [arr[i].chunk0 for i in range(len(numels))] == [sum(per[:i]) for i in range(len(numels))]
    for field, value, msg in (("src", 0x10004, "16-byte"), ("dst", 0x900008, "16-byte"), ("kind", 2, "kind"),
                              ("numel", -1, "elements"), ("src", None, "null")):
        bad = (built.EmaItem * 2)()
        for i in range(2):
            bad[i].src, bad[i].dst, bad[i].numel, bad[i].kind = 0x10000, 0x900000, 8, 0
        setattr(bad[1], field, value)
        assert built.lib.csg_ema_table_plan(bad, 2) < 0 and msg in built.last_error(), (field, built.last_error())
    assert built.lib.csg_ema_table_plan(arr, 0) < 0
    assert ctypes.sizeof(built.EmaItem) == 40
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.EmaTable([torch.zeros(8)], [ops.EMA_AVERAGE])
    with pytest.raises(RuntimeError, match="fp32"):
        ops.EmaTable([torch.zeros(8, dtype=torch.float64)], [ops.EMA_AVERAGE])


def test_scalars_are_the_wrappers(built):
    from canonicalsg2im_amd import ops
    for D in ec.DECAYS + tuple(ec.warmup_decay(0.9999, n) for n in ec.WARMUP_N) + (1e-9, 1.0 - 1e-12):
        d, omd = ops.ema_scalars(D)
        assert (d, omd) == ec.scalars(D)
        assert d == float(np.float32(D)) and omd == float(np.float32(1.0 - D)) and 0.0 <= d <= 1.0 and 0.0 <= omd <= 1.0
    assert ops.ema_scalars(1.0) == (1.0, 0.0) and ops.ema_scalars(0.0) == (0.0, 1.0)
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="decay"):
            ops.ema_scalars(bad)


def test_restatement_agrees_with_an_fp32_evaluation(built):
    """Every row: the fp32 evaluation of the stated sequence lies within the restatement's own bound (and is EQUAL, as bits,
    where the contract is a copy); the bound is not vacuous — a third rounding (the unfused a * b + c) or a decay that is
    off by one fp32 ulp is beyond it somewhere in the table."""
    worst, unfused_beyond, ulp_beyond = 0.0, 0, 0
    for case in ec.table():
        d, omd = ec.scalars(case["decay"])
        for j, (p, e, kind) in enumerate(ec.make(case)):
            what = "%s item %d" % (case["name"], j)
            exact, ref = ec.restate(p, e, kind, d, omd)
            got = ec.fp32_evaluation(p, e, kind, d, omd)
            if exact:
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), what
                continue
            bound = ec.step_bound(p, e, ref, d, omd)
            worst = max(worst, ec.check_average(got, ref, bound, what))
            fin = np.isfinite(ref) & (np.abs(ref) < 1e30)
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                unfused = ((np.float32(d) * e).astype(np.float32) + (np.float32(omd) * p).astype(np.float32)).astype(np.float32)
                d_up = float(np.nextafter(np.float32(d), np.float32(2.0)))
                off = ec.fp32_evaluation(p, e, kind, d_up, omd)
                unfused_beyond += int((np.abs(unfused.astype(np.float64) - ref)[fin] > bound[fin]).sum())
                ulp_beyond += int((np.abs(off.astype(np.float64) - ref)[fin] > bound[fin]).sum())
    assert 0.3 < worst <= 1.0, worst
    assert unfused_beyond > 0 and ulp_beyond > 0, (unfused_beyond, ulp_beyond)


def test_repeated_updates_bound():
    assert ec.steps_factor(4, 0.999) == 4.0 and ec.steps_factor(4, 0.5) == 2.0 and ec.steps_factor(10 ** 6, 0.999) == pytest.approx(1000.0)
    assert ec.steps_factor(7, 1.0) == 7.0
    # 200 fp32 updates of one tensor against the float64 shadow stay inside it
    rng = np.random.RandomState(0)
    e32 = rng.standard_normal(4096).astype(np.float32)
    e64 = e32.astype(np.float64)
    worst_b, d_max = np.zeros(4096), 0.0
    for n in range(1, 201):
        p = (e32 + 0.01 * rng.standard_normal(4096)).astype(np.float32)
        d, omd = ec.scalars(ec.warmup_decay(0.99, n))
        ref = d * e64 + omd * p.astype(np.float64)            # the float64 shadow, advanced with the same scalars
        worst_b = np.maximum(worst_b, ec.step_bound(p, e32, ref, d, omd))
        e32, e64, d_max = ec.fp32_evaluation(p, e32, ec.AVERAGE, d, omd), ref, max(d_max, d)
        assert (np.abs(e32.astype(np.float64) - e64) <= worst_b * ec.steps_factor(n, d_max)).all(), n


def test_warmup_rule_by_hand(built):
    from canonicalsg2im_amd.ema import check_decay, decay_at
    assert decay_at(0.999, 1) == 2.0 / 11.0
    assert decay_at(0.999, 2) == 3.0 / 12.0 == 0.25
    assert decay_at(0.999, 90) == 0.91
    assert decay_at(0.999, 100000) == 0.999 and decay_at(0.9999, 10 ** 9) == 0.9999
    assert decay_at(0.5, 1) == 2.0 / 11.0 and decay_at(0.5, 8) == 0.5 and decay_at(0.5, 9) == 0.5
    assert decay_at(0.999, 1, warmup=False) == 0.999
    assert all(decay_at(0.9999, n) == ec.warmup_decay(0.9999, n) for n in (1, 2, 3, 90, 8990, 8991, 100000))
    assert check_decay(1) == 1.0 and check_decay(0.5) == 0.5
    for bad in (0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            check_decay(bad)


def test_flags(built):
    from canonicalsg2im_amd.scripts import evaluate, sample, train
    a = train.build_parser().parse_args([])
    assert a.ema_decay == 0 and a.ema_warmup == 1 and a.val_ema == 0
    a = train.build_parser().parse_args(["--ema_decay", "0.999", "--ema_warmup", "0", "--val_every", "5", "--val_ema", "1"])
    assert a.ema_decay == 0.999 and a.ema_warmup == 0 and a.val_ema == 1
    for bad in (["--ema_decay", "-0.5"], ["--ema_decay", "1.5"], ["--ema_decay", "nan"], ["--ema_warmup", "2"], ["--val_ema", "2"]):
        with pytest.raises(SystemExit):
            train.build_parser().parse_args(bad)
    with pytest.raises(SystemExit, match="ema_decay"):
        train.main(["--val_every", "5", "--val_ema", "1"])
    assert sample.build_parser().parse_args([]).use_ema == 0 and sample.build_parser().parse_args(["--use_ema", "1"]).use_ema == 1
    assert evaluate.build_parser().parse_args(["--use_ema", "1"]).use_ema == 1
    with pytest.raises(SystemExit, match="checkpoint_name"):
        sample.parse_args(["--use_ema", "1"])


def test_checkpoint_keys(built):
    """EMA off — no attribute at all, or --ema_decay 0 —: `trainer.ema is None` and checkpoint_dict has exactly the keys it had
    before the feature.  The sampler's reader refuses a checkpoint without the averaged weights and names the flag."""
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.sample import model_state_of
    from canonicalsg2im_amd.synth import make_vocab
    today = {"model_state", "gans_model_state", "d_img_state", "d_obj_state", "d_mask_state", "d_img_optim_state",
             "d_obj_optim_state", "d_mask_optim_state", "optim_state", "vocab", "counters"}
    for strip in (True, False):
        opt = T.make_opt(make_vocab("tiny"), TINY)
        if strip:
            del opt.ema_decay, opt.ema_warmup
        torch.manual_seed(0)
        tr = T.Trainer(opt, torch.device("cpu"))
        assert tr.ema is None
        ck = tr.checkpoint_dict(3, 1)
        assert set(ck) == today and ck["counters"] == {"t": 3, "epoch": 1}
    with pytest.raises(KeyError, match="--ema_decay"):
        model_state_of(ck, use_ema=True)
    assert model_state_of(ck) is ck["model_state"]
    ck["model_ema_state"] = {"module." + k: v for k, v in ck["model_state"].items()}
    assert set(model_state_of(ck, use_ema=True)) == set(ck["model_state"])
    with pytest.raises(ValueError, match="ema_decay"):           # a hand-built namespace with a decay out of range
        T.Trainer(T.make_opt(make_vocab("tiny"), TINY, ema_decay=1.5), torch.device("cpu"))
