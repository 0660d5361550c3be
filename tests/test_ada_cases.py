"""Adaptive strength of the discriminator augmentation, without a device: the restatements of tests/ada_cases.py against
their fixed vectors, the host entry points of the library (the host half of csrc/csg_augment.h) against the restatements,
the flags and their refusals, and step24."""
import math

import numpy as np
import pytest
import torch

import ada_cases as ad
import augment_cases as ac


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_against_fixed_vectors():
    for key, draws in ad.DRAW_VECTORS:
        h = ac.key_py(*key)
        assert tuple(ac.step_py(h, 8 + j) >> 40 for j in range(3)) == draws, key
        for p24 in ad.P24_VALUES + [d for d in draws] + [d + 1 for d in draws]:
            assert ad.gate_py(*key, p24) == sum(1 << j for j in range(3) if draws[j] < p24)
    assert [ad.gate_py(*ad.GATE_VECTORS_KEY, n, 1 << 23) for n in range(8)] == ad.GATE_VECTORS
    assert ad.gate_np(*ad.GATE_VECTORS_KEY, 8, 1 << 23).tolist() == ad.GATE_VECTORS
    for key in ad.KEYS:
        for p24 in ad.P24_VALUES:
            assert ad.gate_np(*key, 33, p24).tolist() == [ad.gate_py(*key, n, p24) for n in range(33)], (key, p24)


def test_next_p_restatement_against_its_table():
    for args, want in ad.NEXT_P_TABLE:
        assert ad.next_p(*args) == want, (args, want)
    for args, want in ad.STEP24_VECTORS:
        assert ad.step24(*args) == want, args
    assert ad.T06 == int(math.floor(0.6 * ad.ONE + 0.5))


def test_gate_rate_of_the_restatement():
    """65 536 rows at p24 = 2^22 (p = 1/4): each policy's count lies within 6 sqrt(n p (1 - p)) = 665.1 of n p = 16 384 — six
    standard deviations of a binomial count: a hash whose bits were biased or tied between draws would not stay inside."""
    n, p24 = 65536, 1 << 22
    p = p24 / ad.ONE
    bound = 6.0 * math.sqrt(n * p * (1.0 - p))
    g = ad.gate_np(12345, 7, 1, 0, n, p24)
    counts = [int(((g >> j) & 1).sum()) for j in range(3)]
    print("counts %s, n p = %.0f, bound %.1f" % (counts, n * p, bound))
    for c in counts:
        assert abs(c - n * p) <= bound, counts
    both = int(((g & 3) == 3).sum())                     # two policies together: p^2, the draws are separate
    assert abs(both - n * p * p) <= 6.0 * math.sqrt(n * p * p * (1.0 - p * p)), both


def test_sign_restatement():
    S, C = ad.sign_count([ad.SPECIALS])
    assert (S, C) == (0, 16)                             # six positive, six negative, four of sign 0 — by inspection
    assert ad.sign_count([np.array([0.0, -0.0, np.nan], np.float32)]) == (0, 3)
    assert ad.sign_count([np.array([1e-45, 2.0], np.float32), np.array([-np.inf], np.float32)]) == (1, 3)


# ------------------------------------------------------------------------------------------------ the host entry points
def test_gate_host_equals_the_restatement():
    from canonicalsg2im_amd import ops
    for key in ad.KEYS:
        seed, iteration, pass_id, rank = key
        for p24 in ad.P24_VALUES:
            got = ops.augment_gate_host(seed, iteration, pass_id, 300, p24, rank=rank).numpy()
            assert got.dtype == np.int32 and np.array_equal(got, ad.gate_np(seed, iteration, pass_id, rank, 300, p24)), (key, p24)
            if p24 == ad.ONE:
                assert (got == 7).all()
            if p24 == 0:
                assert (got == 0).all()
    got = ops.augment_gate_host(*ad.GATE_VECTORS_KEY[:3], 8, 1 << 23, rank=ad.GATE_VECTORS_KEY[3])
    assert got.tolist() == ad.GATE_VECTORS
    assert ops.augment_gate_host(0, 0, 0, 0, 5).shape == (0,)


def test_gate_host_counts_equal_the_restatement():
    from canonicalsg2im_amd import ops
    n, p24 = 65536, 1 << 22
    got = ops.augment_gate_host(12345, 7, 1, n, p24).numpy()
    want = ad.gate_np(12345, 7, 1, 0, n, p24)
    for j in range(3):
        assert int(((got >> j) & 1).sum()) == int(((want >> j) & 1).sum())
    assert np.array_equal(got, want)


def test_gate_leaves_the_parameter_rows_alone():
    """Draws 8..10 are new; the rows of draws 1..7 are what tests/augment_cases.py fixed."""
    from canonicalsg2im_amd import ops
    seed, iteration, pass_id, rank, H = ac.ROW_VECTORS_KEY
    assert ops.augment_table_host(seed, iteration, pass_id, 3, H, rank=rank).tolist() == ac.ROW_VECTORS


def _host_update(words, T24, step24):
    from canonicalsg2im_amd import ops
    ctrl = torch.tensor(words, dtype=torch.int64)
    ops.ada_update_host(ctrl, T24, step24)
    return ctrl.tolist()


def test_update_host_over_the_table():
    for (p24, S, C, T24, step24), want in ad.NEXT_P_TABLE:
        words = [p24, S, C, 41, -5, 9, 0, 0]
        got = _host_update(words, T24, step24)
        assert got == ad.update_words(words, T24, step24), (p24, S, C, T24, step24, got)
        assert got[0] == want and got[1:6] == [0, 0, 42, S, C]


def test_update_host_moves_the_counts():
    got = _host_update([100, 30, 40, 0, 0, 0, 0, 0], ad.T06, 10)
    assert got == [110, 0, 0, 1, 30, 40, 0, 0]
    got = _host_update(got, ad.T06, 10)                  # nothing counted since: p stays, the _last words say so
    assert got == [110, 0, 0, 2, 0, 0, 0, 0]


def test_host_refusals():
    from canonicalsg2im_amd._lib import last_error, lib
    import ctypes
    ctrl = torch.tensor([5, 1, 2, 3, 4, 5, 0, 0], dtype=torch.int64)
    keep = ctrl.clone()
    P = ctypes.c_void_p(ctrl.data_ptr())
    for args, what in (((None, ad.T06, 1), "null pointer"), ((ctypes.c_void_p(ctrl.data_ptr() + 4), ad.T06, 1), "misaligned"),
                       ((P, -1, 1), "T24 = -1"), ((P, ad.ONE + 1, 1), "T24 = %d" % (ad.ONE + 1)), ((P, ad.T06, 0), "step24 < 1")):
        rc = lib.csg_ada_update_host(*args)
        assert rc != 0 and what in last_error(), (args, last_error())
    assert torch.equal(ctrl, keep)
    for words, what in (([-1, 1, 2, 0, 0, 0, 0, 0], "p24 = -1"), ([ad.ONE + 1, 1, 2, 0, 0, 0, 0, 0], "p24 = %d" % (ad.ONE + 1)),
                        ([5, 1, ad.MAX_COUNT, 0, 0, 0, 0, 0], "2^38")):
        bad = torch.tensor(words, dtype=torch.int64)
        rc = lib.csg_ada_update_host(ctypes.c_void_p(bad.data_ptr()), ad.T06, 1)
        assert rc != 0 and what in last_error(), (words, last_error())
        assert bad.tolist() == words
    gate = torch.full((4,), 9, dtype=torch.int32)
    G = ctypes.c_void_p(gate.data_ptr())
    for args, what in (((0, 0, 0, 0, 4, -1, G), "p24 = -1"), ((0, 0, 0, 0, 4, ad.ONE + 1, G), "p24 = "),
                       ((0, 0, 0, 0, 4, 5, None), "null pointer"), ((0, -1, 0, 0, 4, 5, G), "non-negative")):
        rc = lib.csg_augment_gate_host(*args)
        assert rc != 0 and what in last_error(), (args, last_error())
    assert (gate == 9).all()
    from canonicalsg2im_amd import ops
    with pytest.raises(RuntimeError, match="p24"):
        ops.augment_gate_host(0, 0, 0, 4, ad.ONE + 1)
    with pytest.raises(RuntimeError, match="step24"):
        ops.ada_update_host(ctrl, ad.T06, 0)
    with pytest.raises(RuntimeError, match="controller"):
        ops.ada_update_host(torch.zeros(7, dtype=torch.int64), ad.T06, 1)


# ------------------------------------------------------------------------------------------------ flags
def _parse(argv):
    from canonicalsg2im_amd.scripts.args import build_parser
    return build_parser().parse_args(argv)


def test_flags_default_to_not_given():
    from canonicalsg2im_amd.d_augment import ada_settings_of
    ns = _parse(["--d_augment", "color"])
    assert ns.d_augment_p is None and ns.d_augment_target is None and ns.d_augment_interval is None and ns.d_augment_kimg is None
    assert ada_settings_of(ns) is None
    import argparse
    assert ada_settings_of(argparse.Namespace()) is None             # a namespace from before the flags existed


def test_flags_parse():
    from canonicalsg2im_amd.d_augment import ada_settings_of
    s = ada_settings_of(_parse(["--d_augment", "color,cutout", "--d_augment_p", "0.25"]))
    assert s == {"p24": 1 << 22, "T24": 0, "interval": 4, "kimg": 500.0, "adaptive": False}
    s = ada_settings_of(_parse(["--d_augment", "color", "--d_augment_target", "0"]))
    assert s["p24"] == ad.ONE and not s["adaptive"]                  # a fixed p defaults to 1
    s = ada_settings_of(_parse(["--d_augment", "color", "--d_augment_target", "0.6"]))
    assert s == {"p24": 0, "T24": ad.T06, "interval": 4, "kimg": 500.0, "adaptive": True}      # adaptive: p starts at 0
    s = ada_settings_of(_parse(["--d_augment", "translation", "--d_augment_target", "0.6", "--d_augment_p", "1",
                                "--d_augment_interval", "2", "--d_augment_kimg", "0.008"]))
    assert s == {"p24": ad.ONE, "T24": ad.T06, "interval": 2, "kimg": 0.008, "adaptive": True}
    assert ada_settings_of(_parse(["--d_augment", "color", "--d_augment_interval", "8"]))["interval"] == 8


@pytest.mark.parametrize("argv, what", [
    (["--d_augment_p", "0.5"], "without --d_augment policies"),
    (["--d_augment_target", "0.6"], "without --d_augment policies"),
    (["--d_augment_interval", "4"], "without --d_augment policies"),
    (["--d_augment_kimg", "100"], "without --d_augment policies"),
    (["--d_augment", "", "--d_augment_p", "1"], "without --d_augment policies"),
    (["--d_augment", "color", "--d_augment_p", "1.5"], "--d_augment_p must be in [0, 1]"),
    (["--d_augment", "color", "--d_augment_p", "-0.1"], "--d_augment_p must be in [0, 1]"),
    (["--d_augment", "color", "--d_augment_p", "nan"], "--d_augment_p must be in [0, 1]"),
    (["--d_augment", "color", "--d_augment_target", "1"], "--d_augment_target must be 0 (a fixed p) or in (0, 1)"),
    (["--d_augment", "color", "--d_augment_target", "-0.5"], "--d_augment_target must be 0 (a fixed p) or in (0, 1)"),
    (["--d_augment", "color", "--d_augment_interval", "0"], "--d_augment_interval must be an integer >= 1"),
    (["--d_augment", "color", "--d_augment_kimg", "0"], "--d_augment_kimg must be a positive number"),
])
def test_flag_refusals(argv, what, capsys):
    with pytest.raises(SystemExit):
        _parse(argv)
    assert what in capsys.readouterr().err


def test_hand_built_settings_are_refused_too():
    from canonicalsg2im_amd.d_augment import ada_settings
    for kw, what in ((dict(p=0.5), "without --d_augment policies"), (dict(p=2.0, policies="color"), "d_augment_p"),
                     (dict(target=1.0, policies="color"), "d_augment_target"), (dict(interval=0, policies="color"), "interval"),
                     (dict(interval=2.5, policies="color"), "interval"), (dict(kimg=-1, policies="color"), "kimg"),
                     (dict(target=1e-9, policies="color"), "units of")):
        with pytest.raises(ValueError, match=what):
            ada_settings(**kw)


def test_step24():
    from canonicalsg2im_amd.d_augment import step24_of
    for (batch, world, K, M), want in ad.STEP24_VECTORS:
        m = M[0] / M[1] if isinstance(M, tuple) else M
        assert step24_of(batch, world, K, m) == want, (batch, world, K, M)


# ------------------------------------------------------------------------------------------------ DAugment without a device
def _cpu_aug(**kw):
    from canonicalsg2im_amd.d_augment import DAugment, ada_settings
    ada = ada_settings(policies="color", **kw)
    return DAugment("color", 0, "cpu", 4, 64, rank=0, ada=ada, world_size=2)


def test_step24_counts_the_pictures_of_one_iteration_once():
    """`batch_size` is per rank by default: 4 x 2 ranks = 8 pictures per iteration.  A caller whose --batch_size is the global
    batch (scripts.train) says so, and the step halves."""
    aug = _cpu_aug(target=0.6, interval=4, kimg=500.0)
    assert aug.pictures_per_iteration == 8 and aug.step24 == ad.step24(8, 1, 4, 500) == ad.step24(4, 2, 4, 500)
    aug.set_pictures_per_iteration(4)
    assert aug.pictures_per_iteration == 4 and aug.step24 == ad.step24(4, 1, 4, 500)


def test_the_sum_over_the_ranks_is_noted_in_an_audit_window():
    """`dist.comm_note` adds to fixed counters: the kind DAugment notes its (S, C) all-reduce under must be one of them."""
    import inspect
    from canonicalsg2im_amd import d_augment, dist as D
    assert 'comm_note("ada_allreduce", 16)' in inspect.getsource(d_augment.DAugment._reduce_counts)
    D.comm_reset()
    D.comm_note("ada_allreduce", 16)
    rep = D.comm_report(2)
    assert rep["ada_allreduce_calls_per_step"] == 0.5 and rep["ada_allreduce_bytes_per_step"] == 8.0


def test_load_meta_on_a_fixed_p_run_and_on_other_ranks(monkeypatch):
    """T = 0: this run's --d_augment_p holds whatever record the checkpoint carries.  Adaptive: the record continues; on a rank
    other than 0 the counts of the running interval start at 0 (the checkpoint holds rank 0's)."""
    from canonicalsg2im_amd import dist as D
    meta = {"seed": 0, "iteration": 5, "policies": "color", "ctrl": [123, 7, 9, 2, 3, 4, 0, 0],
            "ada": {"p24": 55, "T24": ad.T06, "interval": 4, "kimg": 500.0}}
    said = []
    fixed = _cpu_aug(p=0.25)
    fixed.load_meta(dict(meta), say=said.append)
    assert fixed.iteration == 5 and fixed.ctrl.tolist() == [1 << 22] + [0] * 7
    adaptive = _cpu_aug(target=0.6)
    adaptive.load_meta(dict(meta), say=said.append)
    assert adaptive.iteration == 5 and adaptive.ctrl.tolist() == [123, 7, 9, 2, 3, 4, 0, 0]
    monkeypatch.setattr(D, "rank", lambda: 1)
    other = _cpu_aug(target=0.6)
    other.load_meta(dict(meta), say=said.append)
    assert other.ctrl.tolist() == [123, 0, 0, 2, 3, 4, 0, 0]
