"""Adaptive strength of the discriminator augmentation on the device: the gate kernel against the host rows, the gated
transform against the ungated entry (gate of 7s), the input (gate of 0s) and the per-sample restatement of
tests/augment_cases.py (all 8 masks), the sign accumulation and the controller update against tests/ada_cases.py, the
library's refusals, and the flags inside the trainer: p = 1 is the ungated run, p = 0 is no augmentation, the adaptive run's
controller words after every update, replayed against eager steps, resume, an old checkpoint, raw validation, two ranks
(the tiny trainer on each, inside a communication audit window).

The trainer is the tiny one of tests/test_gpu_augment.py, with `--use_img_disc 1` wherever bits are compared between two
trainers (the object discriminator's crop backward has float atomics)."""
import copy
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

import ada_cases as ad
import augment_cases as ac

pytestmark = pytest.mark.gpu

TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "2", "--learning_rate", "5e-3"]
ALL = "color,translation,cutout"
PAD = 64
GATED_SHAPES = [(1, 2, 4, 0), (3, 4, 4, 0), (2, 8, 8, 5), (3, 16, 12, 8), (2, 17, 4, 0), (9, 256, 4, 0)]      # (N, H, Ct, c0)
SENT64 = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.detach().reshape(-1).view(torch.uint8), b.detach().reshape(-1).view(torch.uint8))


def _dev(a, cuda):
    """A numpy float32 / int32 array on the device with its bits intact."""
    return torch.from_numpy(a.view(np.int32).copy()).to(cuda).view(torch.float32 if a.dtype == np.float32 else torch.int32)


def _ctrl(cuda, words):
    """The eight words between two rows of sentinels: (the whole buffer, the record's view)."""
    buf = torch.full((24,), SENT64, dtype=torch.int64, device=cuda)
    buf[8:16] = torch.tensor([int(w) for w in words], dtype=torch.int64)
    return buf, buf[8:16]


def _ctrl_words(buf):
    raw = buf.cpu().tolist()
    assert raw[:8] == [SENT64] * 8 and raw[16:] == [SENT64] * 8, "a word outside the record was written"
    return raw[8:16]


# ------------------------------------------------------------------------------------------------ 1. the gate kernel
def test_gate_kernel_equals_the_host_rows(cuda):
    from canonicalsg2im_amd import ops
    for seed, iteration, pass_id, rank in ad.KEYS:
        for p24 in ad.P24_VALUES:
            buf, ctrl = _ctrl(cuda, [p24, 3, 4, 5, 6, 7, 0, 0])
            got = ops.augment_gate(seed, iteration, pass_id, 300, ctrl, rank=rank).cpu().numpy()
            want = ops.augment_gate_host(seed, iteration, pass_id, 300, p24, rank=rank).numpy()
            assert np.array_equal(got, want) and np.array_equal(got, ad.gate_np(seed, iteration, pass_id, rank, 300, p24))
            assert _ctrl_words(buf) == [p24, 3, 4, 5, 6, 7, 0, 0]                # read, never written
    out = torch.full((12,), 77, dtype=torch.int32, device=cuda)
    _, ctrl = _ctrl(cuda, [1 << 23, 0, 0, 0, 0, 0, 0, 0])
    ops.augment_gate(*ad.GATE_VECTORS_KEY[:3], 8, ctrl, rank=ad.GATE_VECTORS_KEY[3], out=out)
    assert out[:8].tolist() == ad.GATE_VECTORS and bool((out[8:] == 77).all())
    # a record whose p24 is outside [0, 2^24] cannot be refused by a launch that reads it on the device: clamped
    for word, mask in ((-5, 0), (1 << 40, 7)):
        _, ctrl = _ctrl(cuda, [word, 0, 0, 0, 0, 0, 0, 0])
        assert bool((ops.augment_gate(1, 2, 0, 70, ctrl) == mask).all())


# ------------------------------------------------------------------------------------------------ 2. the gated transform
def _launch(x, table, c0, policy, cuda, gate=None, bwd=False):
    """The C ABI entry — the gated one with `gate` (numpy int32, one mask per sample) — on a buffer of our own."""
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    N, H, _, Ct = x.shape
    xd, td = _dev(x, cuda), _dev(table, cuda)
    buf = torch.full((2 * PAD + x.size,), int(ac.SENTINEL), dtype=torch.int32, device=cuda)
    out = buf[PAD:PAD + x.size].view(torch.float32)
    nws = ac.workspace_bytes(N, H)
    ws = torch.empty(nws // 8 + 1, dtype=torch.float64, device=cuda)
    args = (ptr(xd), ptr(out), ptr(td), table.shape[0], N, H, Ct, c0, policy, ptr(ws), nws)
    if gate is None:
        check((lib.csg_augment_bwd if bwd else lib.csg_augment_fwd)(*args, stream()), "augment")
    else:
        gd = _dev(np.asarray(gate, np.int32), cuda)
        check((lib.csg_augment_bwd_gated if bwd else lib.csg_augment_fwd_gated)(*args, ptr(gd), stream()), "augment_gated")
    raw = buf.cpu().numpy()
    assert (raw[:PAD] == ac.SENTINEL).all() and (raw[PAD + x.size:] == ac.SENTINEL).all(), "a float outside the output was written"
    got = raw[PAD:PAD + x.size].view(np.float32).reshape(x.shape)
    assert not (got.view(np.int32) == ac.SENTINEL).any(), "an output float was not written"
    return got


def _table(shape, first=0):
    rows = ac.boundary_rows(shape[1])
    return np.stack([rows[(first + n) % len(rows)] for n in range(shape[0])])


@pytest.fixture(scope="module")
def ungated(cuda):
    """The ungated entry's output for every gated shape, policy and direction: computed once, compared against twice."""
    out = {}
    for shape in GATED_SHAPES:
        x, table = ac.data(shape, 300), _table(shape, 1)
        for policy in ac.ALL_POLICIES:
            for bwd in (False, True):
                out[shape, policy, bwd] = _launch(x, table, shape[3], policy, cuda, bwd=bwd)
    return out


@pytest.mark.parametrize("shape", GATED_SHAPES, ids=lambda s: "N%d_H%d_Ct%d_c%d" % s)
def test_gate_of_sevens_is_the_ungated_entry_and_gate_of_zeros_is_a_copy(shape, cuda, ungated):
    N, H, Ct, c0 = shape
    x, table = ac.data(shape, 300), _table(shape, 1)
    for policy in ac.ALL_POLICIES:
        for bwd in (False, True):
            on = _launch(x, table, c0, policy, cuda, gate=[7] * N, bwd=bwd)
            assert np.array_equal(on.view(np.int32), ungated[shape, policy, bwd].view(np.int32)), (shape, policy, bwd)
            # bits beyond the policies count for nothing: sample n runs policy & gate[n]
            on = _launch(x, table, c0, policy, cuda, gate=[-1] * N, bwd=bwd)
            assert np.array_equal(on.view(np.int32), ungated[shape, policy, bwd].view(np.int32)), (shape, policy, bwd)
            off = _launch(x, table, c0, policy, cuda, gate=[0] * N, bwd=bwd)
            assert np.array_equal(off.view(np.int32), x.view(np.int32)), (shape, policy, bwd)
            off = _launch(x, table, c0, policy, cuda, gate=[7 & ~policy] * N, bwd=bwd)
            assert np.array_equal(off.view(np.int32), x.view(np.int32)), (shape, policy, bwd)


def _restate_gated(fn, x, table, c0, policy, gate):
    parts = [fn(x[n:n + 1], table[n:n + 1], c0, policy & int(gate[n])) for n in range(x.shape[0])]
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))


@pytest.mark.parametrize("shape", GATED_SHAPES, ids=lambda s: "N%d_H%d_Ct%d_c%d" % s)
def test_all_eight_masks_equal_the_restatement(shape, cuda):
    """Hand-set gates that put all 8 masks on different samples (several launches where N < 8), every launch policy:
    sample n against the restatement called with policy & gate[n] — bits where the map copies or zeroes, the derived bound
    on the colour values.  In (3, 16, 12, 8) a block's 1024 float4 cover samples 0 and 1, whose gates differ."""
    N, H, Ct, c0 = shape
    worst = 0.0
    for policy in ac.ALL_POLICIES:
        for k in range(0, 8, N):
            gate = np.asarray([(k + n) % 8 for n in range(N)], np.int32)
            x, table = ac.data(shape, 400 + k), _table(shape, k)
            what = "shape %s policy %d gate %s" % (shape, policy, gate.tolist())
            ref, exact, L = _restate_gated(ac.restate_fwd, x, table, c0, policy, gate)
            got = _launch(x, table, c0, policy, cuda, gate=gate)
            worst = max(worst, ac.check_against(got, ref, exact, L, ac.FWD_ROUNDINGS, what + " forward"))
            ref, exact, L = _restate_gated(ac.restate_bwd, x, table, c0, policy, gate)
            got = _launch(x, table, c0, policy, cuda, gate=gate, bwd=True)
            worst = max(worst, ac.check_against(got, ref, exact, L, ac.BWD_ROUNDINGS, what + " backward"))
    print("%s: worst |device - restatement| / bound %.3f" % (shape, worst))
    assert worst <= 1.0


def test_nan_in_a_sample_that_is_gated_off_stays_there(cuda):
    shape = (3, 17, 8, 4)
    x, table = ac.data(shape, 9), _table(shape, 2)
    bad = x.copy()
    bad[1, 10, 1, 5] = np.nan
    bad[1, 16, 16, 6] = np.inf
    bad[2, 3, 3, 4] = np.nan
    gate = [7, 0, 6]                            # sample 1: everything off; sample 2: colour off, moved and cut
    for bwd in (False, True):
        a, b = _launch(x, table, 4, 7, cuda, gate=gate, bwd=bwd), _launch(bad, table, 4, 7, cuda, gate=gate, bwd=bwd)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)), "sample 0 changed with a NaN in samples 1 and 2"
        assert np.array_equal(b[1].view(np.int32), bad[1].view(np.int32)), "a sample that is gated off is not a bit copy"
        assert int(np.isnan(b[2]).sum()) <= 1, "with colour off a NaN is moved or cut, never spread"
        assert np.array_equal(np.isnan(a[2]), np.zeros_like(a[2], bool))


def test_two_gated_launches_give_the_same_bits(cuda):
    for shape in ((3, 16, 12, 8), (2, 17, 4, 0), (9, 256, 4, 0)):
        N, H, Ct, c0 = shape
        x, table, gate = ac.data(shape, 11), _table(shape), [(3 * n + 1) % 8 for n in range(N)]
        for bwd in (False, True):
            a, b = _launch(x, table, c0, 7, cuda, gate, bwd), _launch(x, table, c0, 7, cuda, gate, bwd)
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (shape, bwd)


def test_autograd_through_ops_with_a_gate(cuda):
    from canonicalsg2im_amd import ops
    for shape, policy in (((2, 8, 8, 5), 7), ((3, 16, 12, 8), 7), ((2, 17, 4, 0), 6)):
        N, H, Ct, c0 = shape
        table, gate = _table(shape, 3), np.asarray([(5 + 3 * n) % 8 for n in range(N)], np.int32)
        x, g = ac.data(shape, 21), ac.data(shape, 22)
        xd = _dev(x, cuda).permute(0, 3, 1, 2).requires_grad_(True)
        y = ops.d_augment(xd, _dev(table, cuda), c0, policy, gate=_dev(gate, cuda))
        assert y.shape == xd.shape and y.permute(0, 2, 3, 1).is_contiguous()
        y.backward(_dev(g, cuda).permute(0, 3, 1, 2))
        ref, exact, L = _restate_gated(ac.restate_fwd, x, table, c0, policy, gate)
        wf = ac.check_against(y.detach().permute(0, 2, 3, 1).cpu().numpy(), ref, exact, L, ac.FWD_ROUNDINGS, "autograd forward")
        ref, exact, L = _restate_gated(ac.restate_bwd, g, table, c0, policy, gate)
        assert xd.grad.shape == xd.shape
        wb = ac.check_against(xd.grad.permute(0, 2, 3, 1).contiguous().cpu().numpy(), ref, exact, L, ac.BWD_ROUNDINGS,
                              "autograd backward")
        assert wf <= 1.0 and wb <= 1.0
        # the C ABI entry gives the same bits, and without a gate the call is the ungated one
        assert np.array_equal(y.detach().permute(0, 2, 3, 1).cpu().numpy().view(np.int32),
                              _launch(x, table, c0, policy, cuda, gate=gate).view(np.int32))
        y0 = ops.d_augment(_dev(x, cuda).permute(0, 3, 1, 2), _dev(table, cuda), c0, policy)
        assert np.array_equal(y0.permute(0, 2, 3, 1).cpu().numpy().view(np.int32), _launch(x, table, c0, policy, cuda).view(np.int32))
    with pytest.raises(RuntimeError, match="gate"):
        ops.d_augment(xd, _dev(table, cuda), c0, policy, gate=torch.zeros(1, dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError, match="gate"):
        ops.d_augment(xd, _dev(table, cuda), c0, policy, gate=torch.zeros(N, dtype=torch.int64, device=cuda))


def test_library_refusals(cuda):
    from canonicalsg2im_amd._lib import HingeItem, last_error, lib, ptr, stream
    x = torch.zeros(2 * 4 * 4 * 8, device=cuda)
    sent = torch.full((2 * 4 * 4 * 8,), 3.0, device=cuda)
    table = torch.zeros((2, 8), dtype=torch.int32, device=cuda)
    gate = torch.full((4,), 7, dtype=torch.int32, device=cuda)
    ws = torch.zeros(64, dtype=torch.float64, device=cuda)
    off2 = ctypes.c_void_p(gate.data_ptr() + 2)
    for fn in (lib.csg_augment_fwd_gated, lib.csg_augment_bwd_gated):
        for g, what in ((None, "null pointer"), (off2, "misaligned")):
            rc = fn(ptr(x), ptr(sent), ptr(table), 2, 2, 4, 8, 5, 7, ptr(ws), 512, g, stream())
            assert rc != 0 and what in last_error(), (rc, last_error())
        for change, what in ((dict(c0=6), "c0 + 3 > Ct"), (dict(policy=8), "policy 8"), (dict(rows=1), "fewer than N = 2")):
            a = dict(dict(rows=2, c0=5, policy=7), **change)
            rc = fn(ptr(x), ptr(sent), ptr(table), a["rows"], 2, 4, 8, a["c0"], a["policy"], ptr(ws), 512, ptr(gate), stream())
            assert rc != 0 and what in last_error(), (change, last_error())
    buf, ctrl = _ctrl(cuda, [5, 1, 2, 3, 4, 5, 0, 0])
    off4 = ctypes.c_void_p(ctrl.data_ptr() + 4)
    for c, what in ((None, "null pointer"), (off4, "misaligned")):
        assert lib.csg_augment_gate(0, 0, 0, 0, 4, c, ptr(gate), stream()) != 0 and what in last_error()
        assert lib.csg_ada_update(c, ad.T06, 1, stream()) != 0 and what in last_error()
    assert lib.csg_augment_gate(0, 0, 0, 0, 4, ptr(ctrl), None, stream()) != 0 and "null pointer" in last_error()
    assert lib.csg_augment_gate(0, 0, 0, 0, 4, ptr(ctrl), off2, stream()) != 0 and "misaligned" in last_error()
    assert lib.csg_augment_gate(0, -1, 0, 0, 4, ptr(ctrl), ptr(gate), stream()) != 0 and "non-negative" in last_error()
    for T24, step24, what in ((-1, 1, "T24 = -1"), (ad.ONE + 1, 1, "T24 = "), (ad.T06, 0, "step24 < 1"), (ad.T06, -3, "step24 < 1")):
        assert lib.csg_ada_update(ptr(ctrl), T24, step24, stream()) != 0 and what in last_error()
    m = torch.ones((1, 1, 2, 3), device=cuda)
    item = (HingeItem * 1)()
    item[0].x, item[0].sb, item[0].sh, item[0].sw, item[0].B, item[0].H, item[0].W = m.data_ptr(), 6, 3, 1, 1, 2, 3
    for args, what in (((None, 1, ptr(ctrl)), "1..4 maps"), ((item, 0, ptr(ctrl)), "1..4 maps"), ((item, 5, ptr(ctrl)), "1..4 maps"),
                       ((item, 1, None), "null pointer"), ((item, 1, off4), "misaligned")):
        assert lib.csg_ada_accumulate(*args, stream()) != 0 and what in last_error(), (what, last_error())
    item[0].x = None
    assert lib.csg_ada_accumulate(item, 1, ptr(ctrl), stream()) != 0 and "bad map 0" in last_error()
    item[0].x, item[0].H = m.data_ptr(), 0
    assert lib.csg_ada_accumulate(item, 1, ptr(ctrl), stream()) != 0 and "bad map 0" in last_error()
    torch.cuda.synchronize()
    assert bool((sent == 3.0).all()) and bool((gate == 7).all())
    assert _ctrl_words(buf) == [5, 1, 2, 3, 4, 5, 0, 0]


# ------------------------------------------------------------------------------------------------ 3. signs and the update
def _maps_np(sizes, seed):
    return [ad.sign_map(n, seed + i) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("scales", [1, 4])
def test_accumulate_equals_the_restatement(cuda, scales):
    from canonicalsg2im_amd import ops
    for k, n in enumerate(ad.MAP_SIZES):
        sizes = [ad.MAP_SIZES[(k + 2 * i) % len(ad.MAP_SIZES)] for i in range(scales)]
        maps = _maps_np(sizes, 50 + k)
        S, C = ad.sign_count(maps)
        assert C == sum(sizes)
        buf, ctrl = _ctrl(cuda, [123, 5, 7, 9, -4, 11, 0, 0])
        dev = [_dev(m.reshape(-1), cuda).view(1, 1, 1, m.size) for m in maps]
        ops.ada_accumulate(dev, ctrl)
        assert _ctrl_words(buf) == [123, 5 + S, 7 + C, 9, -4, 11, 0, 0], (sizes, S, C)
        ops.ada_accumulate(dev, ctrl)                                         # two launches add up
        assert _ctrl_words(buf) == [123, 5 + 2 * S, 7 + 2 * C, 9, -4, 11, 0, 0], (sizes, S, C)


def test_accumulate_reads_strided_maps(cuda):
    """What the PatchGAN hands over: (B, 1, h, w) views of any strides — here channel 1 of a 3-channel NHWC tensor and a
    transposed map — and more than one block's worth of elements."""
    from canonicalsg2im_amd import ops
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, size=(2, 3, 5, 3)).astype(np.float32)             # (B, h, w, channels)
    b = rng.uniform(-0.5, 1, size=(2, 1, 37, 41)).astype(np.float32)
    c = rng.uniform(-1, 0.2, size=(3, 1, 64, 64)).astype(np.float32)         # 12 288 elements: 12 blocks
    ad_, bd, cd = (torch.from_numpy(t).to(cuda) for t in (a, b, c))
    views = [ad_.permute(0, 3, 1, 2)[:, 1:2], bd.transpose(2, 3), cd]
    S, C = ad.sign_count([a[..., 1], b, c])
    buf, ctrl = _ctrl(cuda, [0] * 8)
    ops.ada_accumulate(views, ctrl)
    assert _ctrl_words(buf) == [0, S, C, 0, 0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="map"):
        ops.ada_accumulate([ad_.permute(0, 3, 1, 2)], ctrl)                  # three channels
    with pytest.raises(RuntimeError, match="1..4"):
        ops.ada_accumulate([cd] * 5, ctrl)


def test_update_kernel_equals_the_host(cuda):
    from canonicalsg2im_amd import ops
    for (p24, S, C, T24, step24), want in ad.NEXT_P_TABLE:
        words = [p24, S, C, 41, -5, 9, 0, 0]
        host = torch.tensor(words, dtype=torch.int64)
        ops.ada_update_host(host, T24, step24)
        buf, ctrl = _ctrl(cuda, words)
        ops.ada_update(ctrl, T24, step24)
        got = _ctrl_words(buf)
        assert got == host.tolist() == ad.update_words(words, T24, step24) and got[0] == want, (p24, S, C, T24, step24, got)
    # words the host entry refuses: the device clamps p24 and leaves it alone at a count the products cannot hold
    buf, ctrl = _ctrl(cuda, [-7, 3, 4, 0, 0, 0, 0, 0])
    ops.ada_update(ctrl, ad.T06, 5)
    assert _ctrl_words(buf) == [5, 0, 0, 1, 3, 4, 0, 0]
    buf, ctrl = _ctrl(cuda, [9, ad.MAX_COUNT, ad.MAX_COUNT, 0, 0, 0, 0, 0])
    ops.ada_update(ctrl, ad.T06, 5)
    assert _ctrl_words(buf) == [9, 0, 0, 1, ad.MAX_COUNT, ad.MAX_COUNT, 0, 0]


# ------------------------------------------------------------------------------------------------ 4. the trainer
# a low target, so that the tiny discriminator's r_t (a few per cent either side of 0 in its first steps) crosses it
ADAPTIVE = ["--d_augment_target", "0.02", "--d_augment_interval", "2", "--d_augment_kimg", "0.008"]
T24 = 335544                                     # round(0.02 x 2^24) = round(335544.32)
STEP24 = 1 << 23                                 # 2 pictures x 1 rank x 2 iterations x 2^24 / (1000 x 0.008)
STEPS = 6


def _make(cuda, graphs, policies=ALL, flags=(), seed=0, extra=("--use_img_disc", "1")):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, TINY + list(extra) + ["--d_augment", policies] + list(flags))
    torch.manual_seed(seed)
    tr = T.Trainer(opt, cuda)
    if not graphs:
        tr.graphs = None
    else:
        assert tr.graphs is not None, "graph replay should be available for this recipe"
    return vocab, tr


def _batch(vocab, cuda, seed, B=2):
    from canonicalsg2im_amd.synth import BatchConfig, make_batch
    return [None if t is None else t.to(cuda) for t in make_batch(vocab, BatchConfig(B, 64, 2, 5, "packed"), seed)]


def _step(tr, batch, n):
    torch.manual_seed(1000 + n)
    G, D = tr.step(batch)
    return {k: v.clone() for k, v in G.items()}, {k: v.clone() for k, v in D.items()}


def _weights(tr):
    return [(n, p.detach().clone()) for n, p in list(tr.model.named_parameters()) + list(tr.discriminator.named_parameters())]


def _assert_same_run(a, b, what):
    assert len(a) == len(b)
    for n, ((Ga, Da), (Gb, Db)) in enumerate(zip(a, b), 1):
        assert list(Ga) == list(Gb) and list(Da) == list(Db)
        for k in list(Ga) + list(Da):
            x, y = (Ga[k], Gb[k]) if k in Ga else (Da[k], Db[k])
            assert _same_bits(x, y), "%s: %s of step %d: %r against %r" % (what, k, n, x.flatten()[:3].tolist(), y.flatten()[:3].tolist())


def _assert_same_weights(a, b, what):
    diff = [n for (n, x), (_, y) in zip(a, b) if not _same_bits(x, y)]
    assert not diff, "%s: %d tensors differ, e.g. %s" % (what, len(diff), diff[:3])


def test_p_one_is_the_ungated_run(cuda):
    """`--d_augment_p 1` (every gate is 7, the gated kernels) against the same run without the new flags, over an eager step,
    a capture + replay and a replay: the same losses and weights, bit for bit.  Without the flags nothing of this change
    exists: no record, no gate, today's graph key and checkpoint keys."""
    vocab, plain = _make(cuda, graphs=True)
    _, gated = _make(cuda, graphs=True, flags=["--d_augment_p", "1"])
    aug = gated.d_augment
    assert plain.d_augment.gated is False and plain.d_augment.ctrl is None and plain.d_augment.gates is None
    assert aug.gated and not aug.adaptive and aug.gates.shape == (3, 2) and aug.ctrl.tolist() == [ad.ONE] + [0] * 7
    batch = _batch(vocab, cuda, 90)
    assert len(plain.graphs.key_of(batch)) == 5 and gated.graphs.key_of(batch)[-2:] == (7, "gated")
    assert set(plain.checkpoint_dict()["d_augment"]) == {"seed", "iteration", "policies"}
    a = [_step(plain, batch, n) for n in (1, 2, 3)]
    b = [_step(gated, batch, n) for n in (1, 2, 3)]
    assert plain.graphs.replays == 2 and gated.graphs.replays == 2
    _assert_same_run(a, b, "p = 1 against the ungated run")
    _assert_same_weights(_weights(plain), _weights(gated), "p = 1 against the ungated run")
    assert bool((aug.gates == 7).all()) and aug.ctrl.tolist() == [ad.ONE] + [0] * 7           # a fixed p counts nothing


def test_p_zero_is_no_augmentation(cuda):
    """`--d_augment_p 0` on the eager path: every gate is 0, every sample a bit copy, so the discriminator's losses of step
    1 are those of a trainer without --d_augment, bit for bit."""
    vocab, off = _make(cuda, graphs=False, policies="")
    _, zero = _make(cuda, graphs=False, flags=["--d_augment_p", "0"])
    assert off.d_augment is None and zero.d_augment.gated
    batch = _batch(vocab, cuda, 91)
    (_, Da), (_, Db) = _step(off, batch, 1), _step(zero, batch, 1)
    assert bool((zero.d_augment.gates == 0).all()) and list(Da) == list(Db)
    for k in Da:
        assert _same_bits(Da[k], Db[k]), "%s: %r without --d_augment, %r with p = 0" % (k, float(Da[k]), float(Db[k]))
    _, one = _make(cuda, graphs=False, flags=["--d_augment_p", "1"])
    (_, Dc) = _step(one, batch, 1)
    assert not _same_bits(Da["D_img_real"], Dc["D_img_real"]), "p = 1 scored like no augmentation"


def _record(tr):
    """Clones of the prediction maps every `observe_real` call is handed, beside the call itself."""
    seen, inner = [], tr.d_augment.observe_real

    def observe(scales):
        seen.append([(s[-1] if isinstance(s, (list, tuple)) else s).detach().clone() for s in scales])
        return inner(scales)
    tr.d_augment.observe_real = observe
    return seen


@pytest.fixture(scope="module")
def adaptive_run(cuda):
    """Six eager steps of the adaptive recipe (K = 2, step24 = 2^23, p starts at 1/2); the record, the gates and the maps the
    signs were taken from after every step; a checkpoint after step 3."""
    vocab, tr = _make(cuda, graphs=False, flags=ADAPTIVE + ["--d_augment_p", "0.5"])
    aug = tr.d_augment
    assert aug.adaptive and aug.step24 == STEP24 and aug.ada["T24"] == T24 and aug.ctrl.tolist() == [1 << 23] + [0] * 7
    address = (aug.ctrl.data_ptr(), aug.gates.data_ptr())
    seen = _record(tr)
    batches = [_batch(vocab, cuda, 70 + i) for i in range(STEPS)]
    losses, words, gates, ck3 = [], [], [], None
    for n, b in enumerate(batches, 1):
        losses.append(_step(tr, b, n))
        words.append(aug.ctrl.tolist())
        gates.append(aug.gates.cpu().numpy().copy())
        if n == 3:
            ck3 = copy.deepcopy(tr.checkpoint_dict(3, 0))
    assert (aug.ctrl.data_ptr(), aug.gates.data_ptr()) == address
    assert len(seen) == STEPS, "the signs are taken once per step, on the real pass"
    return {"vocab": vocab, "batches": batches, "losses": losses, "words": words, "gates": gates, "ck3": ck3,
            "weights": _weights(tr), "seen": [[t.cpu().numpy() for t in s] for s in seen], "tr": tr}


def test_adaptive_controller_words(adaptive_run):
    """After every update p24 is `ada_next_p` of the reported (S_last, C_last); C_last is K x the element count of the
    prediction maps; (S, C) between updates are the restated signs of the maps the real pass returned; `updates` counts up;
    the gate arrays are the host gate at the record's p24."""
    from canonicalsg2im_amd import ops
    words, seen = adaptive_run["words"], adaptive_run["seen"]
    per_step = [ad.sign_count(maps) for maps in seen]
    count = per_step[0][1]
    assert count > 0 and all(c == count for _, c in per_step) and len(seen[0]) >= 1
    assert count == sum(int(np.prod(m.shape)) for m in seen[0])
    p24, updates = 1 << 23, 0
    S_last = C_last = 0
    for n in range(1, STEPS + 1):
        # begin_step of iteration n updates when n - 1 > 0 iterations are complete and (n - 1) % K == 0: before steps 3 and 5
        if n - 1 > 0 and (n - 1) % 2 == 0:
            S_last = per_step[n - 3][0] + per_step[n - 2][0]
            C_last = 2 * count
            p24 = ad.next_p(p24, S_last, C_last, T24, STEP24)
            updates += 1
            S, C = per_step[n - 1]
        elif n % 2 == 0:
            S, C = per_step[n - 2][0] + per_step[n - 1][0], 2 * count
        else:
            S, C = per_step[n - 1]
        print("step %d: words %s" % (n, words[n - 1]))
        assert words[n - 1] == [p24, S, C, updates, S_last, C_last, 0, 0], (n, words[n - 1])
        for p in range(3):
            assert np.array_equal(adaptive_run["gates"][n - 1][p], ops.augment_gate_host(0, n, p, 2, p24).numpy()), (n, p)
    assert updates == 2 and words[-1][3] == 2
    c = adaptive_run["tr"].d_augment.read()
    assert c["p24"] == p24 and c["p"] == p24 / ad.ONE and c["r_t"] == S_last / C_last and c["updates"] == 2


def test_adaptive_replayed_equals_eager(cuda, adaptive_run, monkeypatch):
    """The same six steps with graph replay (eager, capture + replay, four replays; the scene-graph encoder's own graph off,
    as in tests/test_gpu_augment.py's `encoder_eager`): the sign accumulation is captured inside S3 and adds to the record on
    every replay; the update and the gate fills run eagerly before it.  The same record after every step, the same losses,
    the same weights."""
    from canonicalsg2im_amd import graphs as csg_graphs
    monkeypatch.setattr(csg_graphs, "MAX_SG_GRAPHS", 0)
    _, tr = _make(cuda, graphs=True, flags=ADAPTIVE + ["--d_augment_p", "0.5"])
    assert tr.graphs.key_of(adaptive_run["batches"][0])[-2:] == (7, "adaptive")
    got, words = [], []
    for n, b in enumerate(adaptive_run["batches"], 1):
        got.append(_step(tr, b, n))
        words.append(tr.d_augment.ctrl.tolist())
    g = tr.graphs
    assert g.captures == 1 and g.replays == STEPS - 1 and g.eager_steps == 1
    assert words == adaptive_run["words"], (words, adaptive_run["words"])
    _assert_same_run(got, adaptive_run["losses"], "replayed against eager")
    _assert_same_weights(_weights(tr), adaptive_run["weights"], "replayed against eager")


def test_adaptive_resume(cuda, adaptive_run):
    """Saved after step 3 (between two updates: S and C are mid-count), loaded into a differently initialised trainer, three
    more steps: the record, the gates, the losses and the weights of the uninterrupted run."""
    ck3, batches = adaptive_run["ck3"], adaptive_run["batches"]
    assert ck3["d_augment"]["ctrl"] == adaptive_run["words"][2] and ck3["d_augment"]["iteration"] == 3
    assert ck3["d_augment"]["ada"] == {"p24": 1 << 23, "T24": T24, "interval": 2, "kimg": 0.008}
    _, tr = _make(cuda, graphs=False, flags=ADAPTIVE + ["--d_augment_p", "0.25"], seed=99)
    address = tr.d_augment.ctrl.data_ptr()
    assert tr.load_checkpoint(copy.deepcopy(ck3)) == (3, 0)
    assert tr.d_augment.ctrl.tolist() == adaptive_run["words"][2] and tr.d_augment.ctrl.data_ptr() == address
    got = []
    for n in (4, 5, 6):
        got.append(_step(tr, batches[n - 1], n))
        assert tr.d_augment.ctrl.tolist() == adaptive_run["words"][n - 1], n
        assert np.array_equal(tr.d_augment.gates.cpu().numpy(), adaptive_run["gates"][n - 1]), n
    _assert_same_run(got, adaptive_run["losses"][3:], "resumed against uninterrupted")
    _assert_same_weights(_weights(tr), adaptive_run["weights"], "resumed against uninterrupted")


def test_checkpoint_without_the_words_loads(cuda, adaptive_run):
    """A checkpoint of a run without the strength flags — `d_augment` = {seed, iteration, policies}, as before this feature —
    and one without the entry at all: the record starts from this run's flags."""
    vocab, old = _make(cuda, graphs=False)
    _step(old, adaptive_run["batches"][0], 1)
    ck = copy.deepcopy(old.checkpoint_dict(1, 0))
    assert ck["d_augment"] == {"seed": 0, "iteration": 1, "policies": ALL}
    _, tr = _make(cuda, graphs=False, flags=ADAPTIVE + ["--d_augment_p", "0.25"], seed=5)
    tr.d_augment.ctrl[1:3] = 17                       # whatever the record held, the load starts it again
    assert tr.load_checkpoint(copy.deepcopy(ck)) == (1, 0)
    assert tr.d_augment.iteration == 1 and tr.d_augment.ctrl.tolist() == [1 << 22] + [0] * 7
    tr.d_augment.ctrl[1:3] = 17
    tr.load_checkpoint({k: v for k, v in ck.items() if k != "d_augment"})
    assert tr.d_augment.iteration == 0 and tr.d_augment.ctrl.tolist() == [1 << 22] + [0] * 7
    _step(tr, adaptive_run["batches"][1], 1)
    assert tr.d_augment.ctrl.tolist()[2] > 0
    # and the other way round: an ungated run loads a gated run's checkpoint and stays ungated
    old.load_checkpoint(copy.deepcopy(adaptive_run["ck3"]))
    assert old.d_augment.iteration == 3 and old.d_augment.ctrl is None


def test_validation_is_raw_and_leaves_the_controller_alone(cuda):
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab, on = _make(cuda, graphs=False, flags=ADAPTIVE + ["--d_augment_p", "1"])
    _, off = _make(cuda, graphs=False, policies="")
    val = _batch(vocab, cuda, 61)
    before = on.d_augment.ctrl.tolist()
    a, _, _ = Evaluator(on).check_model([val], use_gt=True)
    b, _, _ = Evaluator(off).check_model([val], use_gt=True)
    assert set(a) == set(b) and on.d_augment.iteration == 0
    assert on.d_augment.ctrl.tolist() == before == [ad.ONE] + [0] * 7
    for k in a:
        assert _same_bits(a[k], b[k]), "%s: %r with the flags, %r without" % (k, float(a[k]), float(b[k]))


def test_crop_passes_are_gated_with_their_tables(cuda):
    """The default recipe (object discriminator on): every crop pass of a step fills a gate of one row per real object for
    THAT pass and iteration, at the record's p24."""
    from canonicalsg2im_amd import ops
    vocab, tr = _make(cuda, graphs=False, flags=["--d_augment_p", "0.5"], extra=())
    aug, asked = tr.d_augment, []
    fill = aug.crop_gate
    aug.crop_gate = lambda p, n: (asked.append((p, n, aug.iteration, fill(p, n).cpu().numpy())), fill(p, n))[1]
    batch = _batch(vocab, cuda, 78)
    _step(tr, batch, 1)
    img_idx, _ = tr.discriminator.obj_discriminator._object_index(batch[1])
    N = int(img_idx.numel())
    assert sorted(a[:3] for a in asked) == [(p, N, 1) for p in (3, 4, 5)], [a[:3] for a in asked]
    for p, n, it, g in asked:
        assert np.array_equal(g, ops.augment_gate_host(0, it, p, n, 1 << 23).numpy())


# ------------------------------------------------------------------------------------------------ 5. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ada_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from canonicalsg2im_amd import dist as D
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import BatchConfig, make_batch, make_vocab, shard_batch
    D.init_from_env(backend="gloo")
    dev = torch.device("cuda:0")
    vocab = make_vocab("tiny")
    # a global batch of 4, two pictures per rank, as scripts.train runs it: --batch_size is the global batch there
    base = list(TINY)
    del base[base.index("--batch_size"):base.index("--batch_size") + 2]
    argv = base + ["--batch_size", "4", "--gpu_ids", "0,1", "--use_img_disc", "1", "--d_augment", ALL, "--d_augment_p", "0.5"] + ADAPTIVE
    opt = T.make_opt(vocab, argv)
    torch.manual_seed(1234 + rank)
    tr = T.Trainer(opt, dev)
    aug = tr.d_augment
    before = aug.step24
    aug.set_pictures_per_iteration(4)
    seen = _record(tr)
    D.comm_reset()                               # an audit window, as bench.py --gpus N opens: every collective is noted
    words = []
    for n in (1, 2, 3):
        batch = make_batch(vocab, BatchConfig(4, 64, 2, 5, "packed"), seed=80 + n)
        mine = [None if t is None else t.cuda() for t in shard_batch(batch, rank, world)]
        torch.manual_seed(1000 + n)
        tr.step(mine)
        words.append(aug.ctrl.tolist())
    comm = D.comm_report(3)
    out[rank] = {"words": words, "counts": [ad.sign_count([t.cpu().numpy() for t in maps]) for maps in seen],
                 "gates": aug.gates.cpu().numpy(), "step24": (before, aug.step24), "rank": aug.rank, "read": aug.read(),
                 "ada_calls": comm["ada_allreduce_calls_per_step"], "ada_bytes": comm["ada_allreduce_bytes_per_step"],
                 "ckpt": tr.checkpoint_dict(3, 0)["d_augment"] if rank == 0 else None}
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_hold_the_same_p(cuda):
    """Two ranks on one GPU over gloo, in the manner of tests/test_gpu_ddp.py: the tiny trainer with the adaptive flags on
    each rank, three steps on its shard of the batch, inside a communication audit window.  Each rank counts the signs of
    its own real pass; at the top of step 3 (S, C) is summed over the ranks — one noted 16-byte all-reduce among the step's
    other collectives — so both ranks hold the same p24, the restatement's fed the summed counts, and draw their own gates
    (the rank is in the key) at that p24.  step24 counts the global batch once."""
    import torch.multiprocessing as mp
    from canonicalsg2im_amd import ops
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    out = mgr.dict()
    mp.spawn(_ada_worker, args=(world, port, out), nprocs=world, join=True)
    r0, r1 = out[0], out[1]
    # opt.batch_size x world_size = 8 pictures by default; scripts.train's correction to the 4 there are: 4 x 2 x 2^24 / 8
    assert r0["step24"] == r1["step24"] == (1 << 25, 1 << 24)
    assert (r0["rank"], r1["rank"]) == (0, 1)
    c0, c1 = r0["counts"], r1["counts"]
    assert len(c0) == len(c1) == 3 and c0[0][1] == c1[0][1] > 0
    assert [c[0] for c in c0] != [c[0] for c in c1], "the two ranks should count different signs"
    S = c0[0][0] + c0[1][0] + c1[0][0] + c1[1][0]
    C = c0[0][1] + c0[1][1] + c1[0][1] + c1[1][1]
    p24 = ad.next_p(1 << 23, S, C, T24, 1 << 24)
    for r, res, c in ((0, r0, c0), (1, r1, c1)):
        print("rank %d: words %s" % (r, res["words"]))
        assert res["words"][0] == [1 << 23, c[0][0], c[0][1], 0, 0, 0, 0, 0]
        assert res["words"][1] == [1 << 23, c[0][0] + c[1][0], c[0][1] + c[1][1], 0, 0, 0, 0, 0]
        assert res["words"][2] == [p24, c[2][0], c[2][1], 1, S, C, 0, 0], (r, res["words"][2], p24, S, C)
        for p in range(3):
            assert np.array_equal(res["gates"][p][:2], ops.augment_gate_host(0, 3, p, 2, p24, rank=r).numpy()), (r, p)
        assert res["read"]["p24"] == p24 and res["read"]["r_t"] == S / C
        assert res["ada_calls"] == 1 / 3 and res["ada_bytes"] == 16 / 3
    assert r0["words"][2][0] == r1["words"][2][0] == p24
    assert r0["ckpt"]["ctrl"] == r0["words"][2] and r0["ckpt"]["iteration"] == 3


def test_more_than_four_scales_are_refused_at_construction(cuda):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    opt = T.make_opt(make_vocab("tiny"), TINY + ["--use_img_disc", "1", "--num_D", "5", "--d_augment", ALL] + ADAPTIVE)
    with pytest.raises(ValueError, match="at most 4 PatchGAN scales"):
        T.Trainer(opt, cuda)
