"""DiffAugment on the device: the kernels against the restatement of tests/augment_cases.py on every row of its table — bits
where the map is a copy or a zero, the derived bound where means enter —, the table kernel against the numpy hash, the
library's refusals, and `--d_augment` inside the trainer: off-is-off, one transform for feature matching, seeds, replayed
against eager steps, resume, raw validation and raw display crops.

The trainer is the tiny one of tests/test_gpu_ema.py.  The tests that compare bits between two trainers run it with
`--use_img_disc 1`: the object discriminator's crop backward has the only float atomics of the path.  The crop passes are
exercised, eager and beside replayed graphs, by the last test, which compares no loss bits."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import augment_cases as ac

pytestmark = pytest.mark.gpu

TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "2", "--learning_rate", "5e-3"]
ALL = "color,translation,cutout"
PAD = 64                                         # sentinel floats on either side of an output buffer


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.detach().reshape(-1).view(torch.uint8), b.detach().reshape(-1).view(torch.uint8))


def _dev(a, cuda):
    """A numpy array on the device with its bits (NaN payloads, signed zeros) intact."""
    return torch.from_numpy(a.view(np.int32).copy()).to(cuda).view(torch.float32 if a.dtype == np.float32 else torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the kernels
def _launch(x, table, c0, policy, cuda, bwd=False):
    """The C ABI entry on a buffer of our own: (N, H, H, Ct) float32 numpy -> float32 numpy, with the sentinels around the
    output checked."""
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    N, H, _, Ct = x.shape
    xd, td = _dev(x, cuda), _dev(table, cuda)
    buf = torch.full((2 * PAD + x.size,), int(ac.SENTINEL), dtype=torch.int32, device=cuda)
    out = buf[PAD:PAD + x.size].view(torch.float32)
    nws = ac.workspace_bytes(N, H)
    ws = torch.empty(nws // 8 + 1, dtype=torch.float64, device=cuda)
    fn = lib.csg_augment_bwd if bwd else lib.csg_augment_fwd
    check(fn(ptr(xd), ptr(out), ptr(td), table.shape[0], N, H, Ct, c0, policy, ptr(ws), nws, stream()), "augment")
    raw = buf.cpu().numpy()
    assert (raw[:PAD] == ac.SENTINEL).all() and (raw[PAD + x.size:] == ac.SENTINEL).all(), "a float outside the output was written"
    got = raw[PAD:PAD + x.size].view(np.float32).reshape(x.shape)
    assert not (got.view(np.int32) == ac.SENTINEL).any(), "an output float was not written"
    return got


def _through_ops(x, table, c0, policy, cuda):
    from canonicalsg2im_amd import ops
    y = ops.d_augment(_dev(x, cuda).permute(0, 3, 1, 2), _dev(table, cuda), c0, policy)
    assert y.shape == (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) and y.permute(0, 2, 3, 1).is_contiguous()
    return y.permute(0, 2, 3, 1).cpu().numpy()


def _check_case(shape, policy, cuda, seed):
    """Every boundary row of the shape, N rows per launch: forward and backward against the restatement.  -> worst ratios"""
    N, H, Ct, c0 = shape
    rows = ac.boundary_rows(H)
    worst_f = worst_b = 0.0
    for k in range(0, len(rows), N):
        table = np.stack([rows[(k + n) % len(rows)] for n in range(N)])
        x = ac.data(shape, seed + k)
        what = "shape %s policy %d rows %d.." % (shape, policy, k)
        ref, exact, L = ac.restate_fwd(x, table, c0, policy)
        got = _launch(x, table, c0, policy, cuda)
        worst_f = max(worst_f, ac.check_against(got, ref, exact, L, ac.FWD_ROUNDINGS, what + " forward"))
        if k == 0:
            assert np.array_equal(_through_ops(x, table, c0, policy, cuda).view(np.int32), got.view(np.int32)), what
        ref, exact, L = ac.restate_bwd(x, table, c0, policy)
        got = _launch(x, table, c0, policy, cuda, bwd=True)
        worst_b = max(worst_b, ac.check_against(got, ref, exact, L, ac.BWD_ROUNDINGS, what + " backward"))
    return worst_f, worst_b


@pytest.mark.parametrize("shape", ac.SHAPES + ac.SPLIT_SHAPES, ids=lambda s: "N%d_H%d_Ct%d_c%d" % s)
def test_kernel_cases(shape, cuda):
    """All three policies on, tables written by hand: tx, ty in {-t, 0, t} in all combinations, cutout centres at 0, at
    H - 1 + (1 - size % 2) and in the middle, colour rows with s = 0, c = 0.5 and b = -0.5.  Translation and cutout move
    bits; the colour channels stay within ROUNDINGS * 2^-24 * L of the float64 restatement."""
    worst_f, worst_b = _check_case(shape, 7, cuda, seed=100)
    print("%s: worst |device - restatement| / bound: forward %.3f, backward %.3f" % (shape, worst_f, worst_b))
    assert worst_f <= 1.0 and worst_b <= 1.0


@pytest.mark.parametrize("policy", ac.ALL_POLICIES)
def test_policy_subsets(policy, cuda):
    """Each of the 7 non-empty sets: the restatement skips a disabled policy, and wherever it copies — with colour off that
    is every element — the device gives its bits."""
    worst = 0.0
    for shape in ((2, 8, 8, 5), (3, 16, 12, 8)):
        worst = max(worst, *_check_case(shape, policy, cuda, seed=200 + policy))
    print("policy %d: worst ratio %.3f" % (policy, worst))
    assert worst <= 1.0
    # said directly for the two moving policies: whatever the table holds, a policy that is off touches nothing
    shape = (2, 8, 8, 5)
    x, table = ac.data(shape, 5), ac.boundary_rows(8)[[0, 8]]
    got = _launch(x, table, 5, policy, cuda)
    if not policy & ac.COLOR:
        assert np.isin(got.view(np.int32), np.concatenate([x.view(np.int32).ravel(), [0]])).all()
    if policy == ac.COLOR:
        keep = [c for c in range(8) if not 5 <= c < 8]
        assert np.array_equal(got[..., keep].view(np.int32), x[..., keep].view(np.int32))


def test_non_finite_input_stays_in_its_sample(cuda):
    shape = (2, 17, 8, 4)
    x, table = ac.data(shape, 9), ac.boundary_rows(17)[[2, 6]]
    bad = x.copy()
    bad[1, 10, 1, 5] = np.nan                   # (outside sample 1's cutout, and a source of its shifted-back gradient)
    bad[1, 16, 16, 6] = np.inf
    for bwd in (False, True):
        a, b = _launch(x, table, 4, 7, cuda, bwd), _launch(bad, table, 4, 7, cuda, bwd)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)), "sample 0 changed with a NaN in sample 1"
        assert np.isnan(b[1]).any()


def test_two_launches_give_the_same_bits(cuda):
    for shape in ((2, 17, 4, 0), (2, 32, 40, 32), (9, 256, 4, 0)):
        N, H, Ct, c0 = shape
        rows = ac.boundary_rows(H)
        x, table = ac.data(shape, 11), np.stack([rows[n % len(rows)] for n in range(N)])
        for bwd in (False, True):
            a, b = _launch(x, table, c0, 7, cuda, bwd), _launch(x, table, c0, 7, cuda, bwd)
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (shape, bwd)


def test_table_kernel_equals_the_restatement(cuda):
    from canonicalsg2im_amd import ops
    for H, rows in ((2, 3), (32, 300), (64, 16), (256, 257)):
        for pass_id in range(6):
            for rank in (0, 1):
                got = ops.augment_table(12345, 7 + pass_id, pass_id, rows, H, rank=rank, device=cuda).cpu().numpy()
                assert np.array_equal(got, ac.table_np(12345, 7 + pass_id, pass_id, rank, rows, H)), (H, pass_id, rank)
    out = torch.full((5, 8), 77, dtype=torch.int32, device=cuda)
    ops.augment_table((1 << 64) - 1, 5, 4, 3, 16, rank=3, out=out)
    assert np.array_equal(out.cpu().numpy()[:3], np.asarray(ac.ROW_VECTORS)) and bool((out[3:] == 77).all())


def test_autograd_through_ops(cuda):
    from canonicalsg2im_amd import ops
    for shape, policy in (((2, 8, 8, 5), 7), ((3, 16, 12, 8), 7), ((2, 32, 40, 32), 5), ((2, 17, 4, 0), 6)):
        N, H, Ct, c0 = shape
        rows = ac.boundary_rows(H)
        table = np.stack([rows[(3 + 2 * n) % len(rows)] for n in range(N)])
        x, g = ac.data(shape, 21), ac.data(shape, 22)
        xd = _dev(x, cuda).permute(0, 3, 1, 2).requires_grad_(True)
        y = ops.d_augment(xd, _dev(table, cuda), c0, policy)
        y.backward(_dev(g, cuda).permute(0, 3, 1, 2))
        ref, exact, L = ac.restate_fwd(x, table, c0, policy)
        wf = ac.check_against(y.detach().permute(0, 2, 3, 1).cpu().numpy(), ref, exact, L, ac.FWD_ROUNDINGS, "autograd forward %s" % (shape,))
        ref, exact, L = ac.restate_bwd(g, table, c0, policy)
        assert xd.grad.shape == xd.shape
        wb = ac.check_against(xd.grad.permute(0, 2, 3, 1).contiguous().cpu().numpy(), ref, exact, L, ac.BWD_ROUNDINGS,
                              "autograd backward %s" % (shape,))
        print("%s policy %d: forward %.3f backward %.3f of the bound" % (shape, policy, wf, wb))
        assert wf <= 1.0 and wb <= 1.0


def test_autograd_runs_each_kinds_own_adjoint(cuda):
    """DiffAugment, gated DiffAugment and the ADA pipeline go through one autograd Function: for each kind the gradient that
    autograd returns is, bit for bit, what the kind's own _bwd entry gives on the same upstream gradient with the operands
    the forward was called with.  N = 3, Ct = 8, H = 5, c0 = 4: an odd side (the translation wraps, the cutout clips), 25
    pixels (a partial chunk), colour channels in the second float4.  Tables of seed 1, passes 0, 1 and 2 (one per kind, so a
    kind that saved another's table shows), gate and ADA rows at p24 = 2^23, ADA policy 56.  ITERATION 2, not 1: at
    iteration 1 the gate of pass 1 is [3, 4, 3], no row fully off; at iteration 2 it is [0, 1, 4] (asserted below)."""
    from canonicalsg2im_amd import ops
    from canonicalsg2im_amd._lib import check, lib, ptr, stream
    N, Ct, H, c0, seed, it, p24 = 3, 8, 5, 4, 1, 2, 1 << 23
    gate_h = ops.augment_gate_host(seed, it, 1, N, p24)
    ada_h = ops.ada_pipeline_table_host(seed, it, 2, N, H, 56, p24)
    assert bool((gate_h == 0).any()) and bool((gate_h != 0).any()), gate_h.tolist()
    identity = ops.ADA_GEOM_ID | ops.ADA_COLOR_ID
    assert bool(((ada_h[:, 13] & identity) != identity).any()), ada_h[:, 13].tolist()
    tables = [ops.augment_table_host(seed, it, p, N, H).to(cuda) for p in (0, 1)]
    gate, ada_table = gate_h.to(cuda), ada_h.to(cuda)
    torch.manual_seed(31)
    x = ops.empty_nhwc(N, Ct, H, H, cuda).normal_().requires_grad_(True)
    g = ops.empty_nhwc(N, Ct, H, H, cuda).normal_()
    nws = int(lib.csg_augment_workspace_bytes(N, H))
    ws = torch.empty(nws // 8 + 1, dtype=torch.float64, device=cuda)
    head = lambda out, table: (ptr(g), ptr(out), ptr(table), N, N, H, Ct, c0)
    kinds = (("d_augment", lambda: ops.d_augment(x, tables[0], c0, 7),
              lambda out: lib.csg_augment_bwd(*head(out, tables[0]), 7, ptr(ws), nws, stream())),
             ("d_augment, gated", lambda: ops.d_augment(x, tables[1], c0, 7, gate=gate),
              lambda out: lib.csg_augment_bwd_gated(*head(out, tables[1]), 7, ptr(ws), nws, ptr(gate), stream())),
             ("ada_pipeline", lambda: ops.ada_pipeline(x, ada_table, c0),
              lambda out: lib.csg_ada_pipeline_bwd(*head(out, ada_table), stream())))
    grads = []
    for name, forward, adjoint in kinds:
        (gx,) = torch.autograd.grad(forward(), x, g)
        want = ops.empty_nhwc(N, Ct, H, H, cuda)
        check(adjoint(want), name)
        assert gx.shape == x.shape and _same_bits(gx, want), name
        grads.append(gx)
    assert not _same_bits(grads[0], grads[1]) and not _same_bits(grads[0], grads[2]) and not _same_bits(grads[1], grads[2])


def test_library_refusals(cuda):
    from canonicalsg2im_amd._lib import last_error, lib, ptr, stream
    x = torch.zeros(2 * 4 * 4 * 8, device=cuda)
    sent = torch.full((2 * 4 * 4 * 8,), 3.0, device=cuda)
    table = torch.zeros((2, 8), dtype=torch.int32, device=cuda)
    ws = torch.zeros(64, dtype=torch.float64, device=cuda)
    good = dict(table_rows=2, N=2, H=4, Ct=8, c0=5, policy=7)
    for change, what in ((dict(c0=6), "c0 + 3 > Ct"), (dict(Ct=6), "multiple of 4"), (dict(H=1), "H = 1"),
                         (dict(table_rows=1), "fewer than N = 2"), (dict(policy=8), "policy 8")):
        a = dict(good, **change)
        for fn in (lib.csg_augment_fwd, lib.csg_augment_bwd):
            rc = fn(ptr(x), ptr(sent), ptr(table), a["table_rows"], a["N"], a["H"], a["Ct"], a["c0"], a["policy"], ptr(ws), 512, stream())
            assert rc != 0 and what in last_error(), (change, rc, last_error())
    rc = lib.csg_augment_fwd(ptr(x), ptr(x), ptr(table), 2, 2, 4, 8, 5, 7, ptr(ws), 512, stream())
    assert rc != 0 and "not in place" in last_error()
    rc = lib.csg_augment_fwd(ptr(x), ptr(sent), ptr(table), 2, 2, 4, 8, 5, 7, ptr(ws), 8, stream())
    assert rc != 0 and "workspace" in last_error()
    torch.cuda.synchronize()
    assert bool((sent == 3.0).all())


# ------------------------------------------------------------------------------------------------ 2. the trainer
def _make(cuda, graphs, policies=ALL, aug_seed=0, seed=0, strip=False, extra=("--use_img_disc", "1")):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, TINY + list(extra) + ["--d_augment", policies, "--d_augment_seed", str(aug_seed)])
    if strip:                                     # a namespace from before the flags existed
        del opt.d_augment, opt.d_augment_seed
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
    torch.manual_seed(1000 + n)                   # whatever a step draws, it draws the same in every trainer
    G, D = tr.step(batch)
    return {k: v.clone() for k, v in G.items()}, {k: v.clone() for k, v in D.items()}


def _weights(tr):
    return [(n, p.detach().clone()) for n, p in list(tr.model.named_parameters()) + list(tr.discriminator.named_parameters())]


def _assert_same_run(a, b, what):
    """Two lists of (G, D) loss dictionaries: the same keys and the same bits."""
    assert len(a) == len(b)
    for n, ((Ga, Da), (Gb, Db)) in enumerate(zip(a, b), 1):
        assert list(Ga) == list(Gb) and list(Da) == list(Db)
        for k in list(Ga) + list(Da):
            x, y = (Ga[k], Gb[k]) if k in Ga else (Da[k], Db[k])
            assert _same_bits(x, y), "%s: %s of step %d: %r against %r" % (what, k, n, x.flatten()[:3].tolist(), y.flatten()[:3].tolist())


def _assert_same_weights(a, b, what):
    diff = [n for (n, x), (_, y) in zip(a, b) if not _same_bits(x, y)]
    assert not diff, "%s: %d tensors differ, e.g. %s" % (what, len(diff), diff[:3])


@pytest.fixture(scope="module")
def eager_run(cuda):
    """Four eager steps with all three policies on; a checkpoint after step 2."""
    vocab, tr = _make(cuda, graphs=False)
    assert tr.d_augment is not None and tr.d_augment.policy == 7 and tr.d_augment.tables.shape == (3, 2, 8)
    address = tr.d_augment.tables.data_ptr()
    batches = [_batch(vocab, cuda, 70 + i) for i in range(4)]
    losses, ck2 = [], None
    for n, b in enumerate(batches, 1):
        losses.append(_step(tr, b, n))
        assert tr.d_augment.iteration == n and not tr.d_augment.active
        for p in range(3):                        # the persistent tables hold this iteration's rows, where they always were
            assert np.array_equal(tr.d_augment.tables[p].cpu().numpy(), ac.table_np(0, n, p, 0, 2, 64))
        if n == 2:
            ck2 = copy.deepcopy(tr.checkpoint_dict(2, 0))
    assert tr.d_augment.tables.data_ptr() == address and tr._eager_steps == 4
    return {"vocab": vocab, "batches": batches, "losses": losses, "ck2": ck2, "weights": _weights(tr), "tr": tr}


def test_off_is_off(cuda):
    """Three steps (eager, capture + replay, replay) without the flag against a trainer whose namespace has no d_augment
    attribute at all: the same losses and the same weights, bit for bit; no object, today's checkpoint keys."""
    vocab, old = _make(cuda, graphs=True, strip=True)
    _, off = _make(cuda, graphs=True, policies="")
    assert not hasattr(old.opt, "d_augment") and old.d_augment is None and off.d_augment is None
    assert off.discriminator.img_discriminator.d_augment is None
    batch = _batch(vocab, cuda, 90)
    a = [_step(old, batch, n) for n in (1, 2, 3)]
    b = [_step(off, batch, n) for n in (1, 2, 3)]
    _assert_same_run(a, b, "off against a namespace without the flags")
    _assert_same_weights(_weights(old), _weights(off), "off against a namespace without the flags")
    assert set(off.checkpoint_dict()) == set(old.checkpoint_dict()) and "d_augment" not in off.checkpoint_dict()
    assert old.graphs.replays == 2 and off.graphs.replays == 2
    assert len(old.graphs.key_of(batch)) == len(off.graphs.key_of(batch)) == 4


def test_feature_matching_sees_one_transform(cuda):
    """imgs_pred := imgs with all three policies on: the generator update's two PatchGAN passes read the same table, so the
    feature-matching distance is exactly 0.  The discriminator is in eval mode here: a training-mode pass advances the
    spectral-norm vectors, and the second pass would run on other weights whatever the inputs.  The same two pictures
    through tables 0 and 1 differ: a transform keyed per call would not give 0."""
    vocab, tr = _make(cuda, graphs=False)
    imgs, objs, boxes = _batch(vocab, cuda, 75)[:3]
    tr.discriminator.eval()
    gm, aug = tr.gans_model, tr.d_augment
    with torch.no_grad():
        raw = gm.generator_image_terms(imgs, objs, boxes, None, imgs)
        aug.begin_step()
        try:
            terms = gm.generator_image_terms(imgs, objs, boxes, None, imgs)
            f0 = gm.netD_img(imgs, objs, boxes, aug_pass=0)
            f1 = gm.netD_img(imgs, objs, boxes, aug_pass=1)
        finally:
            aug.end_step()
        after = gm.generator_image_terms(imgs, objs, boxes, None, imgs)
    assert float(terms["GAN_Feat"]) == 0.0, float(terms["GAN_Feat"])
    assert not _same_bits(terms["GAN_Img"], raw["GAN_Img"]), "the augmented pass scored like the raw one"
    assert not _same_bits(f0[0][0], f1[0][0]), "tables 0 and 1 gave the same features"
    assert _same_bits(after["GAN_Img"], raw["GAN_Img"]) and float(raw["GAN_Feat"]) == 0.0        # raw outside a step


def test_same_seed_same_bits_other_seed_other_transforms(cuda, eager_run):
    batches = eager_run["batches"]
    _, same = _make(cuda, graphs=False)
    _, other = _make(cuda, graphs=False, aug_seed=1)
    a = [_step(same, b, n) for n, b in enumerate(batches[:3], 1)]
    _assert_same_run(a, eager_run["losses"][:3], "two trainers with the same seed")
    c = [_step(other, b, n) for n, b in enumerate(batches[:3], 1)]
    assert all(not _same_bits(x[1]["D_img_real"], y[1]["D_img_real"]) for x, y in zip(a, c)), "another seed, the same D_img_real"


@pytest.mark.parametrize("encoder_graph", [True, False], ids=["default", "encoder_eager"])
def test_replayed_equals_eager(cuda, eager_run, monkeypatch, encoder_graph):
    """Four steps with graph replay (eager, capture + replay, two replays: the captured PatchGAN passes read the persistent
    tables, refilled before every replay) against the four eager steps, bit for bit.

    `default` is the trainer as it ships.  Its scene-graph encoder has a graph of its own (S0 of graphs.py), first replayed
    in step 4; S0 pads the triplet rows to a multiple of 64, so the encoder's sums round in another order there
    (tests/test_gpu_graphs.py::test_graph_replay_matches_eager holds that path to a tolerance).  The encoder sees neither
    discriminator nor anything the augmentation touches.  Compared: every term of steps 1-3, every term of step 4 but
    `bbox_pred_all` (1.62977469 replayed against 1.62977481 eager), and every weight but the encoder's.
    `encoder_eager` switches S0 off, so the encoder runs eagerly between the replays: every term of all four steps and every
    weight."""
    from canonicalsg2im_amd import graphs as csg_graphs
    if not encoder_graph:
        monkeypatch.setattr(csg_graphs, "MAX_SG_GRAPHS", 0)
    _, tr = _make(cuda, graphs=True)
    assert len(tr.graphs.key_of(eager_run["batches"][0])) == 5 and tr.graphs.key_of(eager_run["batches"][0])[-1] == 7
    got = [_step(tr, b, n) for n, b in enumerate(eager_run["batches"], 1)]
    g = tr.graphs
    print("captures %d replays %d eager %d encoder replays %d" % (g.captures, g.replays, g.eager_steps, g.sg_replays))
    assert g.captures == 1 and g.replays == 3 and g.eager_steps == 1
    assert g.sg_replays == (1 if encoder_graph else 0)
    want = eager_run["losses"]
    for n, ((Ga, Da), (Gb, Db)) in enumerate(zip(got, want), 1):
        for k in list(Ga) + list(Da):
            x, y = (Ga[k], Gb[k]) if k in Ga else (Da[k], Db[k])
            print("step %d %-16s replayed %.9g eager %.9g" % (n, k, float(x.flatten()[0]), float(y.flatten()[0])))
    weights, eager_weights = _weights(tr), eager_run["weights"]
    if encoder_graph:
        drop = lambda G: {k: v for k, v in G.items() if k != "bbox_pred_all"}
        assert "bbox_pred_all" in got[3][0]
        got = got[:3] + [(drop(got[3][0]), got[3][1])]
        want = want[:3] + [(drop(want[3][0]), want[3][1])]
        encoder = {"sg_to_layout." + n for n, _ in tr.model.sg_to_layout.named_parameters()}
        assert encoder and encoder < {n for n, _ in weights}
        weights = [(n, p) for n, p in weights if n not in encoder]
        eager_weights = [(n, p) for n, p in eager_weights if n not in encoder]
    _assert_same_run(got, want, "replayed against eager")
    _assert_same_weights(weights, eager_weights, "replayed against eager")


def test_resume(cuda, eager_run, capsys):
    """Saved after step 2, loaded into a differently initialised trainer, two more steps: the bits of the uninterrupted run.
    A checkpoint without the entry starts at iteration 0; one with other policies or another seed is loaded with one line."""
    ck2, batches = eager_run["ck2"], eager_run["batches"]
    assert ck2["d_augment"] == {"seed": 0, "iteration": 2, "policies": ALL}
    _, tr = _make(cuda, graphs=False, seed=99)
    capsys.readouterr()
    assert tr.load_checkpoint(copy.deepcopy(ck2)) == (2, 0)
    assert tr.d_augment.iteration == 2 and "d_augment" not in capsys.readouterr().out
    got = [_step(tr, batches[n - 1], n) for n in (3, 4)]
    _assert_same_run(got, eager_run["losses"][2:], "resumed against uninterrupted")
    _assert_same_weights(_weights(tr), eager_run["weights"], "resumed against uninterrupted")
    bare = {k: v for k, v in copy.deepcopy(ck2).items() if k != "d_augment"}
    tr.load_checkpoint(bare)
    assert tr.d_augment.iteration == 0
    _, other = _make(cuda, graphs=False, policies="cutout", aug_seed=3)
    capsys.readouterr()
    other.load_checkpoint(copy.deepcopy(ck2))
    out = capsys.readouterr().out
    assert other.d_augment.iteration == 2 and other.d_augment.policy == 4 and other.d_augment.seed == 3
    assert out.count("\n") == 1 and "d_augment" in out and "'cutout'" in out and "seed 3" in out, out


def test_validation_is_raw(cuda):
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab, on = _make(cuda, graphs=False)
    _, off = _make(cuda, graphs=False, policies="")
    val = _batch(vocab, cuda, 61)
    a, _, _ = Evaluator(on).check_model([val], use_gt=True)
    b, _, _ = Evaluator(off).check_model([val], use_gt=True)
    assert set(a) == set(b) and on.d_augment.iteration == 0
    for k in a:
        assert _same_bits(a[k], b[k]), "%s: %r with the flag, %r without" % (k, float(a[k]), float(b[k]))


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "replayed"])
def test_display_crops_are_raw_and_the_crop_passes_are_keyed(cuda, graphs):
    """The default recipe (object discriminator on), three steps — eager; or eager, capture + replay, replay, where the
    object-crop part stays eager beside the replayed graphs.  In every step the crop tables are filled for passes 3, 4 and 5
    of THAT iteration with one row per real object, and the crops kept for display are what ops.crop_objects gives, bit for
    bit.  (No loss bits are compared: the crop backward has float atomics.)"""
    from canonicalsg2im_amd import ops
    vocab, tr = _make(cuda, graphs=graphs, extra=())
    asked = []
    fill = tr.d_augment.crop_table
    tr.d_augment.crop_table = lambda p, n, size: (asked.append((p, n, size, tr.d_augment.iteration)), fill(p, n, size))[1]
    D = tr.discriminator.obj_discriminator
    for it in (1, 2, 3):
        batch = _batch(vocab, cuda, 77 + it)
        imgs, objs, boxes = batch[:3]
        del asked[:]
        _step(tr, batch, it)
        img_idx, obj_idx = D._object_index(objs)
        want = ops.crop_objects(imgs, boxes[img_idx, obj_idx], img_idx, D.object_size)[:, :3]
        assert _same_bits(tr.gans_model.d_real_crops.contiguous(), want.contiguous()), "step %d: the display crops are not raw" % it
        N = int(img_idx.numel())
        assert sorted(asked) == [(p, N, D.object_size, it) for p in (3, 4, 5)], (it, asked)
    if graphs:
        assert tr.graphs.captures == 1 and tr.graphs.replays == 2 and tr.graphs.eager_steps == 1
