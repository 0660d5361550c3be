"""The weight EMA on the device: the kernel against the float64 restatement of tests/ema_cases.py on every row of its table,
the wrapper's refusals, and `WeightEMA` inside the trainer — eager and replayed steps, resume, off-is-off, the sampler and
the swap with its cache invalidation.

The trainer is the tiny one of tests/test_gpu_update_rule.py with `--use_img_disc 1`: without the object discriminator there
are no float atomics on the path (its crop backward has the only ones), so two trainers built from one seed and fed the same
batches hold the same bits, which the resume, off-is-off and swap tests compare.  The learning rate is raised to 5e-3 so
that four steps move the weights far enough for the averaged and the raw pictures to differ in their bytes."""
import copy

import numpy as np
import pytest
import torch

import ema_cases as ec

pytestmark = pytest.mark.gpu

TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss", "--batch_size", "2", "--use_img_disc", "1",
        "--learning_rate", "5e-3"]
DECAY = 0.999


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _same_bits(a, b):
    """Equal as bytes (NaNs and signed zeros included), for any dtype and layout."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.detach().reshape(-1).view(torch.uint8), b.detach().reshape(-1).view(torch.uint8))


# ------------------------------------------------------------------------------------------------ 1. the kernel, row by row
TAIL = 8                                        # sentinel floats behind the last slot


def _device_case(case, cuda):
    """-> (host [(p, e, kind)], sources on the device, the table, over a shadow full of sentinels with e in the slots)."""
    from canonicalsg2im_amd import ops
    host = ec.make(case)
    srcs = [torch.from_numpy(p.view(np.int32).copy()).to(cuda).view(torch.float32) for p, _, _ in host]
    offs, floats = ops.ema_layout([p.size for p, _, _ in host])
    shadow = torch.full((floats + TAIL,), int(ec.SENTINEL), dtype=torch.int32, device=cuda)
    for (p, e, _), o in zip(host, offs):
        shadow[o:o + e.size] = torch.from_numpy(e.view(np.int32).copy()).to(cuda)
    table = ops.EmaTable(srcs, [k for _, _, k in host], shadow=shadow.view(torch.float32))
    assert table.offsets == offs and table.shadow.data_ptr() == shadow.data_ptr()
    return host, srcs, table, shadow


def _slots(shadow, table):
    """(per-item int32 arrays, the int32 array of everything outside the slots) of the shadow, on the host."""
    raw = shadow.cpu().numpy()
    outside = np.ones(raw.size, dtype=bool)
    out = []
    for o, n in zip(table.offsets, table.numels):
        out.append(raw[o:o + n].copy())
        outside[o:o + n] = False
    return out, raw[outside]


def test_kernel_rows(cuda):
    from canonicalsg2im_amd import ops
    worst = 0.0
    for case in ec.table():
        host, srcs, table, shadow = _device_case(case, cuda)
        d, omd = ec.scalars(case["decay"])
        assert (d, omd) == ops.ema_scalars(case["decay"])
        npad = shadow.numel() - sum(table.numels)
        # ---- UPDATE
        ops.ema_update(table, case["decay"])
        got, outside = _slots(shadow, table)
        assert outside.size == npad >= TAIL and (outside == ec.SENTINEL).all(), "%s: a float outside the slots was written" % case["name"]
        for j, ((p, e, kind), g, s) in enumerate(zip(host, got, srcs)):
            what = "%s item %d" % (case["name"], j)
            assert np.array_equal(s.cpu().numpy().view(np.int32), p.view(np.int32)), what + ": UPDATE wrote a source"
            exact, ref = ec.restate(p, e, kind, d, omd)
            if exact:                                           # COPY items, and D = 1: equal as bits
                assert np.array_equal(g, ref.view(np.int32)), what
            else:
                worst = max(worst, ec.check_average(g.view(np.float32), ref, ec.step_bound(p, e, ref, d, omd), what))
        # ---- SWAP: bit for bit, twice is the identity, nothing outside the slots
        ops.ema_swap(table)
        swapped, outside = _slots(shadow, table)
        assert (outside == ec.SENTINEL).all()
        for j, ((p, _, _), g, sw, s) in enumerate(zip(host, got, swapped, srcs)):
            assert np.array_equal(sw, p.view(np.int32)), "%s item %d: the slot after SWAP is not the source" % (case["name"], j)
            assert np.array_equal(s.cpu().numpy().view(np.int32), g), "%s item %d: the source after SWAP is not the slot" % (
                case["name"], j)
        ops.ema_swap(table)
        again, outside = _slots(shadow, table)
        assert (outside == ec.SENTINEL).all()
        for j, ((p, _, _), g, a, s) in enumerate(zip(host, got, again, srcs)):
            assert np.array_equal(a, g) and np.array_equal(s.cpu().numpy().view(np.int32), p.view(np.int32)), \
                "%s item %d: SWAP twice is not the identity" % (case["name"], j)
        # ---- FILL: every slot = its source, whatever the kind
        ops.ema_fill(table)
        filled, outside = _slots(shadow, table)
        assert (outside == ec.SENTINEL).all()
        for j, ((p, _, _), f) in enumerate(zip(host, filled)):
            assert np.array_equal(f, p.view(np.int32)), "%s item %d: FILL" % (case["name"], j)
    print("worst |device - restatement| / bound over the table: %.3f" % worst)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_refusals(cuda):
    """A misaligned, a non-contiguous and a non-fp32 source are refused with a message when the table is made: nothing is
    launched, the shadow keeps its bits.  So are a host tensor, a shadow too small and a decay out of range."""
    from canonicalsg2im_amd import ops
    good = torch.randn(64, device=cuda)
    base = torch.randn(65, device=cuda)
    grid = torch.randn(8, 8, device=cuda)
    shadow = torch.full((256,), int(ec.SENTINEL), dtype=torch.int32, device=cuda)
    before = shadow.clone()
    for bad, msg in ((base[1:], "16-byte aligned"), (grid.t(), "not contiguous"), (grid[:, ::2], "not contiguous"),
                     (torch.randn(64, device=cuda, dtype=torch.float64), "fp32"),
                     (torch.zeros(64, device=cuda, dtype=torch.int32), "fp32"), (torch.randn(64), "no CPU path")):
        with pytest.raises(RuntimeError, match=msg):
            ops.EmaTable([good, bad], [ops.EMA_AVERAGE, ops.EMA_COPY], shadow=shadow.view(torch.float32))
    with pytest.raises(RuntimeError, match="at least 128 floats"):
        ops.EmaTable([good, good.clone()], [0, 1], shadow=shadow.view(torch.float32)[:100])
    with pytest.raises(RuntimeError, match="kinds"):
        ops.EmaTable([good], [2], shadow=shadow.view(torch.float32))
    table = ops.EmaTable([good], [ops.EMA_AVERAGE], shadow=shadow.view(torch.float32))
    for D in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="decay"):
            ops.ema_update(table, D)
    with pytest.raises(RuntimeError, match="EmaTable"):
        ops.ema_swap([good])
    torch.cuda.synchronize()
    assert torch.equal(shadow, before)
    # a source whose storage was replaced after the table was made is followed to its new place, never read at the old one
    holder = torch.nn.Parameter(torch.ones(40, device=cuda))
    table = ops.EmaTable([holder], [ops.EMA_COPY])
    holder.data = torch.full((44,), 2.0, device=cuda)[:40]
    ops.ema_fill(table)
    assert bool((table.slot(0) == 2.0).all())
    holder.data = torch.full((44,), 3.0, device=cuda)[1:41]
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.ema_fill(table)
    assert bool((table.slot(0) == 2.0).all())


# ------------------------------------------------------------------------------------------------ the trainer
def _make(cuda, graphs, seed=0, ema=DECAY, strip=False):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, TINY)
    if strip:                                     # a namespace from before the flags existed
        del opt.ema_decay, opt.ema_warmup
    else:
        opt.ema_decay = ema
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
    return tr.step(batch)


def _flat(named):
    """One float32 host vector of the tensors, in order (logical element order)."""
    return torch.cat([t.detach().reshape(-1) for _, t in named]).cpu().numpy()


class _Host64:
    """The float64 shadow of a trainer's parameters, advanced on the host with the wrapper's own scalars, and the K-step
    bound of tests/ema_cases.py."""

    def __init__(self, tr):
        self.tr = tr
        self.names = [n for n, _ in tr.model.named_parameters()]
        self.e = _flat(tr.model.named_parameters()).astype(np.float64)
        self.worst_b, self.d_max, self.k, self.worst = np.zeros_like(self.e), 0.0, 0, 0.0
        sd = tr.ema.state_dict()
        assert np.array_equal(_flat([(n, sd[n]) for n in self.names]).view(np.int32),
                              _flat(tr.model.named_parameters()).view(np.int32)), "the shadow starts as the live weights"

    def after_step(self):
        from canonicalsg2im_amd.ema import decay_at
        tr = self.tr
        self.k += 1
        assert tr.ema.num_updates == self.k
        d, omd = ec.scalars(decay_at(DECAY, self.k))
        p = _flat(tr.model.named_parameters())
        ref = d * self.e + omd * p.astype(np.float64)
        self.worst_b = np.maximum(self.worst_b, ec.step_bound(p, self.e, ref, d, omd))
        self.e, self.d_max = ref, max(self.d_max, d)
        sd = tr.ema.state_dict()
        got = _flat([(n, sd[n]) for n in self.names])
        ratio = ec.check_average(got, self.e, self.worst_b * ec.steps_factor(self.k, self.d_max), "shadow after step %d" % self.k)
        self.worst = max(self.worst, ratio)
        assert (got != p).any(), "the shadow is the live weights: nothing was averaged"
        for n, b in tr.model.named_buffers():
            if b.is_floating_point():
                assert _same_bits(sd[n], b), "buffer %s of the shadow is not the live one after step %d" % (n, self.k)
            elif n in sd:
                assert torch.equal(sd[n], b), n


@pytest.fixture(scope="module")
def eager_run(cuda):
    """Four eager steps with the EMA on, tracked against the float64 shadow; checkpoints after steps 2 and 4."""
    vocab, tr = _make(cuda, graphs=False)
    assert tr.ema is not None and tr.ema.decay == DECAY and tr.ema.warmup
    host = _Host64(tr)
    batches = [_batch(vocab, cuda, 70 + i) for i in range(4)]
    ck2 = None
    for n, b in enumerate(batches, 1):
        _step(tr, b, n)
        host.after_step()
        if n == 2:
            ck2 = copy.deepcopy(tr.checkpoint_dict(2, 0))
    return {"vocab": vocab, "tr": tr, "host": host, "batches": batches, "ck2": ck2, "ck4": copy.deepcopy(tr.checkpoint_dict(4, 0))}


def test_eager_training(eager_run):
    tr, host = eager_run["tr"], eager_run["host"]
    print("eager: worst |shadow - fp64 shadow| / K-step bound %.3f" % host.worst)
    assert tr.ema.num_updates == 4 and host.k == 4 and tr._eager_steps == 4
    # the state dict has the model's keys, in the model's order, and loads strictly into a fresh model
    sd, live = tr.ema.state_dict(), tr.model.state_dict()
    assert list(sd) == list(live)
    assert all(sd[k].shape == live[k].shape and sd[k].dtype == live[k].dtype and sd[k].stride() == live[k].stride() for k in live)
    assert any(k.endswith("num_batches_tracked") for k in sd) or not any(k.endswith("num_batches_tracked") for k in live)
    from canonicalsg2im_amd.sg2im.meta_models import MetaGeneratorModel
    fresh = MetaGeneratorModel(tr.opt, tr.device)
    fresh.load_state_dict(sd, strict=True)
    ck = eager_run["ck4"]
    assert set(ck) >= {"model_state", "model_ema_state", "ema"} and ck["ema"] == {"decay": DECAY, "warmup": True, "num_updates": 4}
    assert list(ck["model_ema_state"]) == list(ck["model_state"])
    # nested use is refused, and so is an update inside the block
    with tr.ema.swapped():
        with pytest.raises(RuntimeError, match="not re-entrant"):
            with tr.ema.swapped():
                pass
        with pytest.raises(RuntimeError, match="swapped"):
            tr.ema.update()
    assert all(_same_bits(a, b) for a, b in zip(tr.ema.state_dict().values(), sd.values()))


def test_replayed_training(cuda):
    """The same over steps that ARE replayed from HIP graphs: the generator's Adam step of a replayed iteration runs on a side
    stream; an update that did not wait for it would average the weights of the step before."""
    vocab, tr = _make(cuda, graphs=True)
    host = _Host64(tr)
    batch = _batch(vocab, cuda, 80)
    for n in range(1, 6):                          # eager, capture + replay, three replays
        _step(tr, batch, n)
        host.after_step()
    g = tr.graphs
    print("replayed: worst ratio %.3f; captures %d replays %d eager %d" % (host.worst, g.captures, g.replays, g.eager_steps))
    assert g.captures == 1 and g.replays == 4 and g.eager_steps == 1 and tr._eager_steps == 1
    assert tr.ema.num_updates == 5


def test_resume(cuda, eager_run, capsys):
    """Saved after step 2, loaded into a differently initialised trainer, two more steps: shadow and counter are the bits of
    the uninterrupted run.  A checkpoint without the keys fills the shadow from model_state and says so."""
    ck2, ck4, batches = eager_run["ck2"], eager_run["ck4"], eager_run["batches"]
    assert ck2["ema"]["num_updates"] == 2
    _, tr = _make(cuda, graphs=False, seed=99)
    assert tr.load_checkpoint(copy.deepcopy(ck2)) == (2, 0)
    assert tr.ema.num_updates == 2
    assert all(_same_bits(a, b.to(cuda)) for a, b in zip(tr.ema.state_dict().values(), ck2["model_ema_state"].values()))
    for n in (3, 4):
        _step(tr, batches[n - 1], n)
    assert tr.ema.num_updates == 4
    sd = tr.ema.state_dict()
    diff = [k for k in sd if not _same_bits(sd[k], ck4["model_ema_state"][k].to(cuda))]
    assert not diff, "resumed shadow differs from the uninterrupted run's in %d tensors, e.g. %s" % (len(diff), diff[:3])
    live = tr.model.state_dict()
    assert all(_same_bits(live[k], ck4["model_state"][k].to(cuda)) for k in live)
    # without the keys (a reference checkpoint, a run that turns the EMA on late)
    bare = {k: v for k, v in copy.deepcopy(ck2).items() if k not in ("model_ema_state", "ema")}
    capsys.readouterr()
    tr.load_checkpoint(bare)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "model_ema_state" in out and "num_updates = 0" in out, out
    assert tr.ema.num_updates == 0
    sd = tr.ema.state_dict()
    assert all(_same_bits(sd[k], bare["model_state"][k].to(cuda)) for k in sd)


def test_off_is_off(cuda):
    """--ema_decay 0 against a trainer whose namespace has no ema_* attribute at all: no EMA object, today's checkpoint keys,
    and two steps (one eager, one captured and replayed) with the same losses and parameters, bit for bit."""
    vocab, old = _make(cuda, graphs=True, strip=True)
    _, off = _make(cuda, graphs=True, ema=0)
    assert not hasattr(old.opt, "ema_decay") and not hasattr(old.opt, "ema_warmup")
    assert old.ema is None and off.ema is None
    batch = _batch(vocab, cuda, 90)
    for n in (1, 2):
        Ga, Da = _step(old, batch, n)
        Gb, Db = _step(off, batch, n)
        assert list(Ga) == list(Gb) and list(Da) == list(Db)
        assert all(_same_bits(Ga[k], Gb[k]) for k in Ga) and all(_same_bits(Da[k], Db[k]) for k in Da), "losses of step %d" % n
    for (n, a), (_, b) in zip(list(old.model.named_parameters()) + list(old.discriminator.named_parameters()),
                              list(off.model.named_parameters()) + list(off.discriminator.named_parameters())):
        assert _same_bits(a, b), n
    today = {"model_state", "gans_model_state", "d_img_state", "d_img_optim_state", "optim_state", "vocab", "counters"}
    assert set(off.checkpoint_dict()) == today and set(old.checkpoint_dict()) == today
    assert old.graphs.replays == 1 and off.graphs.replays == 1


def test_sampler(cuda, eager_run):
    from canonicalsg2im_amd.sample import Sampler
    ck, vocab, opt = eager_run["ck4"], eager_run["vocab"], eager_run["tr"].opt
    _, objs, boxes, triplets, _, tt, _, _ = _batch(vocab, cuda, 95)
    draw = lambda s: s.generate(objs, triplets, tt, boxes_gt=boxes)[0]
    ema = draw(Sampler(opt, cuda, ck, use_ema=True))
    moved = dict(ck, model_state=ck["model_ema_state"])
    want = draw(Sampler(opt, cuda, moved))
    raw = draw(Sampler(opt, cuda, ck, use_ema=False))
    assert ema.dtype == torch.uint8 and torch.equal(ema, want)
    assert not torch.equal(ema, raw), "the averaged weights draw the raw weights' bytes"
    s = Sampler(opt, cuda)
    s.load(ck, use_ema=True)
    assert torch.equal(draw(s), want)
    bare = {k: v for k, v in ck.items() if k != "model_ema_state"}
    with pytest.raises(KeyError, match="--ema_decay"):
        Sampler(opt, cuda, bare, use_ema=True)
    with pytest.raises(KeyError, match="--ema_decay"):
        s.load(bare, use_ema=True)
    with pytest.raises(ValueError, match="checkpoint"):
        Sampler(opt, cuda, use_ema=True)


def test_swap_and_caches(cuda):
    """Validation on the averaged weights, swapped in and out, leaves training where it was.  The twin never swaps; it runs the
    same validation pass on its raw weights, because a pass advances the discriminator's spectral-norm vectors (evaluate.py),
    which depend on the discriminator's weights alone."""
    from canonicalsg2im_amd.evaluate import Evaluator
    vocab, a = _make(cuda, graphs=True)
    _, b = _make(cuda, graphs=True)
    batch, val = _batch(vocab, cuda, 60), _batch(vocab, cuda, 61)
    for n in (1, 2, 3):                            # eager, capture + replay, replay
        _step(a, batch, n)
        _step(b, batch, n)
    ck = copy.deepcopy(a.checkpoint_dict(3, 0))
    shadow = a.ema.state_dict()
    before = {k: v.detach().clone() for k, v in a.model.state_dict().items()}
    ev = Evaluator(a)
    with a.ema.swapped():
        ev.sampler.invalidate()
        live = a.model.state_dict()
        assert all(_same_bits(live[k], shadow[k]) for k in live), "inside swapped() the live weights are the shadow"
        inside = a.ema.state_dict()
        assert all(_same_bits(inside[k], before[k]) for k in before), "inside swapped() the shadow holds the raw weights"
        losses, _, _ = ev.check_model([val], use_gt=True)
        ev.sampler.invalidate()
    after = a.model.state_dict()
    assert all(_same_bits(after[k], before[k]) for k in before), "after swapped() the weights are not what they were"
    assert all(_same_bits(x, y) for x, y in zip(a.ema.state_dict().values(), shadow.values()))
    # the same pass on a fresh trainer loaded from the averaged weights
    _, c = _make(cuda, graphs=True, seed=5, ema=0)
    c.load_checkpoint(dict(ck, model_state=ck["model_ema_state"]))
    want, _, _ = Evaluator(c).check_model([val], use_gt=True)
    assert set(losses) == set(want)
    for k in want:
        print("swapped %-14s %.9g   fresh trainer %.9g" % (k, float(losses[k]), float(want[k])))
    for k in want:
        assert _same_bits(losses[k], want[k]), "%s: %r inside swapped(), %r from a trainer loaded with the averaged weights" % (
            k, float(losses[k]), float(want[k]))
    # the next training step equals the twin's, which never swapped
    Evaluator(b).check_model([val], use_gt=True)
    Ga, Da = _step(a, batch, 4)
    Gb, Db = _step(b, batch, 4)
    assert all(_same_bits(Ga[k], Gb[k]) for k in Ga) and all(_same_bits(Da[k], Db[k]) for k in Da), "losses after the swap"
    for (n, pa), (_, pb) in zip(list(a.model.named_parameters()) + list(a.discriminator.named_parameters()),
                                list(b.model.named_parameters()) + list(b.discriminator.named_parameters())):
        assert _same_bits(pa, pb), "%s differs from the twin's after the step that followed the swap" % n
    assert all(_same_bits(x, y) for x, y in zip(a.ema.state_dict().values(), b.ema.state_dict().values()))
    assert a.graphs.replays == 3 and b.graphs.replays == 3
