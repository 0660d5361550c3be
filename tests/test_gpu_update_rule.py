"""Every optimiser update of the trainer against the fp64 Adam restatement of tests/adam_cases.py.

Each case runs 4-8 training steps of the tiny trainer with every rate at a value of its own (a swap between groups shows) and
wraps every step in `UpdateChecker`: parameters after the step within 3 e_32 + u of adam64 fed the device's own pre-step
parameters and gradient, tensors without a gradient bit-identical, step counters and moments right at the end of the case.
The worst figures per (case, optimiser) are printed and, with UPDATE_RULE_REPORT=<file>, written there
(profiles/update_rule_errors.txt is such a run).

Which optimiser object takes which path, per case:
  1  eager, both recipes        fused multi-tensor Adam: `optimizer` (two groups), `optimizer_d_img` (fused + capturable, issued
                                eagerly), `optimizer_d_obj`
  2  masks / learned converse   + `optimizer_d_mask` (fused, eager); `optimizer_converse` (plain single-tensor Adam, REINFORCE step)
  3  frozen / graph-only        `optimizer` alone; every other optimiser must stay without state
  4  replayed                   `optimizer` on the side stream beside S3 (OVERLAP) or in stream order, `optimizer_d_img` captured
                                inside graph S3, `optimizer_d_obj` eager on the side stream; static gradient buffers re-pointed
  5  (gradients, not updates)   the replayed steps' gradients against an eager twin's
  6  checkpoint continuation    step counters made device tensors by `train._load_optimizer`, then eager / captured / replayed
  7  learning-rate edit         as 4, after `StepGraphs.invalidate()`
  8  process group up           every Adam step after `GradBuckets.finish()`, outside the graphs"""
import copy
import os

import pytest
import torch

import adam_cases as ac

pytestmark = pytest.mark.gpu

TINY = ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32", "--gconv_hidden_dim", "64",
        "--gconv_num_layers", "2", "--embedding_dim", "8", "--no_vgg_loss"]
RATES = ["--learning_rate", "3e-4", "--img_learning_rate", "2e-4", "--mask_learning_rate", "5e-5", "--beta1", "0.6"]
RTOL = 1e-4                                   # the project's contract (tests/test_gpu_modules.py)


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def dump_table():
    yield
    ac.write_report()


def _make(cuda, argv, graphs, seed=0, batch_size=2):
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    vocab = make_vocab("tiny")
    opt = T.make_opt(vocab, TINY + RATES + ["--batch_size", str(batch_size)] + argv)
    torch.manual_seed(seed)
    tr = T.Trainer(opt, cuda)
    if not graphs:
        tr.graphs = None
    else:
        assert tr.graphs is not None, "graph replay should be available for this recipe"
    return vocab, tr


def _batch(vocab, cuda, B, seed, mask_size=0, converse=False):
    from canonicalsg2im_amd.synth import BatchConfig, make_batch
    batch = list(make_batch(vocab, BatchConfig(B, 64, 2, 5, "packed", mask_size=mask_size), seed))
    if converse:                               # sampled converse edges for the REINFORCE step (synth leaves the counts at zero)
        cc = torch.randint(0, 3, batch[4].shape, generator=torch.Generator().manual_seed(seed)).float()
        cc[:, :2] = 0
        batch[4] = cc
    return [None if t is None else t.to(cuda) for t in batch]


def _run_case(tr, batches, case):
    chk = ac.UpdateChecker(tr, case)
    for b in batches:
        chk.step(b)
    chk.finish()
    return chk


def _moved(chk):
    return {n for n, k in chk.expected_steps.items() if k}


# ------------------------------------------------------------------------------------------------ 1-3: eager
@pytest.mark.parametrize("use_img_disc", [0, 1])
def test_eager_both_recipes(cuda, use_img_disc):
    vocab, tr = _make(cuda, ["--use_img_disc", str(use_img_disc)], graphs=False)
    chk = _run_case(tr, [_batch(vocab, cuda, 2 + i % 2, 20 + i) for i in range(5)], "1 eager use_img_disc=%d" % use_img_disc)
    tags = {chk.hyper[n][0] for n in _moved(chk)}
    assert tags == ({"optimizer", "optimizer_d_img"} | (set() if use_img_disc else {"optimizer_d_obj"})), tags
    assert chk.expected_steps[ac.TRANS] == 5


def test_eager_masks(cuda):
    # (the mask net reads the object vectors followed by the noise row: g_mask_dim = gconv_dim + mask_noise_dim, 32 + 64)
    vocab, tr = _make(cuda, ["--use_img_disc", "0", "--mask_size", "16", "--g_mask_dim", "96"], graphs=False)
    assert tr.graphs is None
    chk = _run_case(tr, [_batch(vocab, cuda, 2, 30 + i, mask_size=16) for i in range(4)], "2 eager masks")
    tags = {chk.hyper[n][0] for n in _moved(chk)}
    assert tags == {"optimizer", "optimizer_d_img", "optimizer_d_obj", "optimizer_d_mask"}, tags


def test_eager_learned_converse(cuda):
    vocab, tr = _make(cuda, ["--use_img_disc", "1", "--learned_converse", "1"], graphs=False, batch_size=3)
    chk = _run_case(tr, [_batch(vocab, cuda, 3, 40 + i, converse=True) for i in range(4)], "2 eager learned converse")
    assert chk.expected_steps["sg_to_layout.module.converse_candidates_weights"] == 4
    assert not tr.optimizer_converse.param_groups[0].get("fused"), "the converse weights are stepped by plain Adam"


def test_frozen_generation(cuda):
    """--freeze 1 --freeze_options generation: every generator and discriminator tensor stays bit-identical (the checker
    holds a tensor without a gradient to that at every step) and has no optimiser state; only the encoder moves."""
    vocab, tr = _make(cuda, ["--freeze", "1", "--freeze_options", "generation"], graphs=False)
    chk = _run_case(tr, [_batch(vocab, cuda, 2, 50 + i) for i in range(4)], "3 frozen generation")
    moved = _moved(chk)
    assert moved and all(n.startswith("sg_to_layout.") for n in moved), sorted(moved)[:5]
    for tag, o in ac.optimizers_of(tr).items():
        assert tag == "optimizer" or not o.state, tag


def test_graph_only_trainer(cuda):
    """--skip_generation 1 (config C1's trainer): the encoder's update at every tensor, four steps."""
    vocab, tr = _make(cuda, ["--skip_generation", "1"], graphs=False, batch_size=3)
    assert not hasattr(tr.model, "layout_to_image_model")
    chk = _run_case(tr, [_batch(vocab, cuda, 3, 60 + i) for i in range(4)], "3 graph-only")
    moved = _moved(chk)
    assert len(moved) >= 10 and all(n.startswith("sg_to_layout.") for n in moved)


def test_checker_sees_a_wrong_beta2_on_the_device(cuda):
    """The checker's device side is live: with beta2 = 0.99 in the image discriminator's (fused) optimiser — a fault the
    2.2 * steps * lr bounds of the older tests cannot see — the param-group check refuses the trainer, and with that check
    off the parameters themselves leave the bound (tests/test_adam_cases.py plants every fault on the host)."""
    vocab, tr = _make(cuda, ["--use_img_disc", "1"], graphs=False)
    for g in tr.discriminator.optimizer_d_img.param_groups:
        g["betas"] = (g["betas"][0], 0.99)
    with pytest.raises(AssertionError, match="optimiser structure"):
        ac.UpdateChecker(tr, "wrong beta2")
    chk = ac.UpdateChecker(tr, "wrong beta2", structure=False)
    raised = []
    for i in range(4):
        try:
            chk.step(_batch(vocab, cuda, 2, 20 + i))
        except AssertionError as e:
            raised.append(i + 1)
            assert "[optimizer_d_img]" in str(e) and "[optimizer]" not in str(e), str(e)[:400]
    print("beta2 = 0.99 on the device: raised at steps %s, e_dev / (3 e_32 + u) at the last step %.3g" % (raised, chk.ratio))
    assert raised == [2, 3, 4], raised            # (the first step is lr * g / (|g| + eps) for any betas)


# ------------------------------------------------------------------------------------------------ 4: replayed
def _sequence(vocab, cuda):
    """A: eager / A: capture / A: replay / B: eager / A: replay after an eager step (point_grads) / B: capture /
    A: replay (the active set switches) / B: replay — every step on a batch of its own."""
    return [_batch(vocab, cuda, {"A": 2, "B": 3}[k], 70 + i) for i, k in enumerate("AAABABAB")]


def _assert_sequence(tr):
    g = tr.graphs
    assert (g.captures, g.replays, g.eager_steps) == (2, 6, 2), (g.captures, g.replays, g.eager_steps)


@pytest.mark.parametrize("use_img_disc,overlap", [(0, True), (1, True), (0, False)])
def test_replayed_both_recipes(cuda, monkeypatch, use_img_disc, overlap):
    from canonicalsg2im_amd import graphs
    if not overlap:
        monkeypatch.setattr(graphs, "OVERLAP", False)
    else:
        assert graphs.OVERLAP, "the default is the overlapped step"
    vocab, tr = _make(cuda, ["--use_img_disc", str(use_img_disc)], graphs=True)
    chk = _run_case(tr, _sequence(vocab, cuda), "4 replayed use_img_disc=%d%s" % (use_img_disc, "" if overlap else " one stream"))
    _assert_sequence(tr)
    assert (tr.graphs.side is not None) == overlap
    g0 = tr.discriminator.optimizer_d_img.param_groups[0]
    assert g0["fused"] and g0["capturable"]
    assert chk.expected_steps[ac.TRANS] == 8


# ------------------------------------------------------------------------------------------------ 5: the gradients themselves
def _copy_state(src, dst):
    from canonicalsg2im_amd import ops
    dst.model.load_state_dict(copy.deepcopy(src.model.state_dict()))                   # parameters, running statistics
    dst.discriminator.load_state_dict(copy.deepcopy(src.discriminator.state_dict()))   # ... and the spectral u / v
    ops.invalidate_weight_caches()


def _grads(tr):
    return {n: (None if p.grad is None else p.grad.detach().double().clone()) for n, p in ac.named_tensors(tr)}


def test_replayed_gradients_are_this_steps(cuda):
    """`UpdateChecker` reads the gradient from the tensor the optimiser reads: a buffer left over from another batch would
    pass it.  Here the gradients of every step of case 4's sequence (image-discriminator recipe: no float atomics on the path)
    are compared with those of an eager twin that starts the step from the graphed trainer's full state:
    |g_graphed - g_twin| <= 1e-4 |g_twin| + 3 d per tensor (L2), d = the distance between two such eager twins."""
    argv = ["--use_img_disc", "1"]
    vocab, graphed = _make(cuda, argv, graphs=True)
    _, twin = _make(cuda, argv, graphs=False, seed=1)
    _, twin2 = _make(cuda, argv, graphs=False, seed=2)
    worst_d, worst_rel, bad = 0.0, 0.0, []
    for it, b in enumerate(_sequence(vocab, cuda)):
        _copy_state(graphed, twin)
        _copy_state(graphed, twin2)
        twin.step(b)
        twin2.step(b)
        graphed.step(b)
        torch.cuda.synchronize()
        gg, gt, gt2 = _grads(graphed), _grads(twin), _grads(twin2)
        assert list(gg) == list(gt) == list(gt2)
        n_grad = 0
        for n in gg:
            assert (gt[n] is None) == (gt2[n] is None), n
            if gg[n] is None and gt[n] is None:
                continue
            zero = torch.zeros_like(gg[n] if gg[n] is not None else gt[n])
            a, t, t2 = (zero if x is None else x for x in (gg[n], gt[n], gt2[n]))
            n_grad += 1
            d, diff, ref = float((t - t2).norm()), float((a - t).norm()), float(t.norm())
            worst_d = max(worst_d, d)
            if ref > 0:
                worst_rel = max(worst_rel, diff / ref)
            if not diff <= RTOL * ref + 3 * d:
                bad.append("step %d %s: |g_graphed - g_twin| %.3e, |g_twin| %.3e, d %.3e" % (it + 1, n, diff, ref, d))
        assert n_grad > 50
    print("case 5: twin-to-twin distance d = %.3e (worst tensor), worst |g_graphed - g_twin| / |g_twin| = %.3e" % (worst_d, worst_rel))
    ac.TABLE.append(("5 gradients vs eager twin", "(d, worst rel. L2)", worst_d, worst_rel, 0.0, 0.0, "twin-to-twin d / worst relative distance"))
    _assert_sequence(graphed)
    assert not bad, "%d gradient tensors differ from the eager twin's\n%s" % (len(bad), "\n".join(bad[:20]))


# ------------------------------------------------------------------------------------------------ 6: checkpoint continuation
def test_checkpoint_continuation(cuda):
    """Three eager steps, a checkpoint in the form plain Adam writes (host step counters, no fused / capturable flags),
    `load_checkpoint` into a fresh graphed trainer, three more steps (eager, capture, replay) whose twins start from the
    checkpoint's (t, m, v): the steps must be taken with t = 4, 5, 6."""
    argv = ["--use_img_disc", "0"]
    vocab, a = _make(cuda, argv, graphs=False)
    bs = [_batch(vocab, cuda, 2, 80 + i) for i in range(6)]
    _run_case(a, bs[:3], "6 before the checkpoint")
    ck = copy.deepcopy(a.checkpoint_dict(t=3))
    keys = {"optim_state": "optimizer", "d_img_optim_state": "optimizer_d_img", "d_obj_optim_state": "optimizer_d_obj",
            "d_mask_optim_state": "optimizer_d_mask"}
    for key in keys:
        for g in ck[key]["param_groups"]:
            g.update(fused=None, capturable=False, foreach=None)
        for st in ck[key]["state"].values():
            st["step"] = st["step"].detach().cpu()
    _, b = _make(cuda, argv, graphs=True, seed=99)
    b.load_checkpoint(ck)
    chk = ac.UpdateChecker(b, "6 after the checkpoint")
    for key, tag in keys.items():
        chk.seed(tag, ck[key])
    assert chk.expected_steps[ac.TRANS] == 3
    for batch in bs[3:]:
        chk.step(batch)
    chk.finish()
    g = b.graphs
    assert (g.captures, g.replays, g.eager_steps) == (1, 2, 1)
    assert chk.expected_steps[ac.TRANS] == 6
    for tag, o in ac.optimizers_of(b).items():
        for grp in o.param_groups:
            for p in grp["params"]:
                st = o.state.get(p)
                if st and grp.get("fused"):
                    assert st["step"].is_cuda and st["step"].dtype == torch.float32, tag


# ------------------------------------------------------------------------------------------------ 7: learning-rate edit
def test_learning_rate_edit(cuda):
    """After a replayed step every group's rate is halved and the graphs are dropped (`StepGraphs.invalidate`: the rate of
    the captured step is baked in); the next three steps (eager, capture, replay) run at the new rates."""
    vocab, tr = _make(cuda, ["--use_img_disc", "0"], graphs=True)
    bs = [_batch(vocab, cuda, 2, 90 + i) for i in range(6)]
    chk = ac.UpdateChecker(tr, "7 learning-rate edit")
    for b in bs[:3]:
        chk.step(b)
    assert tr.graphs.replays == 2
    for o in ac.optimizers_of(tr).values():
        for g in o.param_groups:
            g["lr"] = g["lr"] * 0.5
    tr.graphs.invalidate()
    chk.scale_lr(0.5)
    chk.check_structure()
    for b in bs[3:]:
        chk.step(b)
    chk.finish()
    g = tr.graphs
    assert (g.captures, g.replays, g.eager_steps) == (2, 4, 2)


# ------------------------------------------------------------------------------------------------ 8: process group up
def _update_rule_nccl_worker(rank, port, out):
    """A one-rank nccl group with CSG_DIST_FORCE=1 CSG_GRAPHS_DIST=1 (as `_one_rank_nccl_worker` of tests/test_gpu_graphs.py):
    the gradients travel through the buckets and every Adam step follows `GradBuckets.finish()`, outside the graphs."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      CSG_DIST_FORCE="1", CSG_GRAPHS_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
                      TORCH_NCCL_TRACE_BUFFER_SIZE="2000", TORCH_FR_BUFFER_SIZE="2000")   # (dist.init_from_env sets these)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1)
    from canonicalsg2im_amd import dist as D
    assert D.active() and D.capturable() and D.world_size() == 1
    cuda = torch.device("cuda:0")
    res = {}
    for use_img_disc in (0, 1):
        vocab, tr = _make(cuda, ["--use_img_disc", str(use_img_disc)], graphs=True)
        bs = [_batch(vocab, cuda, 2, 100 + i) for i in range(5)]
        errors = []
        try:
            _run_case(tr, bs, "8 nccl group use_img_disc=%d" % use_img_disc)
        except AssertionError as e:
            errors.append(str(e))
        res[use_img_disc] = {"errors": errors, "captures": tr.graphs.captures, "replays": tr.graphs.replays,
                             "eager_steps": tr.graphs.eager_steps,
                             "fused": bool(tr.optimizer.param_groups[0].get("fused"))}
    res["table"] = list(ac.TABLE)
    out.update(res)
    dist.barrier()
    dist.destroy_process_group()


def test_process_group_up():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    mp.spawn(_update_rule_nccl_worker, args=(port, out), nprocs=1, join=True)
    ac.TABLE.extend(out["table"])
    print("\n".join([ac.HEADER] + ac.format_rows(out["table"])))
    for use_img_disc in (0, 1):
        r = out[use_img_disc]
        assert not r["errors"], "\n".join(r["errors"])
        assert (r["captures"], r["replays"], r["eager_steps"]) == (1, 4, 1), r
        assert r["fused"]
