"""Every normalisation / SPADE code path on a real MI355X against the float64 restatement of the family's contract
(tests/norm_cases.py: the table and `norm_ref64`).

Per row: the ops entry points that served it (and, for _SpadeFused, the launches ops.WINO4_AUDIT counted: `spade_joint`
against `spade_gamma` / `spade_beta`) must be the row's; every output, every gradient that was asked for and the running
statistics must meet the gate below, a gradient not asked for must come back None.  The allocator's free blocks are
filled with NaN before each run; every row runs twice and must reproduce itself bit for bit.  The N-replica rows run in
one fresh child process with a one-rank gloo group and CSG_DIST_FORCE=1 (identity all-reduces, the max(var, eps) form).

Gate: 1e-5 of the largest fp64 entry plus a 1e-6 floor (tests/test_gpu_conv_plans.py), with y and dx judged PER CHANNEL
(channels differ in inv_std by orders of magnitude on the offset and zero-variance rows).  Rows marked `mean_term` add
what handing `mean` over in fp32 costs, computed from the fp64 reference: 2^-24 |mean_c| invstd_c in xhat — times
max|1 + gamma_c| for y, times invstd_c |mean(dn xhat)_c| for dx."""
import os
import sys
import time
import types

import pytest
import torch

import norm_cases as nc
from norm_cases import CASES, case_ids
from conv_cases import kink_mask
from test_gpu_conv_plans import SLICE, _nan_fill, _place

pytestmark = pytest.mark.gpu
GATE, FLOOR = 1e-5, 1e-6
ENTRIES = ("norm_act", "norm_act_pair", "spade_joined", "spade_fused")
KINDS = ("spade_joint", "spade_gamma", "spade_beta")
CHILD_LIMIT = 180             # seconds for the child process of the N-replica rows
WORST = {}                    # path -> worst error / scale seen (printed when the module is done)

LOCAL = [c for c in CASES if not c["multi"]]
MULTI = [c for c in CASES if c["multi"]]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from canonicalsg2im_amd import ops as o
    yield o
    for path in nc.PATHS:                              # the worst error / scale per path over the rows that ran
        if path in WORST:
            print("| worst | %-14s | %.2e |" % (path, WORST[path]), file=sys.stderr)


# ------------------------------------------------------------------------------------ one run of a row on the device
def _spade_module(c, d, k, kind):
    from canonicalsg2im_amd.spade.models.networks.normalization import SPADE
    sp = SPADE("spade%s3x3" % kind, c["C"], nc.SEG_NC)
    _load_spade(sp, c, d, k)
    return sp


def _load_spade(sp, c, d, k):
    C, m = c["C"], d["mods"][k]
    with torch.no_grad():
        sp.mlp_shared[0].weight.copy_(m["w_sh"])
        sp.mlp_shared[0].bias.copy_(m["b_sh"])
        sp.mlp_gamma.weight.copy_(m["w"][:C])
        sp.mlp_beta.weight.copy_(m["w"][C:])
        sp.mlp_gamma.bias.copy_(m["b"][:C])
        sp.mlp_beta.bias.copy_(m["b"][C:])
        pn = sp.param_free_norm
        if getattr(pn, "running_mean", None) is not None:
            pn.running_mean.copy_(m["rm"])
            pn.running_var.copy_(m["rv"])
    sp.param_free_norm.momentum = c["momentum"]


def _spade_grads(out, c, sp, k):
    g = lambda p: None if p.grad is None else p.grad
    cat = lambda a, b: None if g(a) is None else torch.cat([g(a), g(b)])
    out["dw%d" % k] = cat(sp.mlp_gamma.weight, sp.mlp_beta.weight)
    out["db%d" % k] = cat(sp.mlp_gamma.bias, sp.mlp_beta.bias)
    out["dw_sh%d" % k], out["db_sh%d" % k] = g(sp.mlp_shared[0].weight), g(sp.mlp_shared[0].bias)
    pn = sp.param_free_norm
    if c["running"][k] and not c["instance"]:
        out["rm%d" % k], out["rv%d" % k] = pn.running_mean, pn.running_var


def _run(ops, c, d):
    """One forward + backward of row `c`: {tensor name: device tensor or None}."""
    need, K, C = c["need"], c["K"], c["C"]
    g = lambda t: None if t is None or t.grad is None else t.grad
    x4 = d["x"]
    xl, xv = _place(x4, c["xfmt"], "x" in need)
    dys = [t.cuda() for t in d["dy"]]
    out = {}
    if c["mod"] == "affine":
        from canonicalsg2im_amd.sg2im.layers import BatchNorm1dAct, BatchNormAct
        from canonicalsg2im_amd.spade.models.networks.sync_batchnorm import SynchronizedBatchNorm2d
        if c["via"] == "affine2d":
            mod = BatchNormAct(C, fused_slope=c["slopes"][0])
        elif c["via"] == "affine1d":
            mod = BatchNorm1dAct(C, fused_slope=c["slopes"][0])
        else:
            mod = SynchronizedBatchNorm2d(C, affine=True)
        mod.momentum = c["momentum"]
        with torch.no_grad():
            mod.weight.copy_(d["weight"])
            mod.bias.copy_(d["bias"])
            mod.running_mean.copy_(d["mods"][0]["rm"])
            mod.running_var.copy_(d["mods"][0]["rv"])
        mod = mod.cuda().train(c["training"])
        mod.weight.requires_grad_("w" in need)
        mod.bias.requires_grad_("b" in need)
        shape = c["shape"] or tuple(x4.shape)
        xl = x4.reshape(shape).cuda().requires_grad_("x" in need)
        if c["refuse"]:
            return mod, xl
        y = mod(xl) if c["via"] != "affine_sync" else mod(xl, None, c["slopes"][0])
        y.backward(dys[0].reshape(shape))
        out.update(y0=y, dx=g(xl), dweight=g(mod.weight), dbias=g(mod.bias), rm0=mod.running_mean, rv0=mod.running_var)
        return out
    if c["mod"] == "seg":
        from canonicalsg2im_amd.spade.models.networks.architecture import SPADEResnetBlock
        from canonicalsg2im_amd.spade.models.networks.normalization import spade_pair
        seg = d["seg"].cuda().requires_grad_("a" in need)
        kind = "instance" if c["instance"] else "syncbatch"
        if c["via"] == "spade":
            sps = [_spade_module(c, d, 0, kind).cuda().train(c["training"])]
            ys = [sps[0](xv, seg, fused_slope=c["slopes"][0])]
        else:
            opt = types.SimpleNamespace(norm_G="spectralspade%s3x3" % kind, semantic_nc=nc.SEG_NC)
            blk = SPADEResnetBlock(C, C // 2 if c["via"] == "pair" else C, opt)
            sps = [blk.norm_s, blk.norm_0] if c["via"] == "pair" else [blk.norm_0]
            for k, sp in enumerate(sps):
                _load_spade(sp, c, d, k)
            blk.cuda().train(c["training"])
            assert blk.learned_shortcut == (c["via"] == "pair")
            if c["via"] == "pair":            # what SPADEResnetBlock.forward calls on its norms
                ys = list(spade_pair(blk.norm_s, blk.norm_0, xv, seg, c["slopes"][0], c["slopes"][1]))
            else:
                ys = [blk.norm_0(xv, seg, fused_slope=c["slopes"][0])]
        sum((y * dy).sum() for y, dy in zip(ys, dys)).backward()
        out.update(dx=g(xl), dseg=g(seg))
        for k, sp in enumerate(sps):
            out["y%d" % k] = ys[k]
            _spade_grads(out, c, sp, k)
        return out
    rms = [(m["rm"].cuda().clone(), m["rv"].cuda().clone()) if c["running"][k] else (None, None)
           for k, m in enumerate(d["mods"])]
    kw = dict(eps=c["eps"], momentum=c["momentum"])
    leaves = {}
    if c["mod"] == "gb":
        for k in range(K):
            leaves["gb%d" % k] = d["mods"][k]["gb"].cuda().requires_grad_("g" in need)
    elif c["mod"] == "conv":
        for k in range(K):
            m = d["mods"][k]
            actv = m["actv"]
            if c["refuse"] and "do not fit" in c["refuse"]:
                actv = actv[:, :, :, :-4]
            leaves["actv%d" % k] = actv.cuda().requires_grad_("a" in need)
            leaves["w%d" % k] = m["w"].cuda().contiguous(memory_format=torch.channels_last).requires_grad_("w" in need)
            leaves["b%d" % k] = m["b"].cuda().requires_grad_("b" in need)
    if c["path"] == "_NormAct":
        ys = [ops.norm_act(xv, leaves.get("gb0"), rms[0][0], rms[0][1], instance=c["instance"], training=c["training"],
                           slope=c["slopes"][0], **kw)]
    elif c["path"] == "_NormActPair":
        ys = list(ops.norm_act_pair(xv, leaves["gb0"], leaves["gb1"], rms[0][0], rms[0][1], rms[1][0], rms[1][1],
                                    c["slopes"][0], c["slopes"][1], **kw))
    elif c["path"] == "_SpadeJoined":
        ys = [ops.spade_joined(xv, leaves["actv0"], leaves["w0"], leaves["b0"], rms[0][0], rms[0][1], 1, c["slopes"][0],
                               c["in_slope"], **kw)]
    else:
        mods = [(leaves["actv%d" % k], leaves["w%d" % k], leaves["b%d" % k], rms[k][0], rms[k][1], c["slopes"][k],
                 c["in_slope"]) for k in range(K)]
        if c["refuse"]:
            return (lambda: ops.spade_fused(xv, mods, **kw)), rms
        ys = ops.spade_fused(xv, mods, **kw)
    loss = sum((y * dy).sum() for y, dy in zip(ys, dys))
    if loss.requires_grad:
        loss.backward()
    out["dx"] = g(xl)
    for k in range(K):
        out["y%d" % k] = ys[k]
        if c["running"][k] and not c["instance"]:
            out["rm%d" % k], out["rv%d" % k] = rms[k]
        if c["mod"] == "gb":
            out["dgb%d" % k] = g(leaves["gb%d" % k])
        elif c["mod"] == "conv":
            out["dactv%d" % k], out["dw%d" % k], out["db%d" % k] = (g(leaves[t + str(k)]) for t in ("actv", "w", "b"))
    return out


def _serve(ops, c, d):
    """Row `c` twice on NaN-filled memory with the entry points and the SPADE launches recorded: ([outputs of run 0, of
    run 1] as CPU tensors, entry points called, {audit kind: launches}, mlp_shared outputs of run 0)."""
    from canonicalsg2im_amd._lib import lib
    saved = {k: getattr(ops, k) for k in ENTRIES + ("conv2d", "WINO4_AUDIT") + tuple(c["knobs"])}
    served, shared = [], []

    def wrap(name):
        real = saved[name]

        def f(*a, **k):
            served.append(name)
            return real(*a, **k)
        return f

    def conv2d(*a, **k):
        y = saved["conv2d"](*a, **k)
        if k.get("grad_is_pre"):                     # mlp_shared's output: its ReLU gate is read off this tensor
            shared.append(y.detach().double().cpu())
        return y

    prev = lib.csg_wino4_persistent(0) if not c["persistent"] else None
    runs = []
    try:
        for name in ENTRIES:
            setattr(ops, name, wrap(name))
        ops.conv2d = conv2d
        for k, v in c["knobs"].items():
            setattr(ops, k, v)
        for i in range(2):
            _nan_fill()
            del served[:]
            if i:
                del shared[c["K"] if c["mod"] == "seg" else 0:]
            ops.WINO4_AUDIT = {}
            o = _run(ops, c, d)
            torch.cuda.synchronize()
            audit = {k: ops.WINO4_AUDIT.get(k, [0])[0] for k in KINDS}
            runs.append({t: (None if v is None else v.detach().cpu().clone()) for t, v in o.items()})
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        if prev is not None:
            lib.csg_wino4_persistent(0 if prev == 0 else 1)
    return runs, list(served), audit, shared[:c["K"]]


# ------------------------------------------------------------------------------------ judging
def tolerance(c, t, ref, full):
    """(scale, extra) of tensor `t`: per channel for y and dx, the whole tensor otherwise.  `extra` is the fp32-mean term
    of the module docstring on the rows that ask for it (zero elsewhere)."""
    per_channel = t == "dx" or t.startswith("y")
    if not per_channel:
        return ref.abs().max(), 0.0
    C = c["C"]
    red = [i for i in range(ref.dim()) if i != 1]
    scale = ref.abs().amax(red, keepdim=True)
    extra = torch.zeros_like(scale)
    if c["mean_term"]:
        chan = lambda v: v.abs().amax((0, 2, 3)).view(scale.shape)
        dxhat = 2.0 ** -24 * full["mean"].abs() * full["invstd"]               # (G, C, 1, 1)
        if t == "dx":
            dims = (2, 3) if c["instance"] else (0, 2, 3)
            extra = chan(dxhat * full["invstd"] * (full["dn"] * full["xhat"]).mean(dims, keepdim=True).abs())
        else:
            g1 = full["gam1"][int(t[1:])]
            extra = chan(dxhat.expand_as(full["xhat"]) * (1.0 if g1 is None else g1.abs()))
    return scale, extra


def _judge(c, t, got, ref, full, label, msgs):
    g = got.detach().double().cpu()
    if tuple(g.shape) != tuple(ref.shape):
        msgs.append("%s: shape %s, expected %s" % (t, tuple(g.shape), tuple(ref.shape)))
        return
    bad = int((~torch.isfinite(g)).sum())
    if bad:
        msgs.append("%s: %d non-finite entries (memory no kernel wrote?)" % (t, bad))
        return
    scale, extra = tolerance(c, t, ref, full)
    err = (g - ref).abs()
    allow = GATE * scale + FLOOR + extra
    worst = float((err / allow).max())                 # > 1: outside the gate
    rel = float((err / (scale + FLOOR / GATE)).max())
    WORST[c["path"]] = max(WORST.get(c["path"], 0.0), rel)
    print("| %-26s | %-6s | %-34s | %.2e | %.2f |" % (c["name"], t, label, rel, worst), file=sys.stderr)
    if worst > 1.0:
        msgs.append("%s (%s): error %.3e of the scale, %.2f x the allowance (gate %.0e + floor %.0e%s)" % (
            t, label, rel, worst, GATE, FLOOR, " + fp32-mean term" if c["mean_term"] else ""))


def _label(c, served, audit):
    s = "+".join(served)
    if c["path"] == "_SpadeFused":
        s += " j%d g%d b%d" % tuple(audit[k] for k in KINDS)
    return s


def _check(c, d, runs, served, audit, shared):
    """Everything a served row is held to: the path, the tensors against fp64, the second run."""
    assert served == c["calls"], "%s: served by %s, expected %s" % (c["name"], served, c["calls"])
    launch = c["launch"] or ()
    want = {"spade_joint": launch.count("joint"), "spade_gamma": launch.count("pair"), "spade_beta": launch.count("pair")}
    assert audit == want, "%s: launches %s, expected %s (does the device serve the joint form at this size?)" % (
        c["name"], audit, want)
    ref, full = nc.reference(c, d)
    if c["mod"] == "seg":
        # mlp_shared's ReLU gate reads its own fp32 output: where the fp64 pre-activation is within rounding of the kink the
        # reference takes the side the device took (as the convolution matrix does for its producer -> consumer pairs)
        gates = []
        for k in range(c["K"]):
            near = kink_mask(full["mods"][k]["pre_sh"]) == 0
            gates.append(torch.where(near, shared[k], full["mods"][k]["actv"]))
        ref, full = nc.reference(c, d, gates)
    if c["xfmt"] == "slice" and ref["dx"] is not None:
        ref["dx"] = torch.nn.functional.pad(ref["dx"], (0, 0, 0, 0, SLICE, SLICE))
    label, msgs = _label(c, served, audit), []
    assert set(runs[0]) == set(ref), "%s: tensors %s" % (c["name"], sorted(set(runs[0]) ^ set(ref)))
    for t, r in ref.items():
        got = runs[0][t]
        if r is None:
            if got is not None:
                msgs.append("%s was not asked for and came back" % t)
            continue
        if got is None:
            msgs.append("%s was asked for and did not come back" % t)
            continue
        _judge(c, t, got, r, full, label, msgs)
        if not torch.equal(got, runs[1][t]):
            msgs.append("%s: a second run differs (max %.3e)" % (t, float((got - runs[1][t]).abs().max())))
    assert not msgs, "%s:\n  " % c["name"] + "\n  ".join(msgs)


@pytest.mark.parametrize("c", LOCAL, ids=case_ids(LOCAL))
def test_path_against_fp64(ops, c):
    t0 = time.time()
    d = nc.make_data(c)
    if c["refuse"]:
        # refused with a clear error before anything is computed: the running statistics stay what they were
        if c["mod"] == "affine":
            mod, xl = _run(ops, c, d)
            before = (mod.running_mean.clone(), mod.running_var.clone())
            with pytest.raises(RuntimeError, match=c["refuse"]):
                mod(xl, torch.zeros(c["B"], 2 * c["C"], c["H"], c["W"], device="cuda"), 0.2)
            after = (mod.running_mean, mod.running_var)
        else:
            call, rms = _run(ops, c, d)
            before = tuple(t.clone() for t in rms[0])
            with pytest.raises(RuntimeError, match=c["refuse"]):
                call()
            after = rms[0]
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "%s: refused, but the running statistics moved" % c["name"]
        return
    frac = nc.mask_kinks(c, d)
    assert frac <= nc.MASK_CAP, (c["name"], frac)
    runs, served, audit, shared = _serve(ops, c, d)
    _check(c, d, runs, served, audit, shared)
    print("| %-26s | time   | %.2f s |" % (c["name"], time.time() - t0), file=sys.stderr)


# ------------------------------------------------------------------------------------ the N-replica rows, in a child
def _child(rank, port, path):
    """One rank, gloo, CSG_DIST_FORCE=1: every Function takes its N-replica branch with identity all-reduces."""
    import torch.distributed as dist
    os.environ["CSG_DIST_FORCE"] = "1"
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    from canonicalsg2im_amd import dist as csg_dist
    from canonicalsg2im_amd import ops
    assert csg_dist.active()
    res = {}
    for c in MULTI:
        t0 = time.time()
        d = nc.make_data(c)
        nc.mask_kinks(c, d)
        res[c["name"]] = _serve(ops, c, d) + (time.time() - t0,)
    torch.save(res, path)
    dist.destroy_process_group()


def test_n_replica_rows_in_a_child_process(tmp_path):
    """The `multi` rows of the table in ONE fresh child process; the parent judges what the child returns against
    norm_ref64 in its max(var, eps) form.  The child has its own time limit; if it dies the test fails with its exit
    status and starts nothing else."""
    import socket
    import torch.multiprocessing as mp
    t0 = time.time()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    path = str(tmp_path / "multi_rows.pt")
    ctx = mp.spawn(_child, args=(port, path), nprocs=1, join=False)
    try:
        while not ctx.join(timeout=5):
            if time.time() - t0 > CHILD_LIMIT:
                for p in ctx.processes:
                    p.kill()
                pytest.fail("the child process of the N-replica rows exceeded %d s and was killed" % CHILD_LIMIT)
    except Exception as e:                              # ProcessExitedException / ProcessRaisedException
        pytest.fail("the child process of the N-replica rows died: %s (exit code %s)" % (
            str(e).strip().splitlines()[-1] if str(e).strip() else type(e).__name__, getattr(e, "exit_code", None)))
    res = torch.load(path)
    assert set(res) == set(case_ids(MULTI))
    failures = []
    for c in MULTI:
        runs, served, audit, shared, dt = res[c["name"]]
        d = nc.make_data(c)
        nc.mask_kinks(c, d)
        try:
            _check(c, d, runs, served, audit, shared)
        except AssertionError as e:
            failures.append(str(e))
        print("| %-26s | time   | %.2f s (child) |" % (c["name"], dt), file=sys.stderr)
    print("| %-26s | time   | %.2f s |" % ("child process, all rows", time.time() - t0), file=sys.stderr)
    assert not failures, "\n".join(failures)
