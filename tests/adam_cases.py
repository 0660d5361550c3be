"""The parameter update against an fp64 restatement of Adam (no GPU needed to import this file).

Three pieces:

`adam64`         one Adam step written out in fp64, without torch.optim.
`RECIPE`         the reference's optimiser recipe, restated by hand from the reference's scripts/train.py and
                 sg2im/meta_models.py (lines cited at each rule).  Nothing is taken from the trainer under test.
`UpdateChecker`  wraps every training step of a trainer: it clones every parameter before the step, reads each parameter's
                 `.grad` after it, advances two host twins (adam64, and torch's own plain CPU fp32 Adam) from the device's
                 pre-step values and the device's gradient, and holds the device's post-step parameters to the rule of
                 tests/fp64_band.py: e_dev <= 3 * e_32 + u.

Which gradient the step consumed.  After `Trainer.step` and a device synchronisation `p.grad` is the gradient this step's Adam
read, on both paths:
  eager     every optimiser's `zero_grad(set_to_none=True)` runs before its backward (train.py, `_step_eager`,
            `_converse_step`), so the tensor in `.grad` was created by this step's backward, and nothing writes it between the
            backward and the optimiser's step;
  replayed  `.grad` of the generator's and the image discriminator's parameters are the static buffers of `_GraphSet.grads`,
            written by S2 / S3 of this very step (graphs.py `_run`), the encoder's are the static buffers of the replayed
            `_SgGraph` or the tensors of an eager encoder pass, the object discriminator's come from an eager backward after
            `zero_grad(set_to_none=True)`.
A buffer that is consistently the WRONG one (left over from another batch) is invisible from here — optimiser and checker would
read the same tensor; tests/test_gpu_update_rule.py::test_replayed_gradients_are_this_steps compares the gradients themselves
with an eager twin's."""
import math
import os
import re

import torch

K = 3.0            # fp64_band.Band's factor
EPS = 1e-8         # torch.optim.Adam's default, which every optimiser of the reference keeps


# ------------------------------------------------------------------------------------------------ the restatement
def adam64(state, p_before, g, hyper):
    """One Adam step in fp64.  `state`: dict holding (t, m, v) of ONE parameter tensor (empty before its first step);
    `p_before`: the parameter; `g`: its gradient or None; `hyper`: (lr, b1, b2, eps).  Returns the parameter after the step.
    No weight decay, no amsgrad.  A tensor without a gradient is skipped: parameter, moments and t stay untouched."""
    p = p_before.detach().to(torch.float64)
    if g is None:
        return p
    lr, b1, b2, eps = (float(h) for h in hyper)
    g = g.detach().to(torch.float64)
    if "t" not in state:
        state["t"], state["m"], state["v"] = 0, torch.zeros_like(p), torch.zeros_like(p)
    state["t"] += 1
    t = state["t"]
    state["m"] = b1 * state["m"] + (1.0 - b1) * g
    state["v"] = b2 * state["v"] + (1.0 - b2) * g * g
    denom = state["v"].sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    return p - lr / (1.0 - b1 ** t) * state["m"] / denom


# ------------------------------------------------------------------------------------------------ the recipe
# (pattern on the parameter's name, optimiser tag, learning rate, beta1, beta2, eps).  Names are those of
# `model.named_parameters()` (MetaGeneratorModel: `sg_to_layout.module.*`, `layout_to_image_model.module.*`) and of
# `discriminator.named_parameters()` (MetaDiscriminatorModel: `img_/obj_/mask_discriminator.*`).  A learning rate or beta
# given as a string is the command-line option of that name (scripts/args.py:20-23).  First match wins.
RECIPE = (
    # scripts/train.py:314-315, 317, 323: `converse_list`, Adam([{'params': learned_converse_params, 'lr': 1e-2}]) — its own optimiser
    (r"^sg_to_layout\.module\.converse_candidates_weights$", "optimizer_converse", 1e-2, 0.9, 0.999, EPS),
    # scripts/train.py:316, 318, 322: `trans_list`, second group of `optimizer`, 'lr': 1e-2
    (r"^sg_to_layout\.module\.trans_candidates_weights$", "optimizer", 1e-2, 0.9, 0.999, EPS),
    # scripts/train.py:285, 319-321: `base_params` = every other parameter of the MetaGeneratorModel, 'lr': learning_rate;
    # torch.optim.Adam's default betas
    (r"^(sg_to_layout|layout_to_image_model)\.", "optimizer", "learning_rate", 0.9, 0.999, EPS),
    # sg2im/meta_models.py:67-69: optimizer_d_img, lr=opt.img_learning_rate, betas=(opt.beta1, 0.999)
    (r"^img_discriminator\.", "optimizer_d_img", "img_learning_rate", "beta1", 0.999, EPS),
    # sg2im/meta_models.py:80-82: optimizer_d_obj, lr=opt.learning_rate, betas=(opt.beta1, 0.999)
    (r"^obj_discriminator\.", "optimizer_d_obj", "learning_rate", "beta1", 0.999, EPS),
    # sg2im/meta_models.py:88-90: optimizer_d_mask, lr=opt.mask_learning_rate, betas=(opt.beta1, 0.999)
    (r"^mask_discriminator\.", "optimizer_d_mask", "mask_learning_rate", "beta1", 0.999, EPS),
)
# the transitive weights are ONE Parameter registered under six names (sg2im/model.py:32,45 of the reference)
TRANS = "sg_to_layout.module.trans_candidates_weights"


def recipe(name, opt):
    """(optimiser tag, lr, b1, b2, eps) of parameter `name` under the options `opt`."""
    for pat, tag, lr, b1, b2, eps in RECIPE:
        if re.search(pat, name):
            val = lambda x: float(getattr(opt, x)) if isinstance(x, str) else float(x)
            return tag, val(lr), val(b1), val(b2), val(eps)
    raise KeyError("no optimiser recipe for parameter %r" % name)


def named_tensors(tr):
    """[(name, parameter)] of every network of a trainer, each Parameter once (its first name)."""
    return list(tr.model.named_parameters()) + list(tr.discriminator.named_parameters())


def optimizers_of(tr):
    """{tag: optimiser} of a trainer (or of an `oracle.TrainState`, which holds all of them itself)."""
    out = {}
    for owner in (tr, getattr(tr, "discriminator", None)):
        for tag in ("optimizer", "optimizer_converse", "optimizer_d_img", "optimizer_d_obj", "optimizer_d_mask"):
            o = getattr(owner, tag, None) if owner is not None else None
            if o is not None and tag not in out:
                out[tag] = o
    return out


def ulp32(x):
    """One fp32 unit in the last place at magnitude x."""
    x = torch.tensor(abs(float(x)), dtype=torch.float32)
    return float(torch.nextafter(x, torch.tensor(float("inf"))) - x)


def _sync(tr):
    dev = getattr(tr, "device", None)
    if dev is not None and torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the report
TABLE = []                                           # rows (case, optimiser, e_dev, e_32, u, worst e_dev / bound, tensor)
REPORT = os.environ.get("UPDATE_RULE_REPORT")        # a file that receives the table too (profiles/update_rule_errors.txt)
HEADER = "%-46s %-20s %10s %10s %10s %7s  %s" % ("case", "optimiser", "e_dev", "e_32", "u", "ratio", "tensor of the worst ratio")


def format_rows(rows):
    return ["%-46s %-20s %10.2e %10.2e %10.2e %7.3f  %s" % r for r in rows]


def write_report(path=None):
    path = path or REPORT
    if TABLE and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("worst row per (case, optimiser) over the case's steps and tensors; bound = 3 * e_32 + u, ratio = e_dev / bound\n")
            f.write("(rows tagged 'moments': exp_avg / exp_avg_sq at the end of the case)\n")
            f.write(HEADER + "\n" + "\n".join(format_rows(TABLE)) + "\n")


# ------------------------------------------------------------------------------------------------ the checker
class UpdateChecker:
    """`chk.step(batch)` = `before_step()`, `trainer.step(batch)`, `after_step()`; `finish()` at the end of the case.

    trainer_like: `.opt`, `.model`, `.discriminator` (networks), the optimisers under the attribute names RECIPE's tags
    give (`optimizer`, `optimizer_converse` on the trainer; `optimizer_d_*` on the discriminator), `.step(batch)`.
    `structure=False` leaves out the param-group checks (the planted-fault tests show that the arithmetic alone rejects a
    wrong rate).  Violations of one step are collected and raised together at the end of `after_step` / `finish`, after the
    figures have been recorded; `ratio` is the worst e_dev / (3 e_32 + u) of the last step."""

    def __init__(self, trainer_like, case="", structure=True):
        self.tr, self.case = trainer_like, case
        self.named = named_tensors(trainer_like)
        self.names = {id(p): n for n, p in self.named}
        self.hyper = {n: recipe(n, trainer_like.opt) for n, _ in self.named}
        self.st64 = {n: {} for n, _ in self.named}
        self.p32 = {n: torch.zeros(p.shape, dtype=torch.float32, requires_grad=True) for n, p in self.named}
        self.opt32 = {}
        for n, _ in self.named:
            _, lr, b1, b2, eps = self.hyper[n]
            self.opt32[n] = torch.optim.Adam([self.p32[n]], lr=lr, betas=(b1, b2), eps=eps, foreach=False, fused=False)
        self.expected_steps = {n: 0 for n, _ in self.named}
        self.worst = {}                  # optimiser tag -> (ratio, e_dev, e_32, u, tensor)
        self.steps, self.ratio, self.before = 0, 0.0, None
        if structure:
            self.check_structure()

    # ---- who owns what
    def check_structure(self):
        """Every parameter of every network sits in exactly one param group of exactly one optimiser — the one RECIPE names,
        with RECIPE's rate, betas and eps — and the transitive weights are one tensor under all of their names."""
        bad, owners = [], {}
        for tag, o in optimizers_of(self.tr).items():
            for gi, g in enumerate(o.param_groups):
                for p in g["params"]:
                    owners.setdefault(id(p), []).append((tag, gi, g))
        for n, p in self.named:
            own = owners.pop(id(p), [])
            if len(own) != 1:
                bad.append("%s sits in %d param groups (%s)" % (n, len(own), [(t, gi) for t, gi, _ in own]))
                continue
            tag, _, g = own[0]
            want = self.hyper[n]
            got = (tag, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]))
            if got != want or g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
                bad.append("%s: optimiser %r, recipe %r" % (n, got, want))
        if owners:
            bad.append("%d optimiser entries are parameters of no network" % len(owners))
        aliases = [(n, p) for net in (self.tr.model, self.tr.discriminator) for n, p in net.named_parameters(remove_duplicate=False)
                   if n.endswith("predicates_transitive_weights") or n.endswith("trans_candidates_weights")]
        first = dict(self.named).get(TRANS)
        if aliases and (first is None or any(p is not first for _, p in aliases)):
            bad.append("the transitive weights are not ONE tensor: %s" % [n for n, _ in aliases])
        assert not bad, "%s: optimiser structure\n%s" % (self.case, "\n".join(bad[:20]))

    # ---- twins
    def seed(self, tag, state_dict):
        """Start the twins of optimiser `tag` from a checkpointed `optimizer.state_dict()` (entries are positional: the
        k-th parameter over the param groups, as `load_state_dict` reads them)."""
        params = [p for g in optimizers_of(self.tr)[tag].param_groups for p in g["params"]]
        index = [i for g in state_dict["param_groups"] for i in g["params"]]
        assert len(index) == len(params)
        for i, p in zip(index, params):
            st = state_dict["state"].get(i)
            if not st:
                continue
            n = self.names[id(p)]
            t = int(round(float(st["step"])))
            m, v = st["exp_avg"].detach().cpu(), st["exp_avg_sq"].detach().cpu()
            self.st64[n] = {"t": t, "m": m.double(), "v": v.double()}
            self._note_tops(n)
            self.opt32[n].state[self.p32[n]] = {"step": torch.tensor(float(t)), "exp_avg": m.float().clone(),
                                                "exp_avg_sq": v.float().clone()}
            self.expected_steps[n] = t

    def _note_tops(self, n):
        """The largest magnitude each moment of tensor `n` has had so far in the case (see `finish`)."""
        st = self.st64[n]
        for k in ("m", "v"):
            st[k + "_top"] = max(st.get(k + "_top", 0.0), float(st[k].abs().max()))

    def scale_lr(self, factor):
        """The twins follow a learning-rate edit of every group."""
        for n in self.hyper:
            tag, lr, b1, b2, eps = self.hyper[n]
            self.hyper[n] = (tag, lr * factor, b1, b2, eps)
            for g in self.opt32[n].param_groups:
                g["lr"] = lr * factor

    # ---- one step
    def before_step(self):
        _sync(self.tr)
        self.before = {n: p.detach().clone() for n, p in self.named}

    def step(self, batch):
        self.before_step()
        out = self.tr.step(batch)
        self.after_step()
        return out

    def after_step(self):
        _sync(self.tr)
        self.steps += 1
        self.ratio = 0.0
        bad = []
        states = {}
        for tag, o in optimizers_of(self.tr).items():
            for g in o.param_groups:
                for p in g["params"]:
                    states[id(p)] = o.state.get(p)
        for n, p in self.named:
            before = self.before[n]
            grad = p.grad
            if grad is None:
                if not torch.equal(p.detach(), before):
                    bad.append("%s has no gradient and changed (max |dp| %.3e)" % (n, float((p.detach() - before).abs().max())))
                    self.ratio = float("inf")
                st = states.get(id(p))
                if st and not self.expected_steps[n]:
                    bad.append("%s never had a gradient but has optimiser state" % n)
                elif st and float(st["step"]) != float(self.expected_steps[n]):         # skipped: t stays untouched too
                    bad.append("%s has no gradient in this step and its counter moved to %g" % (n, float(st["step"])))
                continue
            tag = self.hyper[n][0]
            b_cpu, g_cpu = before.cpu(), grad.detach().cpu()
            p64 = adam64(self.st64[n], b_cpu, g_cpu, self.hyper[n][1:])
            self._note_tops(n)
            p32 = self.p32[n]
            with torch.no_grad():
                p32.copy_(b_cpu)
            p32.grad = g_cpu.float().clone()
            self.opt32[n].step()
            self.expected_steps[n] += 1
            e_dev = float((p.detach().cpu().double() - p64).abs().max())
            e_32 = float((p32.detach().double() - p64).abs().max())
            u = ulp32(b_cpu.abs().max())
            bound = K * e_32 + u
            ratio = e_dev / bound
            self.ratio = max(self.ratio, ratio)
            if ratio > self.worst.get(tag, (-1.0,))[0]:
                self.worst[tag] = (ratio, e_dev, e_32, u, "step %d %s" % (self.steps, n))
            if not e_dev <= bound:
                bad.append("step %d %s [%s]: e_dev %.3e > 3 * e_32 %.3e + u %.3e (ratio %.1f)" % (self.steps, n, tag, e_dev, e_32, u, ratio))
        assert not bad, "%s: %d violations\n%s" % (self.case, len(bad), "\n".join(bad[:20]))

    # ---- end of a case
    def finish(self):
        """Step counters and moments of every optimiser against the twins'; the case's rows go into TABLE.

        Moments: e_dev <= 3 e_32 + u like the parameters, with u one fp32 ulp of the largest magnitude the moment has had during
        the case.  The moments are never re-synchronised, so the rounding of the step at which a moment was largest is still in
        it at the end (decayed by one beta per step, 0.9 or 0.999): where the gradients shrink during a case — tensors whose
        gradient is rounding noise — one ulp of the FINAL magnitude would be below the rounding any fp32 Adam has made."""
        _sync(self.tr)
        bad = []
        worst_m = {}
        owner = {}
        for tag, o in optimizers_of(self.tr).items():
            for g in o.param_groups:
                for p in g["params"]:
                    owner[id(p)] = o
        for n, p in self.named:
            want = self.expected_steps[n]
            o = owner.get(id(p))
            st = o.state.get(p) if o is not None else None
            if want == 0:
                if st:
                    bad.append("%s never had a gradient but has optimiser state" % n)
                continue
            if not st or "step" not in st:
                bad.append("%s had a gradient in %d steps and has no optimiser state" % (n, want))
                continue
            if float(st["step"]) != float(want):
                bad.append("%s: step counter %g, %d steps with a gradient" % (n, float(st["step"]), want))
            tag = self.hyper[n][0]
            tw = self.opt32[n].state[self.p32[n]]
            for key, k64 in (("exp_avg", "m"), ("exp_avg_sq", "v")):
                ref = self.st64[n][k64]
                e_dev = float((st[key].detach().cpu().double() - ref).abs().max())
                e_32 = float((tw[key].double() - ref).abs().max())
                u = ulp32(self.st64[n][k64 + "_top"])
                ratio = e_dev / (K * e_32 + u)
                if ratio > worst_m.get(tag, (-1.0,))[0]:
                    worst_m[tag] = (ratio, e_dev, e_32, u, "%s of %s" % (key, n))
                if not e_dev <= K * e_32 + u:
                    bad.append("%s %s [%s]: e_dev %.3e > 3 * e_32 %.3e + u %.3e" % (n, key, tag, e_dev, e_32, u))
        if TRANS in self.expected_steps and self.expected_steps[TRANS]:
            # one tensor under six names: stepped once per iteration, not once per name
            st = owner[id(dict(self.named)[TRANS])].state[dict(self.named)[TRANS]]
            if float(st["step"]) != float(self.expected_steps[TRANS]):
                bad.append("the transitive weights were stepped %g times in %d iterations" % (float(st["step"]), self.expected_steps[TRANS]))
        rows = [(self.case, tag, w[1], w[2], w[3], w[0], w[4]) for tag, w in sorted(self.worst.items())]
        rows += [(self.case + " moments", tag, w[1], w[2], w[3], w[0], w[4]) for tag, w in sorted(worst_m.items())]
        TABLE.extend(rows)
        print("\n".join([HEADER] + format_rows(rows)))
        assert not bad, "%s: %d violations at the end of the case\n%s" % (self.case, len(bad), "\n".join(bad[:20]))
        return rows
