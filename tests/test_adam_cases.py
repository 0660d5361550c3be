"""tests/adam_cases.py proves itself on the host: the fp64 restatement against torch's own fp64 Adam, `UpdateChecker` on a
clean run and on eleven planted faults (the nine kinds, two of them both ways), and RECIPE against the committed oracle's optimisers.

The "device" is a small CPU trainer with the networks' names and every optimiser of the recipe; its step takes its gradients
from a seeded sequence (element magnitudes 1e-20 ... 1 inside every tensor, another overall scale at every step, one tensor
without a gradient at step 3, one tensor that never has one) and runs its optimisers."""
import types
import zlib

import pytest
import torch
import torch.nn as nn

import adam_cases as ac

STEPS = 6
SCALES = [1.0, 0.1, 3.0, 0.01, 1.0, 0.3]        # the gradients' overall magnitude varies from step to step: with a constant one
#                                                 m / sqrt(v) stays 1 for any betas and half of the faults would be invisible
SKIPPED = ("layout_to_image_model.module.fc.bias", 3)      # (tensor, step) without a gradient
NEVER = "layout_to_image_model.module.unused"               # a tensor no loss reaches


def _opt(**kw):
    base = dict(learning_rate=3e-4, img_learning_rate=2e-4, mask_learning_rate=5e-5, beta1=0.6)
    base.update(kw)
    return types.SimpleNamespace(**base)


class _Wrapped(nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module


class _Layer(nn.Module):
    def __init__(self, shared):
        super().__init__()
        self.predicates_transitive_weights = shared
        self.net = nn.Linear(5, 3)


class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.trans_candidates_weights = nn.Parameter(torch.empty(7).uniform_(-0.5, 0.5))
        self.converse_candidates_weights = nn.Parameter(torch.empty(7, 7).uniform_(-0.5, 0.5))
        self.gconvs = nn.ModuleList(_Layer(self.trans_candidates_weights) for _ in range(5))     # six names in all
        self.box_net = nn.Linear(6, 4)


class _Generator(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(33, 17)
        self.conv = nn.Conv2d(4, 6, 3)
        self.unused = nn.Parameter(torch.empty(9).uniform_(-0.5, 0.5))


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        self.sg_to_layout = _Wrapped(_Encoder())
        self.layout_to_image_model = _Wrapped(_Generator())


class _Discriminator(nn.Module):
    def __init__(self):
        super().__init__()
        self.img_discriminator = nn.Sequential(nn.Conv2d(3, 8, 4), nn.Conv2d(8, 1, 4))
        self.obj_discriminator = nn.Sequential(nn.Linear(19, 11), nn.Linear(11, 1))
        self.mask_discriminator = nn.Sequential(nn.Conv2d(1, 4, 3))


class ManualAdam(torch.optim.Optimizer):
    """Adam written out in fp32, operation by operation as the formula reads (another order of operations than torch's), with
    switches for the faults torch's own Adam cannot be talked into."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, bias_correction=True, eps_in_sqrt=False, advance=True):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self.bias_correction, self.eps_in_sqrt, self.advance = bias_correction, eps_in_sqrt, advance

    @torch.no_grad()
    def step(self):
        for g in self.param_groups:
            b1, b2 = g["betas"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"], st["exp_avg"], st["exp_avg_sq"] = torch.tensor(0.0), torch.zeros_like(p), torch.zeros_like(p)
                if self.advance or float(st["step"]) == 0:
                    st["step"] += 1
                t = float(st["step"])
                st["exp_avg"].lerp_(p.grad, 1 - b1)                 # (the moments as torch forms them; the update below is not)
                st["exp_avg_sq"].mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                c1, c2 = (1 - b1 ** t, 1 - b2 ** t) if self.bias_correction else (1.0, 1.0)
                if self.eps_in_sqrt:
                    denom = (st["exp_avg_sq"] / c2 + g["eps"]).sqrt()
                else:
                    denom = st["exp_avg_sq"].sqrt() / (c2 ** 0.5) + g["eps"]
                p.sub_(g["lr"] / c1 * st["exp_avg"] / denom)


class HostTrainer:
    """The trainer's surface on the CPU: networks, the recipe's optimisers, `step(k)`.  `fault` plants one mistake."""

    def __init__(self, fault=None, adam=None, seed=0, dtype=torch.float32):
        torch.manual_seed(seed)
        self.opt, self.device, self.fault = _opt(), torch.device("cpu"), fault
        self.model, self.discriminator = _Model().to(dtype), _Discriminator().to(dtype)
        o, d = self.opt, self.discriminator
        adam = adam or torch.optim.Adam
        named = dict(self.model.named_parameters())
        trans, conv = named[ac.TRANS], named["sg_to_layout.module.converse_candidates_weights"]
        base = [p for p in named.values() if p is not trans and p is not conv]
        lr, lr_img, lr_trans, b1_g, b1_d, b2 = o.learning_rate, o.img_learning_rate, 1e-2, 0.9, o.beta1, 0.999
        img, obj = list(d.img_discriminator.parameters()), list(d.obj_discriminator.parameters())
        if fault == "beta2":
            b2 = 0.99
        if fault == "beta1_low":
            b1_g = 0.5
        if fault == "beta1_high":
            b1_d = 0.9
        if fault == "lr_swap":
            lr_img = o.learning_rate
        if fault == "lr_swap_trans":
            lr_trans = o.learning_rate
        if fault == "left_out":
            base = base[:-1]
        if fault == "two_groups":
            img = img + obj[:1]
        self.optimizer = adam([{"params": base, "lr": lr}, {"params": [trans], "lr": lr_trans}], lr=lr, betas=(b1_g, b2))
        self.optimizer_converse = adam([{"params": [conv], "lr": 1e-2}], lr=1e-2, betas=(0.9, b2))
        d.optimizer_d_img = adam(img, lr=lr_img, betas=(b1_d, b2))
        d.optimizer_d_obj = adam(obj, lr=o.learning_rate, betas=(b1_d, b2))
        d.optimizer_d_mask = adam(list(d.mask_discriminator.parameters()), lr=o.mask_learning_rate, betas=(b1_d, b2))

    def gradient(self, name, p, k):
        gen = torch.Generator().manual_seed(zlib.crc32(("%s %d" % (name, k)).encode()))
        mag = 10.0 ** torch.empty(p.shape, dtype=torch.float64).uniform_(-20.0, 0.0, generator=gen)
        sign = torch.where(torch.rand(p.shape, generator=gen) < 0.5, -1.0, 1.0).double()
        g = mag * sign * SCALES[k - 1]
        g.view(-1)[0] = SCALES[k - 1] * (1.0 if k % 2 else -0.7)           # the span's upper end in every tensor
        return g.to(p.dtype)

    def step(self, k):
        for n, p in ac.named_tensors(self):
            p.grad = None
            if n != NEVER and (n, k) != SKIPPED:
                p.grad = self.gradient(n, p, k)
        d = self.discriminator
        for o in (self.optimizer, self.optimizer_converse, d.optimizer_d_img, d.optimizer_d_obj, d.optimizer_d_mask):
            o.step()
        if self.fault == "ulp":
            with torch.no_grad():
                q = dict(self.model.named_parameters())[NEVER]
                q[3] = torch.nextafter(q[3], torch.tensor(float("inf"), dtype=q.dtype))


def test_six_names_one_tensor():
    names = [n for n, _ in _Model().named_parameters(remove_duplicate=False) if "trans" in n]
    assert len(names) == 6


def test_adam64_agrees_with_torch_fp64_adam():
    """adam64 against torch.optim.Adam run in fp64: parameters, moments and step counts over six steps (a step without a
    gradient, a tensor that never has one, gradients spanning 1e-20 ... 1) to 1e-14 relative."""
    tr = HostTrainer(dtype=torch.float64)
    named = ac.named_tensors(tr)
    states = {n: {} for n, _ in named}
    hyper = {n: ac.recipe(n, tr.opt) for n, _ in named}
    owners = {id(p): o for o in ac.optimizers_of(tr).values() for g in o.param_groups for p in g["params"]}
    worst = 0.0
    for k in range(1, STEPS + 1):
        before = {n: p.detach().clone() for n, p in named}
        tr.step(k)
        for n, p in named:
            mine = ac.adam64(states[n], before[n], p.grad, hyper[n][1:])
            rel = float((mine - p.detach()).abs().max() / p.detach().abs().max())
            worst = max(worst, rel)
            assert rel <= 1e-14, (n, k, rel)
            if p.grad is None:
                assert torch.equal(p.detach(), before[n]) and torch.equal(mine, before[n])
    for n, p in named:
        st = owners[id(p)].state.get(p)
        if n == NEVER:
            assert not st and states[n] == {}
            continue
        assert float(st["step"]) == states[n]["t"] == (STEPS - 1 if n == SKIPPED[0] else STEPS)
        for key, k64 in (("exp_avg", "m"), ("exp_avg_sq", "v")):
            rel = float((st[key] - states[n][k64]).abs().max() / states[n][k64].abs().max())
            worst = max(worst, rel)
            assert rel <= 1e-14, (n, key, rel)
        v, v64 = st["exp_avg_sq"], states[n]["v"]                   # (no cancellation in v: every element, down to 1e-40)
        assert float(((v - v64).abs() / v64.clamp_min(1e-300)).max()) <= 1e-14
    print("adam64 vs torch fp64 Adam: worst relative difference %.2e" % worst)


@pytest.mark.parametrize("device_adam", ["torch", "torch_foreach", "manual"])
def test_checker_passes_on_a_clean_run(device_adam):
    """The clean fp32 run, stepped by torch's CPU Adam (single-tensor and multi-tensor) and by the same formula in another
    order of operations: every step inside 3 e_32 + u, counters and moments right at the end."""
    adam = {"torch": None, "torch_foreach": lambda *a, **k: torch.optim.Adam(*a, foreach=True, **k), "manual": ManualAdam}[device_adam]
    tr = HostTrainer(adam=adam)
    chk = ac.UpdateChecker(tr, "host clean " + device_adam)
    for k in range(1, STEPS + 1):
        chk.step(k)
        print("step %d: worst e_dev / (3 e_32 + u) = %.3f" % (k, chk.ratio))
    rows = chk.finish()
    assert {r[1] for r in rows} == {"optimizer", "optimizer_converse", "optimizer_d_img", "optimizer_d_obj", "optimizer_d_mask"}
    assert chk.expected_steps[NEVER] == 0 and chk.expected_steps[SKIPPED[0]] == STEPS - 1 and chk.expected_steps[ac.TRANS] == STEPS
    del ac.TABLE[-len(rows):]                                        # (the report is the device's)


FAULTS = {
    # name: (HostTrainer fault, ManualAdam switches, the param-group check sees it too, finish() sees it too)
    "beta2 is 0.99": ("beta2", None, True, True),
    "beta1 is 0.5 where 0.9 is due": ("beta1_low", None, True, True),
    "beta1 is 0.9 where 0.6 is due": ("beta1_high", None, True, True),
    "the image discriminator steps at the generator's rate": ("lr_swap", None, True, False),
    "the transitive weights step at the base group's rate": ("lr_swap_trans", None, True, False),
    "no bias correction": (None, dict(bias_correction=False), False, False),
    "eps inside the square root": (None, dict(eps_in_sqrt=True), False, False),
    "the step counter is not advanced": (None, dict(advance=False), False, True),
    "a parameter is left out of the optimiser": ("left_out", None, True, True),
    "a parameter sits in two groups": ("two_groups", None, True, False),
    "a gradient-less parameter is perturbed by 1 ulp": ("ulp", None, False, False),
}


@pytest.mark.parametrize("name", list(FAULTS))
def test_checker_rejects_planted_fault(name):
    """One fault at a time in the "device" optimiser: the per-step rule raises, and by the last step the fault is at least
    10x beyond the bound (the ratio is printed).  The arithmetic is judged with the param-group check off, so a wrong rate
    or beta is shown to be caught by what the parameters do, not only by what the groups say."""
    fault, switches, structural, at_finish = FAULTS[name]
    adam = (lambda *a, **k: ManualAdam(*a, **switches, **k)) if switches else None
    tr = HostTrainer(fault=fault, adam=adam)
    if structural:
        with pytest.raises(AssertionError, match="optimiser structure"):
            ac.UpdateChecker(HostTrainer(fault=fault, adam=adam), name)
    chk = ac.UpdateChecker(tr, name, structure=False)
    raised = []
    for k in range(1, STEPS + 1):
        try:
            chk.step(k)
        except AssertionError:
            raised.append(k)
    print("%-58s raised at steps %s; e_dev / (3 e_32 + u) at the last step: %.3g" % (name, raised, chk.ratio))
    assert STEPS in raised, "the checker let the last step pass"
    assert chk.ratio >= 10.0, "margin %.3g" % chk.ratio
    n = len(ac.TABLE)
    if at_finish:
        with pytest.raises(AssertionError, match="at the end of the case"):
            chk.finish()
    else:
        chk.finish()
    del ac.TABLE[n:]


def test_recipe_agrees_with_the_oracle():
    """RECIPE (restated from the reference's scripts/train.py and sg2im/meta_models.py) against the committed oracle's own
    optimisers (`oracle.TrainState`, restated from the same lines by other hands): rate, betas and eps of every tensor, with
    every option at a value of its own, and every tensor of the oracle in exactly one group."""
    import oracle
    from canonicalsg2im_amd import train as T
    from canonicalsg2im_amd.synth import make_vocab
    opt = T.make_opt(make_vocab("tiny"), ["--image_size", "64,64", "--ngf", "4", "--ndf", "8", "--gconv_dim", "32",
                                          "--gconv_hidden_dim", "64", "--gconv_num_layers", "2", "--embedding_dim", "8",
                                          "--no_vgg_loss", "--batch_size", "2", "--mask_size", "16", "--learned_converse", "1",
                                          "--learning_rate", "3e-4", "--img_learning_rate", "2e-4", "--mask_learning_rate", "5e-5",
                                          "--beta1", "0.6"])
    torch.manual_seed(0)
    tr = T.Trainer(opt, torch.device("cpu"))
    ts = T.oracle_state_from(tr, oracle)
    groups = {}
    for tag, o in ac.optimizers_of(ts).items():
        for g in o.param_groups:
            for p in g["params"]:
                groups.setdefault(id(p), []).append((tag, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])))
    assert set(ac.optimizers_of(ts)) == {"optimizer", "optimizer_converse", "optimizer_d_img", "optimizer_d_obj", "optimizer_d_mask"}
    seen, n = set(), 0
    for prefix, state in (("sg_to_layout.module.", ts.sg), ("layout_to_image_model.module.", ts.g), ("img_discriminator.", ts.d),
                          ("obj_discriminator.", ts.dobj), ("mask_discriminator.", ts.dmask)):
        for k, v in state.items():
            if not (torch.is_tensor(v) and v.requires_grad):
                continue
            name = prefix + k
            if k.endswith("predicates_transitive_weights"):          # the shared tensor's other five names
                assert v is ts.sg["trans_candidates_weights"]
                name = ac.TRANS
            assert groups.get(id(v)) == [ac.recipe(name, opt)], (name, groups.get(id(v)), ac.recipe(name, opt))
            seen.add(id(v))
            n += 1
    assert seen == set(groups) and n > 50
    rates = {ac.recipe(name, opt)[:3] for name in ("sg_to_layout.module.box_net.0.weight", ac.TRANS, "img_discriminator.x",
                                                   "obj_discriminator.x", "mask_discriminator.x",
                                                   "sg_to_layout.module.converse_candidates_weights")}
    assert len(rates) == 6
    # and the trainer's own groups, on the host: the same check the device cases run at every construction
    ac.UpdateChecker(tr, "host trainer structure")
