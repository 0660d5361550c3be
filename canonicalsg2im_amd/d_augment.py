"""Differentiable augmentation of everything the discriminators see (DiffAugment, Zhao et al., NeurIPS 2020), opt-in:
`--d_augment color,translation,cutout` (any subset; empty = off), `--d_augment_seed N`.

`DAugment` owns the seed, the iteration counter, the policy mask and the PERSISTENT parameter table of the three PatchGAN
passes.  There is no RNG state: a sample's parameters are a counter-based hash of (seed, iteration, pass, rank << 32 | n)
(csrc/csg_augment.h), so a run restored from a checkpoint continues the parameter stream and N ranks draw different
transforms.  The passes:

    0  PatchGAN in the generator update, fake AND real: feature matching compares the two, they must see one transform
    1  PatchGAN on the fake picture in the discriminator update
    2  PatchGAN on the real picture in the discriminator update (the logged wrong-layout pass reuses it)
    3  crops in the generator update        4  fake crops in the discriminator update        5  real crops there

`Trainer.step` calls `begin_step()` at the top of every iteration, before either of its paths runs: the counter advances
and the tables of passes 0-2 are refilled by three eager launches on the current stream.  The table is allocated once and
its address never changes; the transform kernels read their parameters only from it and the policy is a launch constant,
so the PatchGAN passes stay inside the captured HIP graphs (graphs.py; the policy is part of the shape key).  The crop
tables have a data-dependent number of rows and are filled where the crops are made, in the eager part of the step.

Augmentation is active only between `begin_step()` and `end_step()`: validation, the samplers and anything else that
calls the discriminators sees raw inputs.  Left alone on purpose: the mask discriminator is not augmented, the VGG term
compares raw pictures, and the crops kept for display are the raw ones.

ADAPTIVE STRENGTH (StyleGAN2-ADA, Karras et al., NeurIPS 2020), opt-in on top of the policies: `--d_augment_p P`,
`--d_augment_target T`, `--d_augment_interval K`, `--d_augment_kimg M`.  With any of the four the run is GATED: every policy
is applied to a sample with probability p = p24 / 2^24, decided by three more draws of the sample's hash (8, 9, 10), and
`DAugment` also owns the controller record — eight int64 device words [p24, S, C, updates, S_last, C_last, 0, 0] whose address
never changes — and one persistent (3, rows) int32 gate allocation beside the tables.  `begin_step()` fills the gates by
launches that read p24 from the record ON THE DEVICE; the transform kernels read gate[n] like a table row.  T = 0 keeps p
fixed at P (default 1).  0 < T < 1 makes p ADAPTIVE (P defaults to 0): the real pass of the discriminator update (pass 2,
not the logged wrong-layout pass) adds sign(D(real)) over every element of every PatchGAN scale's prediction map to (S, C)
— inside the captured graph on a replayed step —, and after every K completed iterations `begin_step()` launches the
one-thread update: p24 moves by step24 = max(1, round(batch_size world_size K 2^24 / (1000 M))) towards r_t = S / C = T, up
when r_t > T (the discriminator is too sure of the real pictures), down when r_t < T, clamped to [0, 2^24].  With N > 1 ranks
(S, C) is summed over the ranks first (one int64 all-reduce), so every rank holds the same p.  Nothing is read back during a
step: `read()` (the trainer script's print line, checkpoints) is the only read-back.  Without the four flags there is no
record, no gate, no extra launch: the run is what it was.

THE ADA PIPELINE (StyleGAN2-ADA's own transforms, appendix B of the paper), opt-in by three more policy names:
`ada_blit` (x-flip, rot90, integer translation), `ada_geom` (isotropic scale, pre-rotation, anisotropic scale, post-rotation,
fractional translation) and `ada_color` (brightness, contrast, luma flip, hue rotation, saturation).  Every single transform
is on for a sample with probability p (each of the two rotations with 1 - sqrt(1 - p)), so these names need a strength:
`--d_augment_p` or a non-zero `--d_augment_target` — at p = 1 such transforms leak into the generator, and the flags refuse a
run that would apply them always by default.  The stage is ONE launch (ops.ada_pipeline: an affine resampling with four
bilinear taps and zero fill, then a 3 x 4 colour matrix) that runs BEFORE the DiffAugment kernel when both families are named.
Its parameters are rows of 32 words (csrc/csg_ada_pipeline.h) in one more persistent (3, rows, 32) allocation for passes 0-2,
filled in `begin_step()` after the controller update and beside the gate fills by launches that read p24 on the device; the
crops of passes 3-5 get fresh tables.  The draws are those of the same per-sample key, from index 16 on: naming an `ada_*`
group moves no draw of DiffAugment's rows (1-7) or gates (8-10).  Checkpoints carry the names in `d_augment.policies`,
nothing else.  Deviations from the authors' pipeline (bilinear taps for the wavelet filters, zero fill for reflection, a
bounded normal, clamped scales) are stated in csrc/ada_pipeline.hip; no quality figure is claimed.

This module imports nothing at its top: scripts/args.py checks the flags with `policy_mask` and `ada_settings` without
loading the library.
"""
POLICY_BITS = {"color": 1, "translation": 2, "cutout": 4, "ada_blit": 8, "ada_geom": 16, "ada_color": 32}
DIFF_BITS, ADA_BITS = 7, 56
POLICY_LIST = "color,translation,cutout,ada_blit,ada_geom,ada_color"
PASS_G_IMG, PASS_D_IMG_FAKE, PASS_D_IMG_REAL, PASS_G_OBJ, PASS_D_OBJ_FAKE, PASS_D_OBJ_REAL = range(6)
IMG_PASSES = 3


def policy_mask(policies):
    """The mask (ops.AUG_COLOR | AUG_TRANSLATION | AUG_CUTOUT | AUG_ADA_BLIT | AUG_ADA_GEOM | AUG_ADA_COLOR) of the flag's value:
    a comma list out of color,translation,cutout,ada_blit,ada_geom,ada_color.  '' and None are 0: off.  Anything else is
    refused with a message."""
    if policies is None or policies == "":
        return 0
    if not isinstance(policies, str):
        raise ValueError("d_augment: the policies are a comma list out of %s, got %r" % (POLICY_LIST, policies))
    mask = 0
    for p in (p.strip() for p in policies.split(",")):
        if p not in POLICY_BITS:
            raise ValueError("d_augment: unknown policy %r (a comma list out of %s)" % (p, POLICY_LIST))
        mask |= POLICY_BITS[p]
    return mask


def policy_names(mask):
    return ",".join(n for n, b in POLICY_BITS.items() if mask & b)


ADA_ONE = 1 << 24
ADA_FLAGS = ("d_augment_p", "d_augment_target", "d_augment_interval", "d_augment_kimg")
ADA_DEFAULTS = {"d_augment_target": 0.0, "d_augment_interval": 4, "d_augment_kimg": 500.0}


def step24_of(batch_size, world_size, interval, kimg):
    """max(1, round(batch_size * world_size * interval * 2^24 / (1000 * kimg))), halves rounded up, in exact arithmetic.
    `batch_size` is the PER-RANK batch: batch_size * world_size is the number of pictures all ranks see in one iteration."""
    from fractions import Fraction
    x = Fraction(int(batch_size) * int(world_size) * int(interval) * ADA_ONE) / (1000 * Fraction(kimg))
    return max(1, int(x + Fraction(1, 2)))          # (int() floors a positive Fraction)


def ada_settings(p=None, target=None, interval=None, kimg=None, policies=""):
    """The four flags, checked together.  None when none is given (the ungated run); else {"p24", "T24", "interval", "kimg",
    "adaptive"} with the defaults filled in.  Refused with a message: a flag without policies, P outside [0, 1], T outside
    {0} | (0, 1), K < 1, M <= 0."""
    import math
    given = {"--d_augment_p": p, "--d_augment_target": target, "--d_augment_interval": interval, "--d_augment_kimg": kimg}
    given = {k: v for k, v in given.items() if v is not None}
    mask = policy_mask(policies)
    if mask & ADA_BITS and "--d_augment_p" not in given and not (target is not None and float(target) != 0.0):
        raise ValueError("d_augment: the policies %s need a strength: give --d_augment_p P or a non-zero --d_augment_target "
                         "(every ADA transform is applied with probability p; at p = 1 these transforms leak into the "
                         "generator, so there is no default)" % policy_names(mask & ADA_BITS))
    if not given:
        return None
    if not policy_mask(policies):
        raise ValueError("d_augment: %s without --d_augment policies: there is nothing to gate (give --d_augment a comma list "
                         "out of %s)" % (", ".join(sorted(given)), POLICY_LIST))
    target = ADA_DEFAULTS["d_augment_target"] if target is None else float(target)
    if not (target == 0.0 or 0.0 < target < 1.0):
        raise ValueError("d_augment: --d_augment_target must be 0 (a fixed p) or in (0, 1), got %r" % (target,))
    T24 = int(math.floor(target * ADA_ONE + 0.5))
    if target and not 0 < T24 < ADA_ONE:
        raise ValueError("d_augment: --d_augment_target %r is not in (0, 1) in units of 2^-24" % (target,))
    adaptive = T24 > 0
    p = (0.0 if adaptive else 1.0) if p is None else float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("d_augment: --d_augment_p must be in [0, 1], got %r" % (p,))
    interval = ADA_DEFAULTS["d_augment_interval"] if interval is None else interval
    if not isinstance(interval, int) or isinstance(interval, bool) or interval < 1:
        raise ValueError("d_augment: --d_augment_interval must be an integer >= 1, got %r" % (interval,))
    kimg = ADA_DEFAULTS["d_augment_kimg"] if kimg is None else float(kimg)
    if not (kimg > 0.0 and kimg < float("inf")):
        raise ValueError("d_augment: --d_augment_kimg must be a positive number, got %r" % (kimg,))
    return {"p24": int(math.floor(p * ADA_ONE + 0.5)), "T24": T24, "interval": interval, "kimg": kimg, "adaptive": adaptive}


def ada_settings_of(opt):
    """`ada_settings` of a namespace; one made before the flags existed has none of them: None."""
    return ada_settings(*(getattr(opt, f, None) for f in ADA_FLAGS), policies=getattr(opt, "d_augment", "") or "")


def check_seed(seed):
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 64:
        raise ValueError("d_augment: the seed must be an integer in [0, 2^64), got %r" % (seed,))
    return seed


class DAugment:
    def __init__(self, policies, seed, device, batch_size, image_size, rank=0, ada=None, world_size=1):
        """`ada`: what `ada_settings` returns; None is the ungated run.  `batch_size` sizes the tables and is taken as the
        per-rank batch in step24 (what `opt.batch_size` is under bench.py and in the tests); a caller whose `--batch_size` is the
        global batch (scripts/train.py) says so with `set_pictures_per_iteration`."""
        import torch
        self.policy = policy_mask(policies)
        if not self.policy:
            raise ValueError("DAugment: no policy (an empty --d_augment means off and never reaches this class)")
        self.seed, self.rank, self.device = check_seed(seed), int(rank), device
        self.iteration = 0
        self.active = False
        self.image_size, self.rows = int(image_size), max(int(batch_size), 1)
        # ONE allocation for the three PatchGAN passes; a captured graph keeps its address
        self.tables = torch.zeros((IMG_PASSES, self.rows, 8), dtype=torch.int32, device=device)
        self.ada = None if ada is None else dict(ada)
        self.gated = ada is not None
        self.adaptive = bool(self.gated and ada["adaptive"])
        self.ctrl = self.gates = self.ada_tables = None
        self.diff_policy, self.ada_policy = self.policy & DIFF_BITS, self.policy & ADA_BITS
        if self.ada_policy and not self.gated:
            raise ValueError("DAugment: the policies %s need the strength settings (`ada_settings`)" % policy_names(self.ada_policy))
        if self.gated:
            self.set_pictures_per_iteration(max(int(batch_size), 1) * max(int(world_size), 1))
            self.ctrl = torch.zeros(8, dtype=torch.int64, device=device)        # persistent: captured graphs add to it
            self.ctrl[0] = ada["p24"]
            self.gates = torch.zeros((IMG_PASSES, self.rows), dtype=torch.int32, device=device)
            if self.ada_policy:                  # ONE more allocation: the ADA pipeline's rows of the three PatchGAN passes
                self.ada_tables = torch.zeros((IMG_PASSES, self.rows, 32), dtype=torch.int32, device=device)

    def set_pictures_per_iteration(self, n):
        """step24 for n pictures per iteration over ALL ranks: p can then cross [0, 1] in `kimg` thousand pictures."""
        if self.gated:
            self.pictures_per_iteration = int(n)
            self.step24 = step24_of(int(n), 1, self.ada["interval"], self.ada["kimg"])

    # ------------------------------------------------------------------ the step
    def begin_step(self):
        from . import ops
        if self.adaptive and self.iteration > 0 and self.iteration % self.ada["interval"] == 0:
            # K iterations have added to (S, C) since the last update: one launch moves p24 before this iteration's gates
            self._reduce_counts()
            ops.ada_update(self.ctrl, self.ada["T24"], self.step24)
        self.iteration += 1
        for p in range(IMG_PASSES):
            ops.augment_table(self.seed, self.iteration, p, self.rows, self.image_size, rank=self.rank, out=self.tables[p])
            if self.gated:
                ops.augment_gate(self.seed, self.iteration, p, self.rows, self.ctrl, rank=self.rank, out=self.gates[p])
            if self.ada_policy:
                ops.ada_pipeline_table(self.seed, self.iteration, p, self.rows, self.image_size, self.ada_policy, self.ctrl,
                                       rank=self.rank, out=self.ada_tables[p])
        self.active = True

    def _reduce_counts(self):
        """(N > 1 ranks) one int64 SUM all-reduce of (S, C), in place: every rank then computes the same p24."""
        from . import dist as csg_dist
        if csg_dist.active():
            import torch
            torch.distributed.all_reduce(self.ctrl[1:3], op=torch.distributed.ReduceOp.SUM)
            csg_dist.comm_note("ada_allreduce", 16)

    def end_step(self):
        self.active = False

    def operands(self, pass_id, n, size):
        """(table, gate, ada_table) of pass `pass_id` for n samples of size x size; what the run does not use is None.
        PatchGAN pass 0, 1 or 2: the persistent ones (all their rows: the kernels read the first n).  Crop pass 3, 4 or 5:
        fresh ones of n rows, one eager launch each on the current stream."""
        from . import ops
        if not 0 <= pass_id < 6:
            raise ValueError("DAugment.operands: pass %r (0 .. 5)" % (pass_id,))
        if pass_id < IMG_PASSES:
            if n > self.rows:
                raise RuntimeError("DAugment: a batch of %d pictures, the tables were made for --batch_size %d" % (n, self.rows))
            return (self.tables[pass_id] if self.diff_policy else None,
                    self.gates[pass_id] if self.diff_policy and self.gated else None,
                    self.ada_tables[pass_id] if self.ada_policy else None)
        ada_table = table = gate = None
        if self.ada_policy:
            ada_table = ops.ada_pipeline_table(self.seed, self.iteration, pass_id, n, size, self.ada_policy, self.ctrl,
                                               rank=self.rank)
        if self.diff_policy:
            table = self.crop_table(pass_id, n, size)
            gate = self.crop_gate(pass_id, n) if self.gated else None
        return table, gate, ada_table

    def crop_table(self, pass_id, n, size):
        """A fresh table of n rows for crops of size x size (pass 3, 4 or 5): one eager launch on the current stream."""
        from . import ops
        return ops.augment_table(self.seed, self.iteration, pass_id, n, size, rank=self.rank, device=self.device)

    def crop_gate(self, pass_id, n):
        """A fresh gate of n rows for the crops of pass 3, 4 or 5 (gated runs): one eager launch beside the crop table's."""
        from . import ops
        return ops.augment_gate(self.seed, self.iteration, pass_id, n, self.ctrl, rank=self.rank)

    def observe_real(self, scales):
        """The real pass of the discriminator update hands over what the PatchGAN returned (one entry per scale, the
        prediction map last): on an adaptive run inside a training step, one launch adds its signs to (S, C)."""
        if not (self.adaptive and self.active):
            return
        from . import ops
        ops.ada_accumulate([s[-1] if isinstance(s, (list, tuple)) else s for s in scales], self.ctrl)

    def read(self):
        """The controller's words, read back (a synchronisation: for the print line and for checkpoints, never in a step):
        {"p24", "S", "C", "updates", "S_last", "C_last", "p", "r_t"}; r_t = S_last / C_last, nan before the first update."""
        w = [int(v) for v in self.ctrl.tolist()]
        return {"p24": w[0], "S": w[1], "C": w[2], "updates": w[3], "S_last": w[4], "C_last": w[5], "p": w[0] / ADA_ONE,
                "r_t": w[4] / w[5] if w[5] else float("nan")}

    def apply(self, x, pass_id, c0):
        """x augmented as pass `pass_id` (the PatchGAN's packed input with c0 = S, or the crops with c0 = 0) while a training
        step is running; x itself otherwise."""
        from . import ops
        if not self.active or pass_id is None or x.shape[0] == 0:
            return x
        table, gate, ada_table = self.operands(pass_id, x.shape[0], x.shape[2])
        if self.ada_policy:                      # the ADA stage first, one launch; DiffAugment then runs on its output
            x = ops.ada_pipeline(x, ada_table, c0)
        if self.diff_policy:
            x = ops.d_augment(x, table, c0, self.diff_policy, gate=gate)
        return x

    # ------------------------------------------------------------------ checkpoints
    def _ada_meta(self):
        return {k: self.ada[k] for k in ("p24", "T24", "interval", "kimg")}

    def meta(self):
        out = {"seed": self.seed, "iteration": self.iteration, "policies": policy_names(self.policy)}
        if self.gated:                           # (ungated: exactly the keys above)
            out["ctrl"] = [int(v) for v in self.ctrl.tolist()]
            out["ada"] = self._ada_meta()
        return out

    def load_meta(self, meta, say=print):
        """Continue the parameter stream of a checkpoint: its iteration counter; 0 without the entry.  This run's policies and
        seed hold; one printed line says so when the checkpoint's differ."""
        if self.gated:
            # An adaptive run continues the record's words: p24, the update count and — on one rank, exactly — S and C.  A
            # checkpoint without them (an ungated run's, or one from before the record existed) starts from this run's flags,
            # and so does every fixed-p run (T = 0): there the record holds nothing but p, and this run's --d_augment_p holds as
            # its policies and seed do.  With N > 1 ranks the checkpoint holds RANK 0's counts since the last update (only rank
            # 0 writes it, and S, C are per rank until the update's all-reduce): rank 0 alone keeps them, the other ranks
            # start the interval at 0, so the first update after a resume sees rank 0's part of that interval, not N copies
            # of it.  Written in place: captured graphs keep the address.
            import torch
            from . import dist as csg_dist
            words = (meta or {}).get("ctrl") if self.adaptive else None
            if words is None:
                words = [self.ada["p24"]] + [0] * 7
            words = [int(v) for v in words]
            if csg_dist.rank() != 0:
                words[1] = words[2] = 0
            self.ctrl.copy_(torch.tensor([int(v) for v in words], dtype=torch.int64))
            theirs_ada = (meta or {}).get("ada")
            mine = self._ada_meta()
            if theirs_ada is not None and theirs_ada != mine:
                say("d_augment: the checkpoint was written with the settings %s; this run's hold: %s (p24 = %d continues)" % (
                    theirs_ada, mine, int(words[0])))
        if not meta:
            self.iteration = 0
            return
        self.iteration = int(meta.get("iteration", 0))
        theirs = (policy_mask(meta.get("policies", "")), meta.get("seed", 0))
        if theirs != (self.policy, self.seed):
            say("d_augment: the checkpoint was written with policies '%s' and seed %s; this run's hold: policies '%s', seed %d "
                "(iteration %d continues)" % (policy_names(theirs[0]), theirs[1], policy_names(self.policy), self.seed,
                                              self.iteration))
