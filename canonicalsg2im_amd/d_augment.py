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

This module imports nothing at its top: scripts/args.py checks the flag with `policy_mask` without loading the library.
"""
POLICY_BITS = {"color": 1, "translation": 2, "cutout": 4}
PASS_G_IMG, PASS_D_IMG_FAKE, PASS_D_IMG_REAL, PASS_G_OBJ, PASS_D_OBJ_FAKE, PASS_D_OBJ_REAL = range(6)
IMG_PASSES = 3


def policy_mask(policies):
    """The mask (ops.AUG_COLOR | AUG_TRANSLATION | AUG_CUTOUT) of the flag's value: a comma list out of
    color,translation,cutout.  '' and None are 0: off.  Anything else is refused with a message."""
    if policies is None or policies == "":
        return 0
    if not isinstance(policies, str):
        raise ValueError("d_augment: the policies are a comma list out of color,translation,cutout, got %r" % (policies,))
    mask = 0
    for p in (p.strip() for p in policies.split(",")):
        if p not in POLICY_BITS:
            raise ValueError("d_augment: unknown policy %r (a comma list out of color,translation,cutout)" % (p,))
        mask |= POLICY_BITS[p]
    return mask


def policy_names(mask):
    return ",".join(n for n, b in POLICY_BITS.items() if mask & b)


def check_seed(seed):
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 64:
        raise ValueError("d_augment: the seed must be an integer in [0, 2^64), got %r" % (seed,))
    return seed


class DAugment:
    def __init__(self, policies, seed, device, batch_size, image_size, rank=0):
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

    # ------------------------------------------------------------------ the step
    def begin_step(self):
        from . import ops
        self.iteration += 1
        for p in range(IMG_PASSES):
            ops.augment_table(self.seed, self.iteration, p, self.rows, self.image_size, rank=self.rank, out=self.tables[p])
        self.active = True

    def end_step(self):
        self.active = False

    def image_table(self, pass_id, n):
        """The persistent table of PatchGAN pass 0, 1 or 2 (all its rows: the kernel reads the first n)."""
        if not 0 <= pass_id < IMG_PASSES:
            raise ValueError("DAugment.image_table: pass %r (0, 1 or 2)" % (pass_id,))
        if n > self.rows:
            raise RuntimeError("DAugment: a batch of %d pictures, the tables were made for --batch_size %d" % (n, self.rows))
        return self.tables[pass_id]

    def crop_table(self, pass_id, n, size):
        """A fresh table of n rows for crops of size x size (pass 3, 4 or 5): one eager launch on the current stream."""
        from . import ops
        if not IMG_PASSES <= pass_id < 6:
            raise ValueError("DAugment.crop_table: pass %r (3, 4 or 5)" % (pass_id,))
        return ops.augment_table(self.seed, self.iteration, pass_id, n, size, rank=self.rank, device=self.device)

    def apply(self, x, pass_id, c0):
        """x augmented as pass `pass_id` (the PatchGAN's packed input with c0 = S, or the crops with c0 = 0) while a training
        step is running; x itself otherwise."""
        from . import ops
        if not self.active or pass_id is None or x.shape[0] == 0:
            return x
        n = x.shape[0]
        table = self.image_table(pass_id, n) if pass_id < IMG_PASSES else self.crop_table(pass_id, n, x.shape[2])
        return ops.d_augment(x, table, c0, self.policy)

    # ------------------------------------------------------------------ checkpoints
    def meta(self):
        return {"seed": self.seed, "iteration": self.iteration, "policies": policy_names(self.policy)}

    def load_meta(self, meta, say=print):
        """Continue the parameter stream of a checkpoint: its iteration counter; 0 without the entry.  This run's policies and
        seed hold; one printed line says so when the checkpoint's differ."""
        if not meta:
            self.iteration = 0
            return
        self.iteration = int(meta.get("iteration", 0))
        theirs = (policy_mask(meta.get("policies", "")), meta.get("seed", 0))
        if theirs != (self.policy, self.seed):
            say("d_augment: the checkpoint was written with policies '%s' and seed %s; this run's hold: policies '%s', seed %d "
                "(iteration %d continues)" % (policy_names(theirs[0]), theirs[1], policy_names(self.policy), self.seed,
                                              self.iteration))
