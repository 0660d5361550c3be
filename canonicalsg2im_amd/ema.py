"""Exponential moving average (EMA) of a model's weights: a shadow copy, updated in one launch per training step, that
can be swapped in for validation and is saved beside the raw weights (BigGAN, StyleGAN and OASIS all sample from one).

`WeightEMA(model, decay, warmup=True)` walks `model.named_parameters()` and `model.named_buffers()` of the whole
`MetaGeneratorModel`, graph encoder and generator alike:

  * a parameter is an AVERAGE item:   e' = fmaf(d, e, omd * p)   in fp32, d = (float)D, omd = (float)(1.0 - (double)D);
  * a floating-point buffer (BatchNorm running statistics, spectral-norm u / v) is a COPY item:   e' = p, bit for bit;
  * a buffer that is not floating point (`num_batches_tracked`) is not in the table: it is cloned from the live model
    whenever a state dict is produced.

The shadow is ONE flat fp32 allocation, every tensor's slot at a multiple of 4 floats, and the item table lives in device
memory (ops.EmaTable; csrc/ema.hip): an update, a swap and a fill are one launch each.  The SPADE layers join their
gamma / beta parameters into one allocation at their first call; the constructor makes those joins first, so that the
addresses it records are the final ones, and every launch compares the addresses on the host before it goes out
(`EmaTable.refresh`: a moved tensor is checked and the table uploaded again, never followed blindly).

`update()` counts `num_updates` up to n and uses D_n = min(decay, (1 + n) / (10 + n)) with `warmup` (the classic
`num_updates` rule: the first few hundred steps do not average the initialisation in), `decay` without.  It is issued on
the current stream: the caller orders it behind the optimiser steps (train.Trainer.step: both of its paths return with
the generator's Adam step joined to the current stream).

Spectral normalisation.  A spectrally normalised layer's parameter is `weight_orig`; it is averaged as such, and the live
u / v are copied.  The sigma an eval-mode pass over the swapped-in weights divides by is therefore u . (W_ema v) with the
LIVE u, v — standard practice, not a fresh power iteration on W_ema.

Several ranks.  After the all-reduce every rank holds the same parameters, so every rank keeps its own, identical shadow:
no communication; rank 0 saves.  (Exercised on one rank only.)
"""
import contextlib

import torch

from . import ops


def decay_at(decay, n, warmup=True):
    """The decay of update number n (1, 2, ...): min(decay, (1 + n) / (10 + n)) with warm-up, `decay` without."""
    decay, n = float(decay), int(n)
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


def check_decay(decay):
    """0 < D <= 1 (the trainer's `--ema_decay`; 0 means off and never reaches this class)."""
    d = float(decay)
    if not 0.0 < d <= 1.0:
        raise ValueError("--ema_decay must be 0 (off) or lie in (0, 1], got %r" % (decay,))
    return d


def _join_spade_storage(model):
    """Make the joins the SPADE layers would make at their first call (normalization._joined re-points .data of the gamma /
    beta parameters into one allocation): afterwards the parameters' storage stays where it is."""
    from .spade.models.networks.normalization import _joined
    for m in model.modules():
        if hasattr(m, "mlp_gamma") and hasattr(m, "mlp_beta") and hasattr(m, "joined_weight") and m.mlp_gamma.weight.is_cuda:
            m.joined_weight()
            if m.mlp_gamma.bias is not None and m.mlp_beta.bias is not None:
                _joined(m, "_joined_b", m.mlp_gamma.bias, m.mlp_beta.bias)


class WeightEMA:
    def __init__(self, model, decay, warmup=True):
        self.model, self.decay, self.warmup = model, check_decay(decay), bool(warmup)
        self.num_updates = 0
        self._swapped = False
        _join_spade_storage(model)
        # the table holds the Parameter / buffer objects themselves: a re-pointed `.data` shows in EmaTable.refresh()
        self._live, kinds = [], []
        for _, p in model.named_parameters():
            self._live.append(p)
            kinds.append(ops.EMA_AVERAGE)
        for _, b in model.named_buffers():
            if b.is_floating_point():
                self._live.append(b)
                kinds.append(ops.EMA_COPY)
        if not self._live:
            raise ValueError("WeightEMA: the model has no parameters")
        self.table = ops.EmaTable(self._live, kinds)
        self._slot_of = {id(t): i for i, t in enumerate(self._live)}
        ops.ema_fill(self.table)

    # ------------------------------------------------------------------ the step
    def update(self):
        if self._swapped:
            raise RuntimeError("WeightEMA.update() inside swapped(): the live model holds the averaged weights")
        self.num_updates += 1
        ops.ema_update(self.table, decay_at(self.decay, self.num_updates, self.warmup))

    # ------------------------------------------------------------------ state
    def _view(self, i):
        t = self._live[i]
        return self.table.slot(i).as_strided(t.shape, t.stride())

    def state_dict(self):
        """Keys (and order) of `model.state_dict()`; values are copies from the shadow, shaped and laid out like the live
        tensors; what the shadow does not hold (non-floating buffers) is cloned from the live model."""
        out = {}
        for k, v in self.model.state_dict(keep_vars=True).items():
            i = self._slot_of.get(id(v))
            out[k] = (v.detach() if i is None else self._view(i)).clone()
        return out

    def load_state_dict(self, sd, num_updates):
        """Restore the shadow from a state dict with exactly the model's keys, and the counter."""
        live = self.model.state_dict(keep_vars=True)
        if set(sd) != set(live):
            raise KeyError("WeightEMA.load_state_dict: keys differ from the model's (missing %s, unexpected %s)" % (
                sorted(set(live) - set(sd))[:5], sorted(set(sd) - set(live))[:5]))
        with torch.no_grad():
            for k, v in live.items():
                i = self._slot_of.get(id(v))
                if i is not None:
                    if tuple(sd[k].shape) != tuple(v.shape):
                        raise ValueError("WeightEMA.load_state_dict: %s is %s, the model's is %s" % (
                            k, tuple(sd[k].shape), tuple(v.shape)))
                    self._view(i).copy_(sd[k])
        self.num_updates = int(num_updates)

    def fill_from_model(self):
        """Shadow = the live weights, counter 0 (a checkpoint without an EMA; a run that turns it on late)."""
        ops.ema_fill(self.table)
        self.num_updates = 0

    def meta(self):
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates}

    # ------------------------------------------------------------------ swap
    @contextlib.contextmanager
    def swapped(self):
        """The live model holds the averaged weights inside the block (and the shadow the raw ones): one SWAP launch and
        `ops.invalidate_weight_caches()` on entry, the same on exit, also when the block raises.  The swap writes behind the
        tensors' `_version`: whoever keeps something derived from the weights beyond those caches (a `Sampler` that adopted
        the model) drops it on both sides.  Not re-entrant.  Spectral-norm layers: see the module docstring."""
        if self._swapped:
            raise RuntimeError("WeightEMA.swapped() is not re-entrant: the weights are already swapped in")
        ops.ema_swap(self.table)
        ops.invalidate_weight_caches()
        self._swapped = True
        try:
            yield self
        finally:
            ops.ema_swap(self.table)
            ops.invalidate_weight_caches()
            self._swapped = False

