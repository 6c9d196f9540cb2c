"""Channel pruning by BatchNorm scale: the selection and the weight copy of the reference's ``micronet/compression/pruning`` (network slimming).

The chain is *sparse training -> prune -> refine -> QAT on the pruned widths*:

* sparse training is an ordinary training loop whose optimizer adds ``s * sign(gamma)`` to every BatchNorm scale's gradient --
  ``train.make_optimizer(model, sparse_s=s)`` does it inside the one-launch Adam step (the reference: ``updateBN()``, pruning/main.py:65-69);
* ``regular_prune`` (normal_regular_prune.py:61-130) / ``gc_prune_cfg`` (gc_prune.py:38-132) pick the channels: one global threshold over ``|gamma|``,
  per-layer counts rounded to a base number, and return ``(cfg, masks)`` -- ``cfg`` is what ``models.nin.Net(cfg=)`` / ``models.nin_gc.Net(cfg=)`` and
  ``data.save_state(..., cfg=)`` take;
* ``compact`` (normal_regular_prune.py:186-231) copies the kept channels of a dense net into the narrow one.

All of it is host-side torch on a few thousand scales and a one-off weight copy: there is no hot path here and no kernel."""
import math

import torch
import torch.nn as nn

from ._lib import MicronetHipError

__all__ = ["bn_threshold", "regular_prune", "gc_prune_cfg", "compact"]


def _pruned_bns(model, layers):
    """(name, module) of the first ``layers - 1`` BatchNorm2d of ``model`` (the last block feeds the classifier and keeps its width)."""
    bns = [(n, m) for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)][:max(layers - 1, 0)]
    if not bns:
        raise MicronetHipError("pruning: no BatchNorm2d among the first %d layers of the model" % (layers - 1))
    return bns


def bn_threshold(model, percent, layers):
    """The global pruning threshold (0-dim tensor): element ``int(total * percent)`` -- clamped to ``total - 1`` -- of the ascending sort of ``|gamma|`` over the
    first ``layers - 1`` BatchNorm2d modules (normal_regular_prune.py:61-84)."""
    if not 0.0 <= percent <= 1.0:
        raise ValueError("pruning: percent must be in [0, 1], got %r" % (percent,))
    y = torch.sort(torch.cat([m.weight.detach().abs().reshape(-1) for _, m in _pruned_bns(model, layers)]))[0]
    return y[min(int(y.numel() * percent), y.numel() - 1)]


@torch.no_grad()
def _select(model, percent, layers, bases, fill_small=False):
    thre = bn_threshold(model, percent, layers)
    cfg, masks = [], []
    for (name, m), base in zip(_pruned_bns(model, layers), bases):
        a = m.weight.detach().abs()
        mask = a > thre
        remain = int(mask.sum())
        if remain == 0:                               # the whole layer is under the threshold: it keeps one channel (arg-max of gamma, as the reference)
            remain = 1
            mask[int(torch.argmax(m.weight.detach()))] = True
        if remain % base != 0 and (remain > base or fill_small):      # regular pruning: the nearer multiple of the base number, a tie goes up
            lower = remain // base * base
            remain = lower if 0 < lower and remain - lower < lower + base - remain else lower + base
            remain = min(remain, a.numel())
            cut = torch.sort(a)[0][-remain]
            mask = a >= cut
            if int(mask.sum()) != remain:
                # the reference goes on with this mask and fails later, in the weight copy, on a shape mismatch against Net(cfg)
                raise MicronetHipError("pruning: layer %s keeps %d channels, but %d have |gamma| >= the cut %r (tied scales at the cut); "
                                       "break the tie or choose another percent / base number" % (name, remain, int(mask.sum()), float(cut)))
        cfg.append(remain)
        masks.append(mask)
    for (_, m), mask in zip(_pruned_bns(model, layers), masks):          # (only now: a tie above leaves the model as it was)
        m.weight.mul_(mask.to(m.weight.dtype))        # the "pre-pruned" model: pruned channels are exactly 0 behind the ReLU
        m.bias.mul_(mask.to(m.bias.dtype))
    return cfg, masks


def regular_prune(model, percent, base_number=1, layers=9):
    """Select the channels of the first ``layers - 1`` BatchNorm2d whose ``|gamma|`` exceeds the global threshold (``bn_threshold``) and round each layer's count
    to a multiple of ``base_number`` (normal_regular_prune.py:86-130): a layer left empty keeps its arg-max channel; a count above ``base_number`` that is no
    multiple of it goes to the nearer multiple (a tie up), capped at the layer width, and the layer then keeps its ``count`` largest ``|gamma|``.  Tied scales at
    that cut would keep more channels than ``cfg`` says: that raises ``MicronetHipError``.  Like the reference, gamma and beta of ``model`` are multiplied by the
    mask IN PLACE.  Returns ``(cfg, masks)``: the widths and one bool mask per pruned layer."""
    if int(base_number) != base_number or base_number < 1:
        raise ValueError("pruning: base_number must be a positive integer, got %r" % (base_number,))
    return _select(model, percent, layers, [int(base_number)] * max(layers - 1, 0))


def gc_prune_cfg(model, percent, layers=9):
    """``regular_prune`` for a net of grouped convolutions (gc_prune.py:62-132): the base number of layer j is the smallest count divisible by the group counts of
    both convolutions it touches, read from the model's own conv shapes (``groups[j + 1] = out[j] / in_per_group[j + 1]``), so that ``models.nin_gc.Net(cfg)``
    can be built.  Like the reference it yields a ``cfg`` to retrain from (grouped convs behind a channel shuffle are not copied); the masks are returned for
    inspection.

    One deliberate difference: the reference leaves a count BELOW the base number as it is (gc_prune.py:111-112 only rounds counts above it), and ``Net(cfg)``
    then cannot be built (14 channels into a 16-group convolution).  Here such a layer keeps ``base`` channels, the smallest width the grouped net accepts."""
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    groups = [1] + [convs[j].weight.shape[0] // convs[j + 1].weight.shape[1] for j in range(len(convs) - 1)]
    bases = [math.lcm(groups[j], groups[j + 1]) for j in range(len(groups) - 1)]
    if len(bases) < layers - 1:
        raise MicronetHipError("pruning: %d convolutions give %d base numbers, %d layers need %d" % (len(convs), len(bases), layers, layers - 1))
    return _select(model, percent, layers, bases, fill_small=True)


def _copy(dst, src, what):
    if dst.shape != src.shape:
        raise MicronetHipError("pruning.compact: %s is %s in the new model, the masks select %s" % (what, tuple(dst.shape), tuple(src.shape)))
    dst.copy_(src)


@torch.no_grad()
def compact(model, masks, new_model):
    """Copy the channels ``masks`` keep from the dense ``model`` into ``new_model`` (= the same architecture built with the pruned ``cfg``), as
    normal_regular_prune.py:186-231: BatchNorm scale / shift / running statistics by the layer's own mask, conv weights by (previous mask -> input channels, own
    mask -> output channels), conv bias by the own mask; layers behind the pruned range only lose input channels.  ``index_select`` on the tensors' own device.
    Grouped convolutions raise (their input channels are not a plain slice; retrain from the cfg as gc_prune does).  Returns ``new_model``."""
    mods0, mods1 = list(model.named_modules()), list(new_model.modules())
    if len(mods0) != len(mods1) or any(type(a[1]) is not type(b) for a, b in zip(mods0, mods1)):
        raise MicronetHipError("pruning.compact: the two models do not have the same module structure")
    pairs = list(zip(mods0, mods1))
    idx = lambda mask, ref: torch.nonzero(mask.to(ref.device), as_tuple=False).reshape(-1)
    start, k = None, 0                                # start: kept channels of the layer in front (None: all, the image); k: BatchNorms done
    for (name, m0), m1 in pairs:
        if isinstance(m0, nn.Conv2d):
            if m0.groups != 1:
                raise MicronetHipError("pruning.compact: %s is a grouped convolution (groups = %d); retrain from the cfg instead" % (name, m0.groups))
            w = m0.weight if start is None else m0.weight.index_select(1, idx(start, m0.weight))
            b = m0.bias
            if k < len(masks):
                own = idx(masks[k], w)
                w = w.index_select(0, own)
                b = None if b is None else b.index_select(0, own)
            _copy(m1.weight, w, name + ".weight")
            if b is not None:
                _copy(m1.bias, b, name + ".bias")
        elif isinstance(m0, nn.BatchNorm2d):
            ts = [("weight", m0.weight, m1.weight), ("bias", m0.bias, m1.bias), ("running_mean", m0.running_mean, m1.running_mean),
                  ("running_var", m0.running_var, m1.running_var)]
            own = idx(masks[k], m0.weight) if k < len(masks) else None
            for tname, t0, t1 in ts:
                if t0 is not None:
                    _copy(t1, t0 if own is None else t0.index_select(0, own), "%s.%s" % (name, tname))
            if m0.num_batches_tracked is not None:
                m1.num_batches_tracked.copy_(m0.num_batches_tracked)
            if k < len(masks):
                start = masks[k]
            k += 1
        elif isinstance(m0, nn.Linear):
            raise MicronetHipError("pruning.compact: %s: only convolutional nets (models.nin.Net) are copied" % name)
    return new_model
