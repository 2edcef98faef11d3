"""Weights derived for inference (BatchNorm folded into scale and shift, weights packed in a kernel's operand order)
and the one rule for how long they live: a derived value is kept next to the signature of the tensors it was built
from and rebuilt when that signature differs.  Every write THROUGH THE TENSOR is seen (`load_state_dict`, `.to()`, an
in-place op, an optimizer step); a write through `.data` is not, and is followed by `invalidate_derived(model)`.
This module is the only place that knows how a derived value is stored."""
from __future__ import annotations

import torch
from torch import nn

__all__ = ["signature", "derived", "slots", "drop", "invalidate_derived", "InferenceCache"]

_SLOTS = "_derived"  # the one name in owner.__dict__: {slot name: (signature, key, value)}


def _tensors(sources, out):
    if isinstance(sources, torch.Tensor):
        out.append(sources)
    elif isinstance(sources, nn.Module):
        out.extend(sources.parameters())
        out.extend(sources.buffers())
    elif sources is not None:
        for s in sources:
            _tensors(s, out)
    return out


def signature(sources):
    """(storage, version, device) of every tensor in `sources`: a module (every parameter, then every buffer below
    it), a tensor, None (skipped) or an iterable of these.  Changes when any of them is reloaded, moved or written in
    place THROUGH THE TENSOR ITSELF (`load_state_dict` on this module or a child, `.to()`,
    `with torch.no_grad(): p.mul_(2)`, an optimizer step).  It does NOT see a write through `p.data`
    (`p.data.copy_(...)`, `p.data.mul_(2)`): `.data` is a detached alias with a version counter of its own, and
    reading the contents instead would cost a device -> host round trip on every forward.  Code that writes through
    `.data` (or through a raw pointer) calls `invalidate_derived(model)` afterwards.
    Attributes only, no device memory is read; the cost is host time in proportion to the tensors walked, between one
    and two microseconds per tensor including the walk over the modules (measured on a CPU host: 0.14 ms for
    SecondBackbone's 96 tensors, 0.55 ms for CenterHead's 331), so a source set names what the value is built from and
    no more."""
    return tuple((t.data_ptr(), t._version, t.device) for t in _tensors(sources, []))


def slots(owner):
    """The slots `owner` holds now, {name: (signature, key, value)}; empty when it holds none."""
    return owner.__dict__.get(_SLOTS, {})


def derived(owner, name, build, sources=None, key=None):
    """The value of slot `name` on `owner`: the one kept when `signature(sources)` (default: of `owner`) and `key`
    (whatever the value depends on that is not a tensor, a device for instance) equal what it was built with, else
    `build()` under no_grad, kept and returned.  The slots are one plain dict in `owner.__dict__`: not a parameter,
    buffer or submodule, absent from `state_dict()`, and just as well on a module this package does not define."""
    sig = signature(owner if sources is None else sources)
    hit = slots(owner).get(name)
    if hit is not None and hit[0] == sig and hit[1] == key:
        return hit[2]
    with torch.no_grad():
        value = build()
    owner.__dict__.setdefault(_SLOTS, {})[name] = (sig, key, value)
    return value


def drop(owner):
    """Empty the slots of `owner` itself."""
    slots(owner).clear()


def invalidate_derived(module):
    """Drop every derived weight below `module`; the next forward rebuilds them from the current parameters.  Needed
    only after a write the signature cannot see (`param.data.*`, see signature)."""
    for m in module.modules():
        drop(m)
    return module


class InferenceCache:
    """Mixin of the inference-only layers that hold derived weights: `train()` drops them outright, `invalidate()`
    is invalidate_derived on the module, `_require_eval()` refuses a forward in training mode."""

    def train(self, mode: bool = True):
        drop(self)
        return super().train(mode)

    def invalidate(self):
        return invalidate_derived(self)

    def _require_eval(self):
        if self.training:
            raise RuntimeError(f"{type(self).__name__}: paddle3d_amd implements the inference path only "
                               "(BatchNorm folded into the HIP kernels); call .eval() first")
