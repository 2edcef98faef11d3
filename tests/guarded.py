"""Guarded device allocations and a launch ledger for the memory-safety tests (a helper module, not a conftest).

`guarded(fill, device)` replaces, while it is active, the Python-level allocation functions the library uses
(`torch.empty/zeros/ones/full`, their `*_like` forms and `Tensor.new_empty/new_zeros/new_ones/new_full`) for
allocations on `device` only.  Every such tensor is carved out of a `uint8` buffer of its own:

    [ G bytes PATTERN | nbytes of the tensor, pre-filled with `fill` | G bytes PATTERN ]

* the tensor starts at offset G, a multiple of 512, so its pointer has the alignment torch's caching allocator gives
  (512 bytes) and the library picks the same kernels and vector paths as in production;
* it ends exactly at G + nbytes: the tail band starts on the first byte past the tensor, with no rounding, so an
  overrun of a single element is seen;
* the interior holds the byte `fill` when it is handed out (`zeros`/`ones`/`full` then write their value as usual),
  so an op that reads memory it never wrote computes different bits under fill 0x00 and 0xFF;
* `Guard.check()` lists the allocations whose bands no longer hold PATTERN.

G is 1 MiB.  It has to be at least the largest single row / tile any scenario's kernels store, so that "one row too
many" or "one tile too far" stays inside a band: the widest rows of the scenarios are a 496*432 fp32 canvas plane row
(1.7 KiB), a 128-channel fp16 NHWC map row of 45 columns (11 KiB) and a 64x64 fp32 output tile (16 KiB); whole small
maps (16 x 6 x 48 fp32 = 18 KiB) fit as well, and so does the widest row of the model scenarios (one NHWC row of the
AMP CenterHead's first stage: 128 pixels x 2304 channels x 2 bytes = 576 KiB).  A store further than G from the tensor
is out of this harness's reach: it lands in another block or in unmapped memory, and only a device fault would show it.

What is NOT intercepted: tensors that come out of torch operators (`cat`, `stack`, `arange`, `tensor`, `from_numpy().to`,
`clone`, `contiguous`, `randn`, arithmetic).  Those are written completely by the operator that makes them, so they
carry no stale bytes; an overrun past one of them is not seen.  The library hands such tensors to kernels as inputs
only (every output and workspace is one of the patched calls), and inputs are `const` in the ABI.

`launch_ledger(handle, symbols)` counts the calls of the named C-ABI symbols made through a `paddle3d_amd._lib.lib()`
handle.

`Protocol` is the three-pass run every memory-safety file holds its scenarios to (plain, fill 0x00, fill 0xFF) and the
completeness assertion over the entry points whose table rows name that file; tests/test_guarded_cpu.py shows, on fake
ops, that each of its assertions fails when it should.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass

import numpy as np
import torch

G = 1 << 20          # bytes of guard band on each side; a multiple of 512 (see the module docstring)
PATTERN = 0xA5       # band byte: neither 0x00 nor 0xFF, so that neither fill nor a memset to zero restores it
assert G % 512 == 0

_TORCH_FUNCS = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")
_TENSOR_METHODS = ("new_empty", "new_zeros", "new_ones", "new_full")
# a call that asks for one of these is not a plain dense device allocation: it is passed through untouched
_PASS_THROUGH_KW = ("out", "layout", "pin_memory", "names")


@dataclass
class Damage:
    index: int        # position in Guard.blocks (order of allocation)
    shape: tuple
    dtype: torch.dtype
    side: str         # "head" (before the tensor) or "tail" (after it)
    offset: int       # head: bytes before the first byte of the tensor (-1 is the byte just before);
                      # tail: bytes past the end (0 is the first byte after the tensor)

    def __str__(self):
        return f"allocation #{self.index} {tuple(self.shape)} {self.dtype}: {self.side} guard damaged at byte {self.offset:+d}"


def _shape_of(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


class Guard:
    def __init__(self, fill: int, device="cuda"):
        assert 0 <= int(fill) <= 0xFF
        self.fill = int(fill)
        self.device = torch.device(device)
        self.blocks = []  # (buffer, nbytes, shape, dtype)

    def owns(self, device) -> bool:
        """True when an allocation on `device` (None = torch's default device) is to be guarded."""
        d = torch.device(device) if device is not None else _ORIG["empty"](()).device
        if d.type != self.device.type:
            return False
        return d.index is None or self.device.index is None or d.index == self.device.index

    def alloc(self, shape, dtype, device=None, stride=None) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        dtype = dtype or torch.get_default_dtype()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * _ORIG["empty"]((), dtype=dtype, device="meta").element_size()
        dev = torch.device(device) if device is not None else self.device
        buf = _ORIG["empty"](nbytes + 2 * G, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 512 == 0 or dev.type == "cpu", "caching allocator blocks are 512-byte aligned"
        buf[:G] = PATTERN
        buf[G + nbytes:] = PATTERN
        buf[G:G + nbytes] = self.fill
        self.blocks.append((buf, nbytes, shape, dtype))
        flat = buf[G:G + nbytes].view(dtype)
        if stride is not None:
            return flat.as_strided(shape, stride)
        return flat.view(shape)

    def check(self):
        """Allocations whose guard bands changed, as a list of Damage (empty = all bands intact).  One reduction per
        band on the device, one host read for all of them."""
        if not self.blocks:
            return []
        far = G + 1  # "no damaged byte" sentinel: larger than any distance inside a band
        firsts = []
        pos = torch.arange(G, device=self.blocks[0][0].device)
        for buf, nbytes, _, _ in self.blocks:
            head, tail = buf[:G], buf[G + nbytes:]
            # head: the damaged byte nearest to the tensor; tail: likewise, i.e. the lowest offset
            firsts.append(torch.where(head != PATTERN, G - pos, far).min())
            firsts.append(torch.where(tail != PATTERN, pos, far).min())
        host = torch.stack(firsts).cpu().tolist()
        bad = []
        for i, (_, _, shape, dtype) in enumerate(self.blocks):
            if host[2 * i] != far:
                bad.append(Damage(i, shape, dtype, "head", -host[2 * i]))
            if host[2 * i + 1] != far:
                bad.append(Damage(i, shape, dtype, "tail", host[2 * i + 1]))
        return bad


_ORIG = {name: getattr(torch, name) for name in _TORCH_FUNCS}
_ORIG_METHODS = {name: getattr(torch.Tensor, name) for name in _TENSOR_METHODS}


def _plain(kw) -> bool:
    return all(k not in kw or kw[k] is None or kw[k] is False or kw[k] is torch.strided for k in _PASS_THROUGH_KW)


def _finish(t, value, requires_grad):
    if value is not None:
        t.fill_(value)
    if requires_grad:
        t.requires_grad_(True)
    return t


def _make_creator(g: Guard, name: str, value, takes_value: bool):
    """torch.empty / zeros / ones (value fixed) and torch.full (value is the second argument)."""
    orig = _ORIG[name]

    def creator(*args, dtype=None, device=None, requires_grad=False, **kw):
        plain = _plain(kw)
        if not (plain and g.owns(device)):
            return orig(*args, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        if takes_value:
            size = kw.pop("size") if "size" in kw else args[0]
            v = kw.pop("fill_value") if "fill_value" in kw else args[-1]
            if dtype is None:  # torch.full infers the dtype from the value
                dtype = orig((), v).dtype
            return _finish(g.alloc(_shape_of((size,)), dtype, device), v, requires_grad)
        size = (kw.pop("size"),) if "size" in kw else args
        return _finish(g.alloc(_shape_of(size), dtype, device), value, requires_grad)

    creator.__name__ = name
    return creator


def _make_like(g: Guard, name: str, value, takes_value: bool):
    orig = _ORIG[name]

    def like(t, *args, dtype=None, device=None, requires_grad=False, **kw):
        plain = _plain(kw)
        dev = device if device is not None else t.device
        if not (plain and g.owns(dev) and t.layout == torch.strided):
            return orig(t, *args, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        v = (kw.pop("fill_value") if "fill_value" in kw else args[0]) if takes_value else value
        # the strides torch itself would give (preserve_format keeps a dense permuted layout such as channels_last)
        ref = _ORIG["empty_like"](t, dtype=dtype, device="meta", memory_format=kw.get("memory_format", torch.preserve_format))
        return _finish(g.alloc(ref.shape, ref.dtype, dev, stride=ref.stride()), v, requires_grad)

    like.__name__ = name
    return like


def _make_method(g: Guard, name: str, value, takes_value: bool):
    orig = _ORIG_METHODS[name]

    def method(self, *args, dtype=None, device=None, requires_grad=False, **kw):
        plain = _plain(kw)
        dev = device if device is not None else self.device
        if not (plain and g.owns(dev)):
            return orig(self, *args, dtype=dtype, device=device, requires_grad=requires_grad, **kw)
        if takes_value:
            size = kw.pop("size") if "size" in kw else args[0]
            v = kw.pop("fill_value") if "fill_value" in kw else args[-1]
            return _finish(g.alloc(_shape_of((size,)), dtype or self.dtype, dev), v, requires_grad)
        size = (kw.pop("size"),) if "size" in kw else args
        return _finish(g.alloc(_shape_of(size), dtype or self.dtype, dev), value, requires_grad)

    method.__name__ = name
    return method


_VALUES = {"empty": None, "zeros": 0, "ones": 1, "full": None}


@contextlib.contextmanager
def guarded(fill: int, device="cuda"):
    """Guard every patched allocation on `device` made inside the block; yields the Guard (see the module docstring).
    The patched names are restored on exit, also when the block raises."""
    g = Guard(fill, device)
    try:
        for kind in ("empty", "zeros", "ones", "full"):
            full = kind == "full"
            setattr(torch, kind, _make_creator(g, kind, _VALUES[kind], full))
            setattr(torch, kind + "_like", _make_like(g, kind + "_like", _VALUES[kind], full))
            setattr(torch.Tensor, "new_" + kind, _make_method(g, "new_" + kind, _VALUES[kind], full))
        yield g
    finally:
        for name, fn in _ORIG.items():
            setattr(torch, name, fn)
        for name, fn in _ORIG_METHODS.items():
            setattr(torch.Tensor, name, fn)


@contextlib.contextmanager
def launch_ledger(handle, symbols):
    """Count the calls of the C-ABI `symbols` made through `handle` (`paddle3d_amd._lib.lib()`): yields {symbol: calls}.
    There is no default name set: a caller that asserts "nothing else ran" says which names it watches
    (`_lib.symbols()` is all of them, `_lib.symbols(module)` one block of the table).

    A counting Python wrapper is put on the handle as an instance attribute under each name; it calls the original
    function object (with its argtypes / restype) through.  The originals are put back on exit, also on an exception."""
    calls = {name: 0 for name in symbols}
    originals = {name: getattr(handle, name) for name in symbols}

    def counting(name, fn):
        def wrapper(*args):
            calls[name] += 1
            return fn(*args)

        wrapper.__name__ = name
        wrapper.__wrapped__ = fn
        return wrapper

    try:
        for name, fn in originals.items():
            setattr(handle, name, counting(name, fn))
        yield calls
    finally:
        for name, fn in originals.items():
            setattr(handle, name, fn)


def _host(v):
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    return v.detach().contiguous().cpu()


def _bits(t):
    return t.reshape(-1).view(torch.uint8)


def _nontrivial(t):
    """The number of elements that are neither 0 nor -1 (this code base's "no neighbour") nor NaN."""
    x = t.reshape(-1)
    x = x[~torch.isnan(x)].double() if x.dtype.is_floating_point else x.long()
    return int(((x != 0) & (x != -1)).sum())


class Protocol:
    """One memory-safety file's scenarios, its ledger and the assertions they are held to.

    `module` is the file's bare name: the ledger counts `_lib.symbols(module)`, the names whose table rows say their
    scenarios live here.  A scenario is a function that builds seeded inputs and returns `(inputs, call)`; `call()`
    returns the dict of specified outputs (tensors or ndarrays), in which `__trivial_ok__` may name the outputs that
    are legally all 0 / -1.  `tolerant` maps (scenario, output suffix) to {dtype: relative bound of max(|plain|, 1)}
    for the outputs that are documented as order dependent; everything else compares bit for bit.  `before_pass()`
    runs ahead of every pass, outside the guard and the ledger; `may_allocate_nothing` names the scenarios whose
    guarded passes need not allocate.  `handle` / `symbols` replace the library and its table (the CPU self-test)."""

    def __init__(self, module, tag, device, tolerant=None, before_pass=None, may_allocate_nothing=(), handle=None,
                 symbols=None):
        self.module, self.tag, self.device = module, tag, torch.device(device)
        self.tolerant, self.before_pass, self.may_allocate_nothing = tolerant or {}, before_pass, set(may_allocate_nothing)
        self.handle, self.symbols = handle, symbols
        self.scenarios = {}
        self.ledger = {}   # symbol -> calls, summed over the guarded 0xFF pass of every scenario that ran
        self.ran = set()

    def scenario(self, fn):
        self.scenarios[fn.__name__] = fn
        return fn

    def _count(self, calls):
        for sym, n in calls.items():
            self.ledger[sym] = self.ledger.get(sym, 0) + n

    def run(self, name, mode):
        """One pass of a scenario: (specified outputs on the host, guard damage, names of changed inputs, calls per
        symbol, names of the outputs that may be trivial)."""
        if self.handle is None:
            from paddle3d_amd import _lib

            self.handle, self.symbols = _lib.lib(), _lib.symbols(self.module)
        if self.before_pass is not None:
            self.before_pass()
        print(f"[{self.tag}] {name}: {mode}", flush=True)
        ctx = contextlib.nullcontext(None) if mode == "plain" else guarded(int(mode, 16), self.device)
        with ctx as g, launch_ledger(self.handle, self.symbols) as calls:
            inputs, call = self.scenarios[name]()
            before = {k: v.clone() for k, v in inputs.items()}
            outs = call()
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            damage = g.check() if g is not None else []
            trivial_ok = outs.pop("__trivial_ok__", set())
            host = {k: _host(v) for k, v in outs.items()}
            changed = [k for k, v in inputs.items() if not torch.equal(_bits(_host(v)), _bits(_host(before[k])))]
            if g is not None and self.device.type == "cuda":  # every guarded tensor has the caching allocator's alignment
                assert all(buf.data_ptr() % 512 == 0 for buf, _, _, _ in g.blocks)
            assert g is None or len(g.blocks) > 0 or name in self.may_allocate_nothing, f"{name} [{mode}]: nothing allocated"
        return host, damage, changed, {k: v for k, v in calls.items() if v}, trivial_ok

    def check_scenario(self, name):
        ref, damage, changed, calls, trivial_ok = self.run(name, "plain")
        assert damage == [] and changed == [], f"{name} [plain]: inputs written: {changed}"
        assert ref, f"{name}: no outputs"
        for k, v in ref.items():  # 4. the specified outputs are not trivial
            if k not in trivial_ok:
                assert v.numel() > 0 and _nontrivial(v) > 0, f"{name}: output {k} {tuple(v.shape)} is empty or all 0 / -1"
        for mode in ("0x00", "0xFF"):
            got, damage, changed, calls_g, _ = self.run(name, mode)
            # 1. no store outside an output or a workspace
            assert damage == [], f"{name} [{mode}]: " + "; ".join(str(d) for d in damage)
            # 3. inputs are const
            assert changed == [], f"{name} [{mode}]: inputs written: {changed}"
            # 2. no result depends on what its buffer held before
            assert set(got) == set(ref), (name, mode, set(got) ^ set(ref))
            for k, want in ref.items():
                have = got[k]
                assert have.shape == want.shape and have.dtype == want.dtype, (name, mode, k, have.shape, want.shape)
                tols = next((t for (scn, key), t in self.tolerant.items() if scn == name and k.endswith(key)), None)
                if tols is not None:
                    tol = tols[want.dtype]  # (a dtype without a bound of its own is an error, not a default)
                    err = float((have.double() - want.double()).abs().max())
                    bound = tol * max(float(want.double().abs().max()), 1.0)
                    assert bool(torch.isfinite(have).all()) and err <= bound, f"{name} [{mode}]: {k}: {err} > {bound}"
                    continue
                diff = (_bits(have) != _bits(want)).nonzero().reshape(-1)
                if diff.numel():
                    first = int(diff[0]) // have.element_size()
                    raise AssertionError(
                        f"{name} [{mode}]: output {k} {tuple(have.shape)} {have.dtype} depends on the previous contents "
                        f"of memory: {diff.numel()} bytes differ from the plain run, first at element {first} "
                        f"(plain {want.reshape(-1)[first].item()!r}, guarded {have.reshape(-1)[first].item()!r})")
            assert set(calls_g) == set(calls), (f"{name} [{mode}]: other entry points ran than in the plain run: "
                                                f"{sorted(set(calls_g) ^ set(calls))}")
        self._count(calls_g)
        self.ran.add(name)

    def check_complete(self, required, count=None):
        """Every name of `required` (`count` of them, where the file states a literal count) is reached by a scenario.
        Scenarios that did not run in this process (the test selected alone, or with -k) are run here in their plain
        form under the ledger, so the assertion never depends on test selection."""
        for name in self.scenarios:
            if name not in self.ran:
                self._count(self.run(name, "plain")[3])
                self.ran.add(name)
        required = list(required)
        assert count is None or len(required) == count, (self.module, len(required), count)
        missing = [s for s in required if not self.ledger.get(s)]
        assert not missing, (f"{len(missing)} of the {len(required)} required entry points of {self.module} are reached "
                             f"by no scenario: {missing}.  This is intended to fail for a symbol newly added to the "
                             f"table: add a scenario to tests/{self.module}.py that calls it.")
