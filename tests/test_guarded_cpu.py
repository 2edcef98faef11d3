"""The guarded-allocation harness (tests/guarded.py) proves it can fail: small fake "ops" on the CPU, one per defect
class the GPU memory-safety scenarios are meant to catch, plus the plumbing (argument forms, other devices, restore);
then the Protocol every memory-safety file runs its scenarios through, on a fake handle with two Python functions as
entry points: each of its assertions fails, with its own message, on the defect it is there for.
No GPU is needed; test_launch_ledger_on_the_real_handle loads the built libpaddle3d_amd.so (`python -m
paddle3d_amd.build`), the same precondition as tests/test_abi.py."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import G, PATTERN, Protocol, guarded, launch_ledger  # noqa: E402


def _bits(t):
    return t.detach().contiguous().view(torch.uint8).flatten().clone()


def _both_fills(op, *args):
    """Run `op` under fill 0x00 and 0xFF: [(output bits, damage list)] * 2."""
    res = []
    for fill in (0x00, 0xFF):
        with guarded(fill, "cpu") as g:
            out = op(*args)
            res.append((_bits(out), g.check()))
    return res


def _poke(t, byte_offset):
    """Store one byte at `byte_offset` relative to the first byte of t (negative: before it; nbytes + k: past it)."""
    n = t.numel() * t.element_size()
    lo = min(byte_offset, 0)
    raw = torch.as_strided(t.view(torch.uint8).flatten(), (n - lo + G,), (1,), t.storage_offset() * t.element_size() + lo)
    raw[byte_offset - lo] = 0x3C


def op_ok(x):
    out = torch.empty(x.shape[0], 3, dtype=torch.float32, device=x.device)
    out.copy_(x[:, :3])
    return out


def op_stale_row(x):
    out = torch.empty_like(x)
    out[:-1] = x[:-1]  # the last row is never written
    return out


def op_accumulate(x):
    acc = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    acc += x.sum(0)  # accumulates into memory nobody cleared
    return acc


def test_constants():
    assert G % 512 == 0 and G >= 1 << 20
    assert PATTERN not in (0x00, 0xFF)


def test_correct_op_is_clean_and_fill_independent():
    x = torch.randn(7, 5)
    (b0, d0), (b1, d1) = _both_fills(op_ok, x)
    assert d0 == [] and d1 == []
    assert torch.equal(b0, b1) and torch.equal(b0, _bits(x[:, :3]))


@pytest.mark.parametrize("where,side,offset", [("before", "head", -1), ("end", "tail", 0),
                                               ("far_end", "tail", G - 1), ("far_before", "head", -G)])
def test_one_stray_byte_is_reported(where, side, offset):
    with guarded(0x00, "cpu") as g:
        other = torch.empty(4, dtype=torch.int32)           # allocation 0: untouched
        out = torch.empty((5, 3), dtype=torch.float16)      # allocation 1: 30 bytes, not a multiple of anything useful
        other.zero_()
        out.zero_()
        nbytes = out.numel() * out.element_size()
        _poke(out, {"before": -1, "end": nbytes, "far_end": nbytes + G - 1, "far_before": -G}[where])
        bad = g.check()
    assert len(bad) == 1, [str(b) for b in bad]
    d = bad[0]
    assert (d.index, d.shape, d.dtype, d.side, d.offset) == (1, (5, 3), torch.float16, side, offset), str(d)
    assert "(5, 3)" in str(d) and side in str(d)


def test_damage_on_both_sides_and_nearest_offset_reported():
    with guarded(0xFF, "cpu") as g:
        out = torch.empty(10, dtype=torch.float32)
        _poke(out, 40 + 100)
        _poke(out, 40 + 7)
        _poke(out, -3)
        _poke(out, -200)
        bad = g.check()
    assert [(d.side, d.offset) for d in bad] == [("head", -3), ("tail", 7)]


def test_unwritten_row_differs_between_fills():
    x = torch.randn(6, 4)
    (b0, d0), (b1, d1) = _both_fills(op_stale_row, x)
    assert d0 == [] and d1 == []
    assert not torch.equal(b0, b1)
    assert torch.equal(b0[:-16], b1[:-16])  # only the last row (4 floats) differs


def test_accumulation_into_empty_differs_between_fills():
    x = torch.rand(6, 4) + 1.0
    (b0, _), (b1, _) = _both_fills(op_accumulate, x)
    assert not torch.equal(b0, b1)
    assert torch.equal(b0, _bits(x.sum(0)))  # right on clean memory, which is why an unguarded test never notices


def test_interior_is_filled_and_zeros_family_overwrites_it():
    with guarded(0xFF, "cpu"):
        e = torch.empty(3, 2, dtype=torch.int32)
        assert bool((e == -1).all())
        assert bool(torch.isnan(torch.empty(5)).all())
        assert bool((torch.zeros(3, 2) == 0).all()) and bool((torch.ones((2,), dtype=torch.int64) == 1).all())
        f = torch.full((4, 2), -1, dtype=torch.int32)
        assert f.dtype == torch.int32 and bool((f == -1).all())
        assert torch.full((2,), 0.5).dtype == torch.float32 and torch.full((2,), 3).dtype == torch.int64
        assert bool((torch.zeros_like(e) == 0).all()) and bool((torch.full_like(e, 7) == 7).all())
        assert bool((torch.ones_like(e, dtype=torch.float16) == 1).all())
        assert bool((e.new_zeros(2, 3) == 0).all()) and e.new_zeros((2, 3)).shape == (2, 3)
        assert e.new_empty((4,)).dtype == torch.int32 and e.new_empty(4, dtype=torch.float64).dtype == torch.float64
        assert bool((e.new_full((2,), 9) == 9).all()) and bool((e.new_ones(2) == 1).all())
    with guarded(0x00, "cpu"):
        assert bool((torch.empty(3, 2, dtype=torch.float32) == 0).all())


def test_argument_forms_of_the_library_call_sites():
    with guarded(0x00, "cpu") as g:
        a = torch.empty((2, 3), dtype=torch.float16, device="cpu")           # size as a tuple
        b = torch.empty(2, 3, dtype=torch.float16, device=torch.device("cpu"))  # as separate ints
        c = torch.empty([2, 3], device="cpu", dtype=torch.float16)           # a list, keywords swapped
        d = torch.empty(torch.Size([2, 3]))                                  # default dtype and device
        e = torch.empty(0, 4, dtype=torch.int32)                             # no bytes at all
        s = torch.empty((), dtype=torch.int32)                               # a scalar counter
        p = torch.empty(3, 4, 5, requires_grad=True)
        w = torch.nn.Parameter(torch.empty(3, 3, 4, 8))                      # as sparse.py builds its weights
        z = torch.zeros(size=(2, 2))
        n_alloc = len(g.blocks)
        for t in (a, b, c):
            assert t.shape == (2, 3) and t.dtype == torch.float16 and t.is_contiguous()
        assert d.dtype == torch.float32 and e.shape == (0, 4) and s.shape == () and z.shape == (2, 2)
        assert p.requires_grad and p.is_leaf and w.shape == (3, 3, 4, 8)
        # ordinary tensor behaviour of a carved view
        a.copy_(torch.arange(6).view(2, 3))
        assert a.view(-1).tolist() == [0, 1, 2, 3, 4, 5] and a.t().contiguous().shape == (3, 2)
        assert a[1:].data_ptr() == a.data_ptr() + 6
        like = torch.empty_like(a, dtype=torch.int64)
        assert like.shape == (2, 3) and like.dtype == torch.int64
        assert g.check() == []
    assert n_alloc == 9


def test_like_keeps_a_dense_permuted_layout():
    x = torch.randn(2, 4, 3, 5).contiguous(memory_format=torch.channels_last)
    with guarded(0x00, "cpu") as g:
        y = torch.empty_like(x)
        z = torch.empty_like(x, memory_format=torch.contiguous_format)
        assert y.stride() == x.stride() and z.is_contiguous()
        y.copy_(x)
        assert torch.equal(y, x) and g.check() == []


def test_other_devices_and_special_requests_pass_through():
    with guarded(0x00, "cuda") as g:  # guards cuda only: nothing on the CPU is touched (and no GPU is needed)
        a = torch.empty(3, 4)
        b = torch.zeros((2,), dtype=torch.int32, device="cpu")
        c = torch.empty_like(a)
        d = a.new_zeros(5)
        m = torch.empty(2, 2, device="meta")
        assert g.blocks == [] and a.shape == (3, 4) and b.tolist() == [0, 0] and c.shape == (3, 4) and d.shape == (5,)
        assert m.device.type == "meta"
    with guarded(0x00, "cpu") as g:
        m = torch.empty(2, 2, device="meta")
        o = torch.zeros(4)
        torch.empty(4, out=o)
        assert m.device.type == "meta" and len(g.blocks) == 1  # only `o`


def test_device_index_matching():
    from guarded import Guard

    g = Guard(0, "cuda:1")
    assert g.owns("cuda:1") and g.owns("cuda") and not g.owns("cuda:0") and not g.owns("cpu") and not g.owns(None)
    g = Guard(0, "cuda")
    assert g.owns("cuda:0") and g.owns(torch.device("cuda", 3)) and not g.owns(None)
    assert Guard(0, "cpu").owns(None)


def test_workspace_is_guarded_and_exact():
    from paddle3d_amd.ops._common import workspace

    with guarded(0xFF, "cpu") as g:
        small, odd = workspace(10, "cpu"), workspace(1000, torch.device("cpu"))
        assert small.numel() == 256 and odd.numel() == 1000 and odd.dtype == torch.uint8
        assert len(g.blocks) == 2 and g.blocks[1][1] == 1000 and g.blocks[1][0].numel() == 1000 + 2 * G
        assert bool((odd == 0xFF).all())
        _poke(odd, 1000)  # a kernel using one byte more than pd3_*_workspace() reported
        bad = g.check()
    assert [(d.index, d.side, d.offset) for d in bad] == [(1, "tail", 0)]


def test_names_are_restored_after_exit_and_after_an_exception():
    names = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")
    methods = ("new_empty", "new_zeros", "new_ones", "new_full")
    before = [getattr(torch, n) for n in names] + [getattr(torch.Tensor, n) for n in methods]
    with guarded(0x00, "cpu"):
        assert torch.empty is not before[0] and torch.Tensor.new_zeros is not before[9]
    assert [getattr(torch, n) for n in names] + [getattr(torch.Tensor, n) for n in methods] == before
    with pytest.raises(ZeroDivisionError):
        with guarded(0xFF, "cpu"):
            torch.empty(3)
            1 / 0
    after = [getattr(torch, n) for n in names] + [getattr(torch.Tensor, n) for n in methods]
    assert all(a is b for a, b in zip(after, before))
    assert torch.empty is before[0]


def test_launch_ledger_counts_and_restores():
    class Handle:
        pass

    h = Handle()
    h.pd3_a = lambda x: x + 1
    h.pd3_b = lambda: 7
    fa, fb = h.pd3_a, h.pd3_b
    with launch_ledger(h, ("pd3_a", "pd3_b")) as calls:
        assert h.pd3_a is not fa and h.pd3_a.__wrapped__ is fa
        assert h.pd3_a(1) == 2 and h.pd3_a(5) == 6
        assert calls == {"pd3_a": 2, "pd3_b": 0}
    assert h.pd3_a is fa and h.pd3_b is fb
    with pytest.raises(KeyError):
        with launch_ledger(h, ("pd3_a", "pd3_b")) as calls:
            h.pd3_b()
            raise KeyError("x")
    assert calls == {"pd3_a": 0, "pd3_b": 1} and h.pd3_a is fa and h.pd3_b is fb


def test_launch_ledger_on_the_real_handle():
    from paddle3d_amd import _lib

    L = _lib.lib()
    orig = L.pd3_version
    with launch_ledger(_lib.lib(), _lib.symbols("test_memory_safety_gpu")) as calls:
        assert set(calls) == set(_lib.symbols("test_memory_safety_gpu"))
        v = L.pd3_version()
        assert _lib.lib().pd3_target_arch() == b"gfx950"
    assert calls["pd3_version"] == 1 and calls["pd3_target_arch"] == 1 and sum(calls.values()) == 2
    assert L.pd3_version is orig and L.pd3_version() == v and L.pd3_version.argtypes is not None


# ---- the Protocol on fake entry points --------------------------------------------------------------------------------
def _fake_protocol(**kw):
    """A Protocol over a handle whose two "entry points" are Python functions on CPU tensors."""
    h = types.SimpleNamespace(pd3_copy=lambda dst, src: dst.copy_(src),
                              pd3_double=lambda dst, src: torch.mul(src, 2, out=dst))
    return Protocol("fake_module", "protocol-self-test", "cpu", handle=h, symbols=("pd3_copy", "pd3_double"), **kw), h


torch_empty = torch.empty  # the unpatched function: what a before_pass hook has to see


def _x():
    return torch.randn(6, 4, generator=torch.Generator().manual_seed(1))


def _guarded_now(t):
    """True for a tensor carved out of a guarded buffer (the fake defects below need the bands to write into)."""
    return t.untyped_storage().nbytes() >= t.numel() * t.element_size() + 2 * G


def test_protocol_passes_a_clean_scenario_and_counts_its_calls():
    P, h = _fake_protocol()

    @P.scenario
    def clean():
        inputs = dict(x=_x())

        def call():
            out, two = torch.empty(6, 4), torch.empty_like(inputs["x"])
            h.pd3_copy(out, inputs["x"])
            h.pd3_double(two, inputs["x"])
            h.pd3_double(two, inputs["x"])
            return dict(out=out, two=two.numpy(), none=torch.full((3,), -1, dtype=torch.int32), __trivial_ok__={"none"})

        return inputs, call

    P.check_scenario("clean")
    assert P.ran == {"clean"} and P.ledger == {"pd3_copy": 1, "pd3_double": 2}  # the 0xFF pass's calls
    host, damage, changed, calls, trivial_ok = P.run("clean", "0xFF")
    assert torch.equal(host["out"], _x()) and torch.equal(host["two"], 2 * _x()) and trivial_ok == {"none"}
    assert damage == [] and changed == [] and calls == {"pd3_copy": 1, "pd3_double": 2}
    assert h.pd3_copy.__name__ == "<lambda>"  # the ledger's wrappers are gone


def _defect(body, **kw):
    """A Protocol with one scenario `bad` whose call() is body(handle, inputs)."""
    P, h = _fake_protocol(**kw)

    @P.scenario
    def bad():
        inputs = dict(x=_x())
        return inputs, lambda: body(h, inputs)

    return P


def _overrun(h, inputs):  # one element past the output
    out = torch.empty(6, 4)
    h.pd3_copy(out, inputs["x"])
    if _guarded_now(out):
        for b in range(4):
            _poke(out, out.numel() * 4 + b)
    return dict(out=out)


def _stale(h, inputs):  # the last row is never written
    out = torch.empty(6, 4)
    h.pd3_copy(out[:-1], inputs["x"][:-1])
    return dict(out=out)


def _writes_input(h, inputs):
    out = torch.empty(6, 4)
    h.pd3_copy(out, inputs["x"])
    h.pd3_double(inputs["x"], inputs["x"])
    return dict(out=out)


def _trivial(h, inputs):
    out, idx = torch.empty(6, 4), torch.full((5,), -1, dtype=torch.int32)
    h.pd3_copy(out, inputs["x"])
    return dict(out=out, idx=idx)


def _other_symbols(h, inputs):  # another path under the guard than in production
    out = torch.empty(6, 4)
    if _guarded_now(out):
        h.pd3_double(out, inputs["x"] / 2)
    else:
        h.pd3_copy(out, inputs["x"])
    return dict(out=out)


@pytest.mark.parametrize("body,message", [
    (_overrun, r"bad \[0x00\]: allocation #0 \(6, 4\) torch.float32: tail guard damaged at byte \+0"),
    (_stale, r"bad \[0x..\]: output out \(6, 4\) torch.float32 depends on the previous contents of memory: \d+ bytes differ "
             r"from the plain run, first at element 2\d \(plain .*, guarded (0.0|nan)\)"),
    (_writes_input, r"bad \[plain\]: inputs written: \['x'\]"),
    (_trivial, r"bad: output idx \(5,\) is empty or all 0 / -1"),
    (_other_symbols, r"bad \[0x00\]: other entry points ran than in the plain run: \['pd3_copy', 'pd3_double'\]"),
], ids=["overrun", "stale", "writes_input", "trivial", "other_symbols"])
def test_protocol_fails_each_defect_with_its_own_message(body, message):
    P = _defect(body)
    with pytest.raises(AssertionError, match=message):
        P.check_scenario("bad")
    assert P.ran == set() and P.ledger == {}  # a failed scenario counts for nothing


def test_protocol_tolerance_and_allocation_rules():
    def noisy(h, inputs):  # an order-dependent sum: the last bits differ from run to run
        acc = torch.zeros(6, 4, dtype=torch.float64)
        h.pd3_copy(acc, inputs["x"])
        return dict(grad_acc=acc + (1e-9 if _guarded_now(acc) else 0.0))

    with pytest.raises(AssertionError, match="depends on the previous contents"):
        _defect(noisy).check_scenario("bad")
    _defect(noisy, tolerant={("bad", "acc"): {torch.float64: 1e-8}}).check_scenario("bad")
    with pytest.raises(AssertionError, match=r"bad \[0x00\]: grad_acc: 1\.0\d*e-09 > \d"):  # (relative to max |plain|)
        _defect(noisy, tolerant={("bad", "acc"): {torch.float64: 1e-10}}).check_scenario("bad")
    with pytest.raises(KeyError):  # a dtype without a bound of its own is an error, not a default
        _defect(noisy, tolerant={("bad", "acc"): {torch.float32: 1e-4}}).check_scenario("bad")

    def allocates_nothing(h, inputs):
        return dict(n=np.array([3]))

    with pytest.raises(AssertionError, match=r"bad \[0x00\]: nothing allocated"):
        _defect(allocates_nothing).check_scenario("bad")
    seen = []
    P = _defect(allocates_nothing, may_allocate_nothing={"bad"}, before_pass=lambda: seen.append(torch.empty is torch_empty))
    P.check_scenario("bad")
    assert seen == [True] * 3  # the hook runs ahead of every pass, outside the guard


def test_protocol_completeness():
    P, h = _fake_protocol()

    @P.scenario
    def copies():
        inputs = dict(x=_x())

        def call():
            out = torch.empty(6, 4)
            h.pd3_copy(out, inputs["x"])
            return dict(out=out)

        return inputs, call

    P.check_scenario("copies")
    P.check_complete(["pd3_copy"], 1)
    with pytest.raises(AssertionError, match=r"1 of the 2 required entry points of fake_module are reached by no scenario: "
                                             r"\['pd3_double'\].*tests/fake_module.py"):
        P.check_complete(["pd3_copy", "pd3_double"], 2)
    with pytest.raises(AssertionError):  # the literal count a file states
        P.check_complete(["pd3_copy"], 2)

    @P.scenario
    def doubles():
        inputs = dict(x=_x())

        def call():
            out = torch.empty(6, 4)
            h.pd3_double(out, inputs["x"])
            return dict(out=out)

        return inputs, call

    assert P.ran == {"copies"}
    P.check_complete(["pd3_copy", "pd3_double"], 2)  # runs what did not run, in its plain form
    assert P.ran == {"copies", "doubles"} and P.ledger == {"pd3_copy": 1, "pd3_double": 1}
