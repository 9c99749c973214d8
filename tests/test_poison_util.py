"""poison_util.arena catches what it is for.  A fake "library" -- source text compiled here under
a file name inside honk_amd/, so the arena's caller-frame test takes it for the package -- plays
each kind of wrong call on CPU tensors: a write one byte past the buffer, one byte before it, an
output whose last element stays unwritten, a scratch element added in before it is written.
Each must fail check() or the comparison across fills, with the allocation site named; a
well-behaved fake passes, and an allocation from outside honk_amd/ is not intercepted."""
import os

import numpy as np
import pytest
import torch

import poison_util as pu

FAKE_FILE = os.path.join(pu.PACKAGE, "_fake_library.py")
FAKE = '''
import torch


def _bytes(t):                       # the raw storage behind a buffer, as a kernel's pointer sees it
    return torch.tensor([], dtype=torch.uint8).set_(t.untyped_storage())


def good(x):
    ws = torch.empty(x.numel() * 4 + 3, dtype=torch.uint8)       # line 10
    out = torch.empty_like(x)                                    # line 11
    acc = torch.zeros((), dtype=torch.float32)                   # line 12
    part = ws[:x.numel() * 4].view(torch.float32)
    part.copy_(x.view(-1) * 2)
    out.view(-1).copy_(part + 1)
    acc += out.sum()
    return out, acc


def one_past(x):
    ws = torch.empty(5, dtype=torch.uint8)                       # line 21
    off = ws.storage_offset()
    _bytes(ws)[off + 5] = 7
    return x + 1


def one_before(x):
    out = torch.empty(3, 2, dtype=torch.float32)                 # line 28
    off = out.storage_offset() * 4
    _bytes(out)[off - 1] = 7
    out.copy_(x)
    return out


def tail_unwritten(x):
    out = torch.empty_like(x)                                    # line 36
    out.view(-1)[:-1] = x.view(-1)[:-1] * 2
    return out


def scratch_read_first(x):
    ws = torch.empty(x.numel(), dtype=torch.float32)             # line 42
    ws[1:] = 0
    ws += x.view(-1)                                             # ws[0] was never written
    return ws.sum()
'''


@pytest.fixture(scope="module")
def fake():
    ns = {}
    exec(compile(FAKE, FAKE_FILE, "exec"), ns)
    return ns


X = torch.arange(6, dtype=torch.float32).reshape(3, 2) + 1


def _run(fn, fill):
    with pu.arena(fill) as a:
        with pu.frozen(X):
            res = fn(X)
    return a, res


def test_layout_of_an_intercepted_allocation(fake):
    for shape, dtype in (((3, 2), torch.float32), ((), torch.int32), ((5,), torch.uint8), ((0, 4), torch.float16)):
        with pu.arena(0x3C) as a:
            t = eval(compile("torch.empty(shape, dtype=dtype)", FAKE_FILE, "eval"), dict(torch=torch, shape=shape, dtype=dtype))
        raw, nbytes, site = a.allocations[-1]
        assert site == "honk_amd/_fake_library.py:1"
        assert t.shape == shape and t.dtype == dtype and t.is_contiguous()
        assert nbytes == t.numel() * t.element_size() and raw.numel() == 2 * pu.G + nbytes
        assert t.storage_offset() * t.element_size() == pu.G
        assert t.numel() == 0 or t.data_ptr() == raw.data_ptr() + pu.G    # (an empty tensor's pointer is null)
        assert bool((raw == 0x3C).all())
        a.check()
    # the fills as numbers
    with pu.arena(0xFF) as a:
        fake["good"](X)
    ws = a.allocations[0][0]
    assert a.sites() == ["honk_amd/_fake_library.py:10", "honk_amd/_fake_library.py:11", "honk_amd/_fake_library.py:12"]
    assert np.isnan(ws[:4].numpy().view(np.float32)).all() and np.isnan(ws[:2].numpy().view(np.float16)).all()
    assert ws[:4].numpy().view(np.int32)[0] == -1
    c = np.full(4, 0x3C, np.uint8)
    assert abs(c.view(np.float32)[0] - 0.0115) < 1e-4 and abs(float(c.view(np.float16)[0]) - 1.06) < 1e-2
    assert abs(float(torch.from_numpy(c[:2].copy()).view(torch.bfloat16)[0]) - 0.0115) < 1e-4


def test_torch_zeros_is_guarded_and_zero(fake):
    a, (out, acc) = _run(fake["good"], 0xFF)
    raw, nbytes, site = a.allocations[2]
    assert site.endswith(":12") and nbytes == 4
    assert bool((raw[:pu.G] == 0xFF).all()) and bool((raw[pu.G + 4:] == 0xFF).all())
    assert float(acc) == float((X * 2 + 1).sum())


def test_well_behaved_passes(fake):
    res = []
    for fill in pu.FILLS:
        a, (out, acc) = _run(fake["good"], fill)
        a.check()
        assert a.untouched(out) == []
        res.append((out.clone(), acc.clone()))
    for out, acc in res[1:]:
        assert pu.bits_equal(out, res[0][0]) and pu.bits_equal(acc, res[0][1])
    assert torch.equal(res[0][0], X * 2 + 1)


@pytest.mark.parametrize("fill", pu.FILLS)
def test_one_byte_past_the_end(fake, fill):
    a, _ = _run(fake["one_past"], fill)
    with pytest.raises(AssertionError, match=r"honk_amd/_fake_library\.py:21: 5-byte buffer, byte 5 \(offset 0 past"):
        a.check()


@pytest.mark.parametrize("fill", pu.FILLS)
def test_one_byte_before_the_buffer(fake, fill):
    a, out = _run(fake["one_before"], fill)
    assert torch.equal(out, X)
    with pytest.raises(AssertionError, match=r"honk_amd/_fake_library\.py:28: 24-byte buffer, byte -1 \(before"):
        a.check()


def test_unwritten_tail_of_an_output(fake):
    outs = {}
    for fill in pu.FILLS:
        a, out = _run(fake["tail_unwritten"], fill)
        a.check()                                  # (inside its bounds: the guards cannot see it)
        assert a.sites() == ["honk_amd/_fake_library.py:36"]
        assert a.untouched(out) == [5]             # the element, by the fill it still holds
        outs[fill] = out
    assert not pu.bits_equal(outs[0x00], outs[0xFF]) and not pu.bits_equal(outs[0x00], outs[0x3C])
    assert torch.isnan(outs[0xFF].view(-1)[5]) and torch.equal(outs[0xFF].view(-1)[:5], X.view(-1)[:5] * 2)


def test_scratch_read_before_it_is_written(fake):
    sums = {}
    for fill in pu.FILLS:
        a, s = _run(fake["scratch_read_first"], fill)
        a.check()
        assert a.sites() == ["honk_amd/_fake_library.py:42"]
        sums[fill] = s
    assert float(sums[0x00]) == float(X.sum())      # zero pages: the bug is invisible
    assert torch.isnan(sums[0xFF])                  # NaN fill: it poisons the result
    assert not pu.bits_equal(sums[0x3C], sums[0x00])  # a finite fill: a wrong finite result


def test_allocations_from_outside_the_package_are_left_alone():
    with pu.arena(0xFF) as a:
        t = torch.empty(4, dtype=torch.float32)
        z = torch.zeros(3)
        e = torch.empty_like(z)
        n = torch.nn.Linear(3, 2)      # torch's own allocations
    assert a.allocations == []
    assert t.storage_offset() == 0 and z.storage_offset() == 0 and e.storage_offset() == 0
    assert torch.empty is pu._EMPTY and torch.zeros is pu._ZEROS and torch.empty_like is pu._EMPTY_LIKE


def test_frozen_catches_a_modified_input():
    x = X.clone()
    with pu.frozen(x, None):
        x + 1
    with pytest.raises(AssertionError, match=r"input 0 \(shape \(3, 2\)"):
        with pu.frozen(x):
            x[2, 1] = -x[2, 1]
    z = torch.zeros(2)
    with pytest.raises(AssertionError, match="input 1"):
        with pu.frozen(x, z):
            z[0] = -0.0                # bit-equality: a signed zero counts
