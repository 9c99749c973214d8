"""Poisoned, guard-banded buffers for the library's own allocations ("Memory
contract"; include/honk_hip.h: contents on entry are ignored, only bytes [0, bytes) are touched,
inputs are not modified).

``with arena(fill) as a:`` replaces torch.empty, torch.empty_like and torch.zeros for calls made
from files under honk_amd/ (decided by the caller's frame: the tests' own allocations and torch's
own are left alone).  Each such allocation becomes one uint8 allocation of G + nbytes + G bytes
filled with the byte ``fill``; the caller gets ``raw[G:G + nbytes].view(dtype).view(shape)``, so
the buffer keeps the allocator's alignment (G is a multiple of 512), holds ``fill`` in every byte
(torch.zeros: zeros) and has a guard on the very next byte after its last.  ``a.check()`` asserts
both guards of every allocation made so far still hold ``fill`` and names the allocation site and
the first dirty offset otherwise.

The fills are bytes: 0x00 is zero in every format; 0xFF is NaN as fp32 / bf16 / fp16 and -1 as an
integer; 0x3C is a small finite value (0.0115 as fp32 and bf16, 1.06 as fp16) -- there because
fmaxf, v_max and the f16x2 admission all swallow NaN.

``with frozen(*tensors):`` clones the tensors on entry and asserts bit-equality on exit."""
import os
import sys

import torch

G = 4096
FILLS = (0x00, 0xFF, 0x3C)
PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "honk_amd") + os.sep

_EMPTY, _EMPTY_LIKE, _ZEROS = torch.empty, torch.empty_like, torch.zeros


def _site(frame):
    """"honk_amd/<file>:<line>" if `frame` runs a file of the package, else None."""
    name = frame.f_code.co_filename
    if not os.path.abspath(name).startswith(PACKAGE):
        return None
    return f"honk_amd/{os.path.abspath(name)[len(PACKAGE):]}:{frame.f_lineno}"


def _shape(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _first_dirty(t, fill):
    bad = (t != fill).nonzero()
    return int(bad[0]) if bad.numel() else None


class arena:
    def __init__(self, fill):
        assert 0 <= fill <= 0xFF
        self.fill = fill
        self.allocations = []          # (raw, nbytes, site)
        self.tensors = []              # what each allocation returned, in the same order

    # ---- the replaced factories ------------------------------------------------------------
    def _alloc(self, site, shape, dtype, device, zero, extra):
        if set(extra) - {"requires_grad"} or extra.get("requires_grad"):
            raise NotImplementedError(f"poison_util: {site} allocates with {sorted(extra)}")
        dtype = dtype or torch.get_default_dtype()
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((G + nbytes + G,), self.fill, dtype=torch.uint8, device=device)
        body = raw[G:G + nbytes]
        if zero:
            body.zero_()
        self.allocations.append((raw, nbytes, site))
        self.tensors.append(body.view(dtype).view(shape))
        return self.tensors[-1]

    def buffer(self, shape, dtype, device, site="the test's own buffer"):
        """A poisoned, guard-banded buffer for a test that hands the C ABI a pointer itself."""
        return self._alloc(site, _shape((shape,)), dtype, device, False, {})

    def _empty(self, *size, dtype=None, device=None, **kw):
        site = _site(sys._getframe(1))
        if site is None:
            return _EMPTY(*size, dtype=dtype, device=device, **kw)
        return self._alloc(site, _shape(size), dtype, device, False, kw)

    def _zeros(self, *size, dtype=None, device=None, **kw):
        site = _site(sys._getframe(1))
        if site is None:
            return _ZEROS(*size, dtype=dtype, device=device, **kw)
        return self._alloc(site, _shape(size), dtype, device, True, kw)

    def _empty_like(self, t, dtype=None, device=None, **kw):
        site = _site(sys._getframe(1))
        if site is None:
            return _EMPTY_LIKE(t, dtype=dtype, device=device, **kw)
        # contiguous, as torch.empty_like of the contiguous (or expanded) tensors the package passes
        return self._alloc(site, tuple(t.shape), dtype or t.dtype, device or t.device, False, kw)

    def __enter__(self):
        assert torch.empty is _EMPTY, "arenas do not nest"
        torch.empty, torch.empty_like, torch.zeros = self._empty, self._empty_like, self._zeros
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, torch.zeros = _EMPTY, _EMPTY_LIKE, _ZEROS
        return False

    # ---- the checks ------------------------------------------------------------------------
    def sites(self):
        return [site for _, _, site in self.allocations]

    def typed(self):
        """[(site, tensor)] of the allocations that are not byte workspaces: the library's outputs,
        gradients and statistics, each of which a call writes in full (a workspace is uint8 and may
        keep regions nothing writes or reads)."""
        return [(a[2], t) for a, t in zip(self.allocations, self.tensors) if t.dtype != torch.uint8]

    def check(self):
        """Both guards of every allocation still hold the fill."""
        for raw, nbytes, site in self.allocations:
            lo = _first_dirty(raw[:G].flip(0), self.fill)
            assert lo is None, (f"{site}: {nbytes}-byte buffer, byte {-1 - lo} (before the buffer) was written "
                                f"(fill 0x{self.fill:02X})")
            hi = _first_dirty(raw[G + nbytes:], self.fill)
            assert hi is None, (f"{site}: {nbytes}-byte buffer, byte {nbytes + hi} (offset {hi} past the end) was "
                                f"written (fill 0x{self.fill:02X})")

    def untouched(self, t):
        """The flat indices of the elements of `t` whose every byte still holds the fill: what a call
        that promises to write all of `t` must leave empty (an element that a correct call writes
        with the fill's own pattern would show up too: use the fills' other two to tell)."""
        b = t.contiguous().view(-1).view(torch.uint8).view(-1, t.element_size())
        return (b == self.fill).all(dim=1).nonzero().view(-1).tolist()


class frozen:
    """Inputs are not modified: bit-equality of every tensor with its clone on entry."""

    def __init__(self, *tensors):
        self.tensors = [t for t in tensors if t is not None]

    def __enter__(self):
        self.before = [t.detach().clone() for t in self.tensors]
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            for i, (t, b) in enumerate(zip(self.tensors, self.before)):
                same = torch.equal(t.detach().contiguous().view(-1).view(torch.uint8),
                                   b.contiguous().view(-1).view(torch.uint8))
                assert same, f"input {i} (shape {tuple(t.shape)}, {t.dtype}) was modified"
        return False


def bits_equal(a, b):
    """Bit-equality of two tensors / arrays (NaN payloads and signed zeros included)."""
    import numpy as np
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
