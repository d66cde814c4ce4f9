"""Canary bands around every tensor argument of every native launch.

Every kernel launch of ``veon_amd`` goes through ``_lib.launch(name, device, *args)``
with tensors passed as tensors.  ``guarded()`` replaces that one attribute for the
duration of a ``with`` block.  Per launch it

* moves each distinct storage behind the tensor arguments into a fresh ``uint8``
  buffer ``band | storage.nbytes() | band`` filled with ``fill``; the slot starts at a
  multiple of 256 (PyTorch's own bases are at least that aligned, so a kernel takes
  the same aligned / vector path as without the guard) and a view keeps its offset
  into the storage.  ``storage.nbytes()`` is what the caller asked for, not the
  allocator's rounded block, so the first byte past a tensor is canary;
* calls the real launch with each tensor replaced by its relocated address
  (None, host arrays, byref structs and scalars pass unchanged);
* synchronises and requires every band byte to equal ``fill`` and every storage that
  is reached only through ``const`` parameters (const-ness read per parameter from
  include/veon_hip.h) to be byte-identical to what went in;
* copies every other storage back, so the wrapper's tensors hold the results.

The default fill 0xFF is NaN in fp32 / bf16 / fp16 and -1 in every integer type: an
out-of-range READ whose value is used poisons the output, and the reference
comparison of the wrapped test sees it.

Limits.  An out-of-range read whose value is DISCARDED is not detected.  Memory a
kernel reaches through a pointer table or a host struct (``veon_optim_update``'s
record table, ``veon_vit_block``'s weights) is not moved: only the tensor arguments
themselves are banded.  An overrun of more than ``band`` bytes leaves the buffer.

The function that performs the launch is a parameter, so the relocation can be
tested with CPU tensors and Python "kernels" that touch the relocated addresses with
``ctypes.memmove``; only the default path insists on device tensors.
"""
import contextlib
import os
import re
import time

import torch

from veon_amd import _lib
from veon_amd.build import INCLUDE

HEADER = os.path.join(INCLUDE, 'veon_hip.h')
LIMIT = 256 << 20       # bytes of storages per launch: the guard is for small shapes
ALIGN = 256


class GuardError(RuntimeError):
    """A launch the guard refuses to run (never a silent pass-through)."""


def parse_params(path=HEADER):
    """{entry point: [(parameter name, is_pointer, is_const), ...]} of every prototype of
    the header, the trailing ``void *stream`` included.  Same strict style as
    ``_lib._parse_header`` (which drops ``const``): a statement that is not a prototype,
    or a parameter without a name, raises."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', ' ', text)
    text = re.sub(r'typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;', ' ', text, flags=re.S)
    table = {}
    for stmt in text.split(';'):
        stmt = ' '.join(stmt.split())
        if stmt in ('', '}'):
            continue
        m = re.fullmatch(r'(.+?)\b(veon_\w+) ?\((.*)\)', stmt)
        if m is None or m.group(2) in table:
            raise ValueError('%s: not a prototype: %r' % (path, stmt))
        params = []
        args = m.group(3).strip()
        for decl in ([] if args == 'void' else args.split(',')):
            pm = re.fullmatch(r'\s*(.*?[\s*])(\w+)\s*', decl)
            if pm is None or not pm.group(1).replace('const', '').strip(' *'):
                raise ValueError('%s: %s: parameter without a name: %r'
                                 % (path, m.group(2), decl))
            head = pm.group(1)
            is_ptr = '*' in head
            is_const = is_ptr and 'const' in head[:head.index('*')].split()
            params.append((pm.group(2), is_ptr, is_const))
        table[m.group(2)] = params
    return table


PARAMS = parse_params()


def stream_entry_points(params=None):
    """The entry points that launch work: those ending in ``void *stream``."""
    params = PARAMS if params is None else params
    return sorted(n for n, p in params.items() if p and p[-1] == ('stream', True, False))


class Log(list):
    """Entry points launched, in order; ``unguarded``: (entry, position, parameter) of
    tensors left in place; ``seconds`` / ``inner_seconds``: wall time inside the guard and
    inside the real launch, their difference over ``len(self)`` is the per-launch cost."""

    def __init__(self):
        super().__init__()
        self.unguarded = []
        self.seconds = 0.0
        self.inner_seconds = 0.0
        self.bytes = 0


class _Slot:
    def __init__(self, storage, fill, band):
        self.storage = storage
        self.nbytes = storage.nbytes()
        self.src = torch.empty(0, dtype=torch.uint8, device=storage.device).set_(
            storage, 0, (self.nbytes,))
        self.buf = torch.full((band + self.nbytes + band + ALIGN - 1,), fill,
                              dtype=torch.uint8, device=storage.device)
        base = self.buf.data_ptr()
        self.off = (base + band + ALIGN - 1) // ALIGN * ALIGN - base
        self.addr = base + self.off
        self.inner = self.buf[self.off:self.off + self.nbytes]
        self.inner.copy_(self.src)
        self.args = []          # (position, parameter name, is_const)

    def who(self):
        return ', '.join('argument %d (%s)' % (i, n) for i, n, _ in self.args)


def _offsets(mask, shift):
    return [int(v) + shift for v in torch.nonzero(mask).flatten()[:8].tolist()]


def _guarded_launch(real, name, device, args, fill, band, limit, log, device_only):
    params = PARAMS.get(name)
    if params is None:
        raise GuardError('%s is not declared in %s' % (name, HEADER))
    if len(args) != len(params) - 1:
        raise GuardError('%s takes %d arguments before the stream, got %d'
                         % (name, len(params) - 1, len(args)))
    if device_only:
        for i, a in enumerate(args):
            if isinstance(a, torch.Tensor) and not a.is_cuda:
                raise GuardError('%s: argument %d (%s) is a %s tensor, not on the device'
                                 % (name, i, params[i][0], a.device))
        if torch.cuda.is_current_stream_capturing():
            raise GuardError('%s: launch while the stream is capturing' % name)
    slots, new_args = {}, list(args)
    for i, a in enumerate(args):
        if not isinstance(a, torch.Tensor):
            continue
        pname, is_ptr, is_const = params[i]
        if not is_ptr:
            raise GuardError('%s: argument %d (%s) is a tensor but not a pointer parameter'
                             % (name, i, pname))
        storage = a.untyped_storage()
        new_args[i] = a.data_ptr()
        if storage.nbytes() == 0:
            continue                              # nothing to band: the address stays
        if not storage.resizable():               # foreign memory (placement.py)
            log.unguarded.append((name, i, pname))
            continue
        key = storage.data_ptr()
        slot = slots.get(key)
        if slot is None:
            if sum(s.nbytes for s in slots.values()) + storage.nbytes() > limit:
                raise GuardError('%s: storages exceed %d bytes: the guard is for small '
                                 'shapes' % (name, limit))
            slot = slots[key] = _Slot(storage, fill, band)
        slot.args.append((i, pname, is_const))
        new_args[i] = slot.addr + (a.data_ptr() - storage.data_ptr())
    const_slots = [s for s in slots.values() if all(c for _, _, c in s.args)]
    kept = {id(s): s.inner.clone() for s in const_slots}
    log.append(name)
    log.bytes += sum(s.nbytes for s in slots.values())
    t0 = time.perf_counter()
    real(name, device, *new_args)
    log.inner_seconds += time.perf_counter() - t0
    if not slots:
        return
    flags = []
    for s in slots.values():
        front, back = s.buf[:s.off], s.buf[s.off + s.nbytes:]
        flags += [(front != fill).any(), (back != fill).any()]
        flags.append((s.inner != kept[id(s)]).any() if id(s) in kept
                     else torch.zeros((), dtype=torch.bool, device=s.buf.device))
    flags = torch.stack(flags).tolist()           # the one synchronisation per launch
    for k, s in enumerate(slots.values()):
        hit_front, hit_back, changed = flags[3 * k:3 * k + 3]
        if hit_front:
            raise AssertionError('%s: %s: front band overwritten at byte offsets %s of the '
                                 'slot (%d bytes)' % (name, s.who(), _offsets(
                                     s.buf[:s.off] != fill, -s.off), s.nbytes))
        if hit_back:
            raise AssertionError('%s: %s: back band overwritten at byte offsets %s of the '
                                 'slot (%d bytes)' % (name, s.who(), _offsets(
                                     s.buf[s.off + s.nbytes:] != fill, s.nbytes), s.nbytes))
        if changed:
            raise AssertionError('%s: %s: reached only through const pointers but changed '
                                 'at byte offsets %s' % (name, s.who(), _offsets(
                                     s.inner != kept[id(s)], 0)))
    for s in slots.values():
        if id(s) not in kept:
            s.src.copy_(s.inner)


@contextlib.contextmanager
def guarded(fill=0xFF, band=4096, launch=None, limit=None):
    """Run every ``_lib.launch`` of the block between canary bands (module docstring).
    ``launch``: the function that performs the launch, ``_lib.launch`` by default; with
    another one the tensors may live anywhere."""
    real = _lib.launch if launch is None else launch
    device_only = launch is None
    limit = LIMIT if limit is None else limit
    log = Log()

    def wrapper(name, device, *args):
        t0 = time.perf_counter()
        try:
            _guarded_launch(real, name, device, args, fill, band, limit, log, device_only)
        finally:
            log.seconds += time.perf_counter() - t0

    wrapper.__wrapped__ = real
    saved = _lib.launch
    _lib.launch = wrapper
    try:
        yield log
    finally:
        _lib.launch = saved
