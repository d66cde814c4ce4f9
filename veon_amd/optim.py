"""The parameter update that ends a training iteration: ``clip_grad_norm_`` (the configs'
``grad_clip=dict(max_norm=5, norm_type=2)``), AdamW (``lr=1e-4, weight_decay=1e-2``) and
the weight EMA of ``MEGVIIEMAHook`` (mmdet3d/core/hook/ema.py), fused.

On a ROCm device a step is three launches of csrc/optim_step.hip over flat fp32 arenas
(sum of squares per chunk, finish, update; one launch without clipping) whatever the number
of parameters; torch runs a few kernels per parameter and the reference's EMA three more per
``state_dict`` entry.  No host synchronisation, no allocation and no upload in steady state;
bit-reproducible.  The per-step scalars are launch arguments, so the step is launched and
never replayed from a captured graph.

``FusedAdamW``           the optimizer (clip and EMA folded in when asked for)
``ModelEMA``             the reference's class; alone it is one launch per update
``MEGVIIEMAHook``        the reference's hook as a plain class (no mmcv)
``adamw_ema_step_torch`` / ``grad_norm_torch``   the same arithmetic in elementary torch ops
                         at any dtype and device, in the kernels' order: the CPU path and
                         the tests' yardstick

Per element, fp32, one rounding per operation, in this order (all ``c_*`` are formed in
double on the host and rounded once, ``step_scalars``)::

    g = grad * coef                          coef = 1 without clipping
    p = p * c_decay                          c_decay = 1 - lr * weight_decay
    m = m + c_1mb1 * (g - m)                 c_1mb1 = 1 - beta1
    v = v * c_b2 + c_1mb2 * (g * g)          c_b2 = beta2, c_1mb2 = 1 - beta2
    p = p - c_step * (m / (sqrt(v) / c_bc2 + c_eps))
                                             c_step = lr / (1 - beta1^t), c_bc2 = sqrt(1 - beta2^t)
    e = e * c_d + c_1md * p                  c_d = d, c_1md = 1.0 - d

The last line is the reference's ``v *= d; v += (1.0 - d) * msd[k]`` to the bit.  The
clipped gradients are not written back to ``p.grad`` (torch scales them in place): nothing
reads them between the step and the next ``zero_grad``.
"""
import copy
import ctypes
import math
import os

import torch

from . import _lib

CHUNK = 4096          # elements per partial sum and per record: veon_optim_chunk()
FINISH_THREADS = 256  # the finish workgroup
SLOT = 4              # a tensor's arena slot starts at a multiple of 4 elements (16 bytes)
MAX_GROUPS = 8        # VEON_OPTIM_MAX_GROUPS
# longest chain of fp32 additions a squared element passes through in the chunk sums: 16 in
# its lane (the first onto 0), 6 butterfly steps, 4 waves (the first onto 0)
NORM_CHAIN = 16 + 6 + 4
_SCALAR_NAMES = ('c_decay', 'c_1mb1', 'c_b2', 'c_1mb2', 'c_step', 'c_bc2', 'c_eps')


# ------------------------------------------------------------------ scalars
def step_scalars(lr, betas, eps, weight_decay, step):
    """The seven per-group scalars of step ``step`` (1-based) in double, in the order of
    VEON_OPTIM_GROUP_SCALARS; the kernel's entry point and the mirror round them to fp32."""
    beta1, beta2 = betas
    return (1.0 - lr * weight_decay, 1.0 - beta1, beta2, 1.0 - beta2,
            lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step), eps)


def ema_scalars(d):
    return (d, 1.0 - d)


# ------------------------------------------------------------------ torch mirrors
def _scalar(x, like):
    """A 0-dim tensor of ``like``'s dtype and device: an op with it is the plain
    tensor-tensor op (a Python scalar divisor becomes a reciprocal multiply on a device).
    For fp32 the value is rounded once, as the entry point does."""
    if isinstance(x, torch.Tensor):
        return x.to(device=like.device, dtype=like.dtype)
    return torch.tensor(x, dtype=like.dtype, device=like.device)


def _sqrt(x):
    """The correctly rounded square root, as sqrtf in the kernel: torch's fp32 sqrt on the
    CPU is not (about 0.6 % of its results are one ulp off), the fp64 one rounded to fp32
    is, because a square root of an fp32 number never lies that close to a rounding tie."""
    return x.double().sqrt().to(x.dtype) if x.dtype == torch.float32 else x.sqrt()


def adamw_ema_step_torch(p, grad, exp_avg, exp_avg_sq, ema, coef, scalars, ema_c=None):
    """One update of one tensor IN PLACE, the sequence of the module docstring in
    elementary torch ops.  ``grad`` None: EMA only.  ``ema`` None: no EMA.  ``coef``: None
    (no clipping), a number or a 0-dim tensor; ``scalars``: ``step_scalars(...)``;
    ``ema_c``: ``ema_scalars(d)``."""
    with torch.no_grad():
        if grad is not None:
            c = {k: _scalar(v, p) for k, v in zip(_SCALAR_NAMES, scalars)}
            g = grad if coef is None else grad * _scalar(coef, p)
            p.mul_(c['c_decay'])
            exp_avg.add_(c['c_1mb1'] * (g - exp_avg))
            exp_avg_sq.mul_(c['c_b2']).add_(c['c_1mb2'] * (g * g))
            p.sub_(c['c_step'] * (exp_avg / (_sqrt(exp_avg_sq) / c['c_bc2'] + c['c_eps'])))
        if ema is not None:
            c_d, c_1md = (_scalar(v, ema) for v in ema_c)
            ema.mul_(c_d).add_(c_1md * p.to(ema.dtype))


def ema_line_torch(e, m, d):
    """The reference's two lines with its Python scalars, in place, at any dtype: the path
    of the entries the fp32 kernel cannot take.  For fp32 it equals the mirror bit for bit."""
    with torch.no_grad():
        e.mul_(d)
        e.add_((1.0 - d) * m.detach())


def _block_sum_torch(vals):
    """lane_reduce.h block_sum over (..., 256) lane values: the xor butterfly at distance
    32, 16, .., 1 inside each wave of 64, then the four waves added in index order from 0."""
    v = vals.reshape(*vals.shape[:-1], 4, 64)
    lane = torch.arange(64, device=v.device)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    total = torch.zeros_like(v[..., 0, 0])
    for w in range(4):
        total = total + v[..., w, 0]
    return total


def chunk_partials_torch(arena):
    """The per-chunk sums of squares of a flat arena (numel a multiple of CHUNK) in the
    order of k_optim_sumsq, in the arena's dtype."""
    x = arena.reshape(-1, CHUNK // (4 * FINISH_THREADS), FINISH_THREADS, 4)
    acc = torch.zeros_like(x[:, 0, :, 0])
    for j in range(x.shape[1]):
        for k in range(4):
            acc = acc + x[:, j, :, k] * x[:, j, :, k]
    return _block_sum_torch(acc)


def finish_torch(partials, max_norm):
    """k_optim_finish: (norm, coef) as 0-dim fp32 tensors from the chunk partials."""
    n = partials.numel()
    rows = -(-n // FINISH_THREADS)
    pad = partials.new_zeros(rows * FINISH_THREADS, dtype=torch.float64)
    pad[:n] = partials.to(torch.float64)
    pad = pad.reshape(rows, FINISH_THREADS)
    acc = torch.zeros_like(pad[0])
    for r in range(rows):
        acc = acc + pad[r]
    norm = _block_sum_torch(acc).sqrt().to(torch.float32)
    c = _scalar(max_norm, norm) / (norm + _scalar(1e-6, norm))
    return norm, torch.where(c > 1.0, torch.ones_like(c), c)


def grad_norm_torch(arena, max_norm=None):
    """The total gradient norm in the kernels' summation order.  ``arena``: the flat
    gradient arena (or any flat tensor; it is zero-padded to whole chunks, which adds exact
    zeros).  -> norm, or (norm, coef) with ``max_norm``."""
    flat = arena.reshape(-1)
    pad = -flat.numel() % CHUNK
    if pad or flat.numel() == 0:
        flat = torch.cat([flat, flat.new_zeros(pad or CHUNK)])
    norm, coef = finish_torch(chunk_partials_torch(flat), 1.0 if max_norm is None else max_norm)
    return norm if max_norm is None else (norm, coef)


# ------------------------------------------------------------------ records
def _records(entries):
    """The device table's rows for ``entries`` = [(p, ema or None, arena offset or -1,
    group)]: one row per piece of at most CHUNK elements, as int64 words
    (p address, ema address, offset, count | group << 32)."""
    rows = []
    for p, e, off, group in entries:
        n = p.numel()
        for s in range(0, n, CHUNK):
            rows.append((p.data_ptr() + 4 * s, e.data_ptr() + 4 * s if e is not None else 0,
                         off + s if off >= 0 else -1, min(CHUNK, n - s) | (group << 32)))
    return rows


def _upload_records(rows, device):
    table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
    return table.to(device)


def _check_native_tensor(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError('%s must be contiguous fp32, got %s with strides %s'
                         % (what, t.dtype, t.stride()))


# ------------------------------------------------------------------ EMA
def _unwrap(model):
    return model.module if hasattr(model, 'module') and isinstance(
        model.module, torch.nn.Module) else model


class ModelEMA:
    """The reference's ``ModelEMA`` (ema.py:17-59): a deep copy of the model in eval mode
    whose floating ``state_dict`` entries follow ``e = e * d + (1 - d) * model``, with
    ``d = decay * (1 - exp(-updates / 2000))``.  ``.ema``, ``.updates`` and ``.decay`` as
    there; ``update(trainer=None, model=None)`` takes the reference's arguments: the pairs
    are bound at construction, so a ``model`` that is not the one given there raises
    ``ValueError``, and so does an entry of either model whose storage has been replaced
    since (``model.to()``, ``p.data = ...``, a buffer assigned anew): the device table holds
    addresses.  ``.module`` wrappers are unwrapped.

    ``track='all'``: every floating entry, as the reference (frozen CLIP and DepthAnything
    weights included).  ``track='changing'``: parameters with ``requires_grad=False`` are
    left out (they equal the model's for ever); buffers stay.  An entry that shares its
    storage with an earlier one is updated once.

    Handed to ``FusedAdamW(ema=...)``, the entries of the trained parameters are updated
    inside the optimizer's update launch and all others by EMA-only records of the same
    launch, with the ``d`` of ``updates + 1``; ``update()`` then only advances ``updates``,
    so the order of an mmcv runner (optimizer hook, then ``MEGVIIEMAHook.after_train_iter``)
    stays as it is.  Used alone, ``update()`` is one launch on a ROCm device and the torch
    mirror on the CPU.  The kernel is fp32: on a device, an entry that is not contiguous fp32
    (half CLIP or DepthAnything weights) takes the torch line instead, one small torch
    sequence per such entry, alone and under ``FusedAdamW`` alike."""

    def __init__(self, model, decay=0.9999, updates=0, track='all'):
        if track not in ('all', 'changing'):
            raise ValueError("track must be 'all' or 'changing', got %r" % (track,))
        self.ema_model = copy.deepcopy(model).eval()
        self.ema = _unwrap(_unwrap(self.ema_model))
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / 2000))
        self.track = track
        for p in self.ema.parameters():
            p.requires_grad_(False)
        src = _unwrap(_unwrap(model))
        frozen = {id(p) for p in src.parameters() if not p.requires_grad}
        by_name = dict(src.named_parameters(remove_duplicate=False))
        msd = src.state_dict(keep_vars=True)
        self._source = src
        self.pairs = []           # (key, model tensor, ema tensor)
        self._homes = []          # (key, dict that holds the live tensor, its name, address)
        seen = set()
        for k, v in self.ema.state_dict().items():
            m = msd[k]
            if not v.dtype.is_floating_point or v.numel() == 0 or v.data_ptr() in seen:
                continue
            if track == 'changing' and k in by_name and id(by_name[k]) in frozen:
                continue
            seen.add(v.data_ptr())
            self.pairs.append((k, m.detach(), v))
            # the model's side only: nothing but this class writes the copy, and in place
            owner, name = src.get_submodule(k.rpartition('.')[0]), k.rpartition('.')[2]
            held = owner._parameters if name in owner._parameters else owner._buffers
            self._homes.append((k, held, name, m.data_ptr()))
        self._fused = False       # True: a FusedAdamW updates the entries
        self._table = None

    @staticmethod
    def native_ok(m, e):
        """The update kernel can take this pair: both contiguous fp32."""
        return all(t.dtype == torch.float32 and t.is_contiguous() for t in (m, e))

    def check_storage(self, model=None):
        """ValueError if ``model`` is not the bound one, or an entry's storage moved."""
        if model is not None and _unwrap(_unwrap(model)) is not self._source:
            raise ValueError('ModelEMA.update was handed another model than the one it was '
                             'built on; build a new ModelEMA for it')
        for k, held, name, address in self._homes:
            t = held.get(name)
            if t is None or t.data_ptr() != address:
                raise ValueError('state_dict entry %s no longer lives where ModelEMA bound it '
                                 '(model.to(), p.data = ..., a buffer assigned anew): build '
                                 'the ModelEMA, and its optimizer, after such a change' % k)

    def update(self, trainer=None, model=None):
        self.check_storage(model)
        self.updates += 1
        if self._fused or not self.pairs:
            return
        ema_c = ema_scalars(self.decay(self.updates))
        dev = self.pairs[0][2].device
        native = [(m, e) for _, m, e in self.pairs
                  if dev.type == 'cuda' and self.native_ok(m, e)]
        for _, m, e in self.pairs:
            if dev.type != 'cuda':
                adamw_ema_step_torch(m, None, None, None, e, None, None, ema_c)
            elif not self.native_ok(m, e):
                ema_line_torch(e, m, ema_c[0])
        if not native:
            return
        if self._table is None:
            self._table = _upload_records(_records([(m, e, -1, 0) for m, e in native]), dev)
        _lib.launch('veon_optim_update', dev, self._table, self._table.shape[0], None, None,
                    None, None, _lib.host_array(ema_c, ctypes.c_double), 0)


# ------------------------------------------------------------------ optimizer
class FusedAdamW(torch.optim.Optimizer):
    """AdamW with ``clip_grad_norm_(max_norm)`` and the weight EMA folded into its step.

    ``FusedAdamW(params, lr, betas, eps, weight_decay, max_norm=None, ema=None)``;
    ``ema``: a ``ModelEMA`` of the model that owns ``params``.  Up to 8 parameter groups,
    fp32 contiguous parameters.  ``amsgrad``, ``maximize``, ``capturable`` and
    ``differentiable`` are accepted so that an AdamW config can be passed on unchanged,
    and raise ``ValueError`` when set.

    The optimizer owns three flat fp32 arenas (gradients, ``exp_avg``, ``exp_avg_sq``; each
    tensor's slot padded to 16 bytes) and BINDS every ``p.grad`` to its view of the gradient
    arena: autograd then accumulates in place, the addresses never change, the record
    table is uploaded once and a step uploads nothing.  ``zero_grad()`` is one fill of the
    arena and ignores ``set_to_none`` (the views must survive).  ``step()`` checks by
    identity that every ``p.grad`` is still the bound view and raises ``ValueError``
    otherwise: ``model.zero_grad(set_to_none=True)`` and DDP's
    ``gradient_as_bucket_view=True`` both replace the tensors; ``attach_grads()`` binds
    them again.  It also compares every parameter's address (and, through the
    ``ModelEMA``, every EMA entry's) with the one in the record table and raises
    ``ValueError`` when one moved (``model.to()``, ``p.data = ...``): build the optimizer
    after such a change.

    A parameter backward never touched has a zero gradient and IS stepped (weight decay,
    decaying moments), where torch skips a parameter whose ``grad`` is None.  The reference
    trains with ``find_unused_parameters=False``, which assumes every parameter gets a
    gradient in every iteration; under that assumption the two agree.

    One step count per group, on the host.  ``grad_norm``: the device scalar of the last
    step's total norm before clipping (None without ``max_norm``); ``clip_grad_norm_()``
    returns the same; reading it is the caller's synchronisation.  ``state_dict()`` /
    ``load_state_dict()`` speak ``torch.optim.AdamW``'s format, so a checkpoint goes either
    way.  CPU parameters run the torch mirror."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 max_norm=None, ema=None, amsgrad=False, maximize=False, capturable=False,
                 differentiable=False):
        for name, flag in (('amsgrad', amsgrad), ('maximize', maximize),
                           ('capturable', capturable), ('differentiable', differentiable)):
            if flag:
                raise ValueError('FusedAdamW does not support %s=True' % name)
        if max_norm is not None and not float(max_norm) > 0:
            raise ValueError('max_norm must be positive or None, got %r' % (max_norm,))
        self.max_norm = None if max_norm is None else float(max_norm)
        self._built = False
        # the keys of torch.optim.AdamW's groups, so that a state_dict loads there
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False,
                        fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._build(ema)

    # -------------------------------------------------------------- construction
    def add_param_group(self, param_group):
        if self._built:
            raise ValueError('FusedAdamW lays its arenas out once: pass every parameter '
                             'group to the constructor')
        super().add_param_group(param_group)

    @staticmethod
    def _check_group(group):
        if not 0.0 <= group['lr'] or not 0.0 <= group['eps'] or not 0.0 <= group['weight_decay'] \
                or not all(0.0 <= b < 1.0 for b in group['betas']):
            raise ValueError('invalid lr / betas / eps / weight_decay: %r' % (
                {k: group[k] for k in ('lr', 'betas', 'eps', 'weight_decay')},))
        for name in ('amsgrad', 'maximize', 'capturable', 'differentiable'):
            if group.get(name):
                raise ValueError('FusedAdamW does not support %s=True' % name)

    def _build(self, ema):
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError('FusedAdamW takes at most %d parameter groups, got %d'
                             % (MAX_GROUPS, len(self.param_groups)))
        self._slots = []            # (group index, index in group, parameter, offset)
        self._addresses = []        # p.data_ptr() of each slot, as the record table has it
        off, dev = 0, None
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            for pi, p in enumerate(group['params']):
                _check_native_tensor(p, self._name(gi, pi, p))
                if dev is not None and p.device != dev:
                    raise ValueError('parameters on different devices: %s and %s'
                                     % (dev, p.device))
                dev = p.device
                self._slots.append((gi, pi, p, off))
                self._addresses.append(p.data_ptr())
                off += -(-p.numel() // SLOT) * SLOT
        self._device = dev
        self._numel = max(CHUNK, -(-off // CHUNK) * CHUNK)   # whole chunks, zero padding
        self._native = dev.type == 'cuda'
        arenas = torch.zeros(3, self._numel, dtype=torch.float32, device=dev)
        self._grad_arena, self._m_arena, self._v_arena = arenas[0], arenas[1], arenas[2]
        self._views = [self._grad_arena[o:o + p.numel()].view_as(p)
                       for _, _, p, o in self._slots]
        self._steps = [0] * len(self.param_groups)
        self._partials = torch.zeros(self._numel // CHUNK, dtype=torch.float32, device=dev)
        self._scal = torch.zeros(2, dtype=torch.float32, device=dev)   # norm, coef
        self._norm, self._coef = self._scal[0], self._scal[1]
        self.attach_grads()

        self._ema = ema
        self._ema_of = {}           # id(parameter) -> ema tensor
        self._ema_rest, self._ema_torch = [], []
        entries = []
        if ema is not None:
            if ema._fused:
                raise ValueError('this ModelEMA already belongs to an optimizer')
            by_ptr = {p.data_ptr(): p for _, _, p, _ in self._slots if p.numel()}
            rest, by_torch = [], []
            for k, m, e in ema.pairs:
                if e.device != dev:
                    raise ValueError('EMA entry %s is on %s, the parameters on %s'
                                     % (k, e.device, dev))
                p = by_ptr.get(m.data_ptr())
                if p is not None and p.numel() == m.numel() and ema.native_ok(m, e):
                    self._ema_of[id(p)] = e
                elif self._native and not ema.native_ok(m, e):
                    by_torch.append((k, m, e))     # not fp32: the torch line, after the launch
                else:
                    rest.append((k, m, e))
            self._ema_rest, self._ema_torch = rest, by_torch
            ema._fused = True
            entries = [(m, e, -1, 0) for _, m, e in rest]
        entries = [(p, self._ema_of.get(id(p)), o, gi) for gi, _, p, o in self._slots] + entries
        self._table = None
        if self._native:
            rows = _records(entries)
            self._n_records = len(rows)
            if rows:
                self._table = _upload_records(rows, dev)
        self._built = True

    def _name(self, gi, pi, p):
        names = self.param_groups[gi].get('param_names')
        label = names[pi] if names else 'parameter %d' % pi
        return '%s of group %d, shape %s' % (label, gi, tuple(p.shape))

    # -------------------------------------------------------------- gradients
    def attach_grads(self):
        """Bind every ``p.grad`` to its view of the gradient arena (again); a gradient that
        sits elsewhere is copied in first."""
        with torch.no_grad():
            for (_, _, p, _), view in zip(self._slots, self._views):
                if p.grad is not view:
                    if p.grad is not None:
                        view.copy_(p.grad)
                    p.grad = view

    def zero_grad(self, set_to_none=True):
        """One fill of the gradient arena; ``set_to_none`` is ignored."""
        self._grad_arena.zero_()

    def _check_bound(self):
        for (gi, pi, p, _), view, address in zip(self._slots, self._views, self._addresses):
            if p.data_ptr() != address:
                raise ValueError(
                    '%s no longer lives where FusedAdamW bound it (model.to(), p.data = '
                    '...): build the optimizer after such a change' % self._name(gi, pi, p))
            if p.grad is not view:
                raise ValueError(
                    '%s: p.grad is no longer the view FusedAdamW bound (zero_grad('
                    'set_to_none=True) on the module and DDP gradient_as_bucket_view=True '
                    'replace it); call attach_grads() after whatever replaced it'
                    % self._name(gi, pi, p))
        if self._ema is not None:
            self._ema.check_storage()

    @property
    def grad_arena(self):
        """The flat fp32 gradient arena every ``p.grad`` is a view of (padding is zero and
        must stay zero)."""
        return self._grad_arena

    def counts(self):
        """Elements and table rows of a step: ``trained``, ``ema_only`` (elements of the
        ``ema_only_entries`` EMA-only entries the kernel updates), ``arena`` (with padding)
        and ``records`` (None on the CPU)."""
        return dict(trained=sum(p.numel() for _, _, p, _ in self._slots),
                    ema_only=sum(e.numel() for _, _, e in self._ema_rest),
                    ema_only_entries=len(self._ema_rest),
                    arena=self._numel, records=self._n_records if self._native else None)

    @property
    def grad_norm(self):
        """Device scalar: the total norm before clipping of the last ``step()`` or
        ``clip_grad_norm_()``; None without ``max_norm``."""
        return None if self.max_norm is None else self._norm

    def clip_grad_norm_(self):
        """The total gradient norm as a device scalar, and the coefficient the next
        ``step()`` would apply; the gradients themselves are not scaled (module
        docstring).  ``step()`` runs this itself."""
        if self.max_norm is None:
            raise ValueError('FusedAdamW was built without max_norm')
        if self._native:
            _lib.launch('veon_optim_sumsq', self._device, self._grad_arena, self._numel,
                        self._partials)
            _lib.launch('veon_optim_clip_finish', self._device, self._partials,
                        self._partials.numel(), self.max_norm, self._scal)
        else:
            norm, coef = grad_norm_torch(self._grad_arena, self.max_norm)
            self._norm.copy_(norm)
            self._coef.copy_(coef)
        return self._norm

    # -------------------------------------------------------------- step
    def _host_scalars(self):
        # the d of the update() that follows this step (it only counts)
        d = self._ema.decay(self._ema.updates + 1) if self._ema is not None else 0.0
        vals = list(ema_scalars(d))
        for group, step in zip(self.param_groups, self._steps):
            vals += step_scalars(group['lr'], group['betas'], group['eps'],
                                 group['weight_decay'], step)
        return vals

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_bound()
        for group in self.param_groups:
            self._check_group(group)
        self._steps = [s + 1 for s in self._steps]
        if self.max_norm is not None:
            self.clip_grad_norm_()
        vals = self._host_scalars()
        if self._native:
            _lib.launch('veon_optim_update', self._device, self._table, self._n_records,
                        self._grad_arena, self._m_arena, self._v_arena,
                        self._scal if self.max_norm is not None else None,
                        _lib.host_array(vals, ctypes.c_double), len(self.param_groups))
            for _, m, e in self._ema_torch:
                ema_line_torch(e, m, vals[0])
            return loss
        coef = self._coef if self.max_norm is not None else None
        ema_c = vals[:2]
        for gi, _, p, o in self._slots:
            n = p.numel()
            adamw_ema_step_torch(p, self._grad_arena[o:o + n].view_as(p),
                                 self._m_arena[o:o + n].view_as(p),
                                 self._v_arena[o:o + n].view_as(p), self._ema_of.get(id(p)),
                                 coef, vals[2 + 7 * gi:9 + 7 * gi], ema_c)
        for _, m, e in self._ema_rest:
            adamw_ema_step_torch(m, None, None, None, e, None, None, ema_c)
        return loss

    # -------------------------------------------------------------- checkpoints
    def state_dict(self):
        """``torch.optim.AdamW``'s format: per parameter ``step`` (fp32 scalar tensor),
        ``exp_avg`` and ``exp_avg_sq`` (copies), once the group has stepped."""
        for gi, _, p, o in self._slots:
            if self._steps[gi]:
                n = p.numel()
                self.state[p] = dict(
                    step=torch.tensor(float(self._steps[gi]), dtype=torch.float32),
                    exp_avg=self._m_arena[o:o + n].view_as(p).clone(),
                    exp_avg_sq=self._v_arena[o:o + n].view_as(p).clone())
        try:
            return super().state_dict()
        finally:
            self.state.clear()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        try:
            for group in self.param_groups:
                self._check_group(group)
            steps = [set() for _ in self.param_groups]
            self._m_arena.zero_()
            self._v_arena.zero_()
            for gi, pi, p, o in self._slots:
                st = self.state.get(p)
                if not st:
                    steps[gi].add(0)
                    continue
                if st.get('max_exp_avg_sq') is not None:
                    raise ValueError('the state holds amsgrad buffers')
                steps[gi].add(int(st['step']))
                n = p.numel()
                self._m_arena[o:o + n].view_as(p).copy_(st['exp_avg'])
                self._v_arena[o:o + n].view_as(p).copy_(st['exp_avg_sq'])
            for gi, s in enumerate(steps):
                if len(s) > 1:
                    raise ValueError('group %d holds parameters at different steps %s; '
                                     'FusedAdamW keeps one count per group' % (gi, sorted(s)))
            self._steps = [s.pop() if s else 0 for s in steps]
        finally:
            self.state.clear()


# ------------------------------------------------------------------ hook
class MEGVIIEMAHook:
    """The reference's ``MEGVIIEMAHook`` (ema.py:63-122) as a plain class with the hook
    methods it defines (no mmcv import): call them from a hand-written loop, or derive a
    class from this one and ``mmcv.runner.Hook`` to register it with a runner
    (INTEGRATION.md).  ``track``: as ``ModelEMA``.  ``before_run`` builds
    ``runner.ema_model``; hand that to ``FusedAdamW(ema=runner.ema_model)`` to fold the
    update into the optimizer's step."""

    def __init__(self, init_updates=0, decay=0.9990, resume=None, track='all'):
        self.init_updates = init_updates
        self.resume = resume
        self.decay = decay
        self.track = track

    def before_run(self, runner):
        # a SyncBatchNorm's process group cannot be deep-copied: park them around the copy
        parked = [(m, m.process_group) for m in runner.model.modules()
                  if isinstance(m, torch.nn.SyncBatchNorm)]
        for m, _ in parked:
            m.process_group = None
        try:
            runner.ema_model = ModelEMA(runner.model, self.decay, track=self.track)
        finally:
            for m, group in parked:
                m.process_group = group
        runner.ema_model.updates = self.init_updates
        if self.resume is not None:
            self._log(runner, 'resume ema checkpoint from %s' % self.resume)
            cpt = torch.load(self.resume, map_location='cpu')
            runner.ema_model.ema.load_state_dict(cpt['state_dict'], strict=False)
            runner.ema_model.updates = cpt['updates']

    def after_train_iter(self, runner):
        runner.ema_model.update(runner, _unwrap(runner.model))

    def after_train_epoch(self, runner):
        self.save_checkpoint(runner)

    def save_checkpoint(self, runner):
        """Rank 0 only: ``epoch_{n}_ema.pth`` in ``runner.work_dir``."""
        if torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_rank() != 0:
            return
        ema_checkpoint = {'epoch': runner.epoch,
                          'state_dict': runner.ema_model.ema.state_dict(),
                          'updates': runner.ema_model.updates}
        save_path = os.path.join(runner.work_dir, 'epoch_%d_ema.pth' % (runner.epoch + 1))
        torch.save(ema_checkpoint, save_path)
        self._log(runner, 'Saving ema checkpoint at %s' % save_path)

    @staticmethod
    def _log(runner, msg):
        logger = getattr(runner, 'logger', None)
        if logger is not None:
            logger.info(msg)
