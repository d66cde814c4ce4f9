"""ctypes binding of libveon_hip.so (the C ABI declared in include/veon_hip.h).

The product path has NO fallback: if the library is missing or a tensor is not
on a ROCm device, the call raises.  Pointers are passed as raw device addresses
(``tensor.data_ptr()``) and the launch goes to PyTorch's current HIP stream, so
the ops are hipGraph-capturable and race-free against surrounding torch ops
(the reference launches on the legacy default stream, bev_pool_cuda.cu:127,136).
"""
import ctypes
import os
import re

import torch

from . import half as _half
from .build import INCLUDE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libveon_hip.so')
LIB_PATHS = {'bf16': LIB_PATH, 'fp16': os.path.join(_HERE, 'libveon_hip_f16.so')}
# tools/lib_ab.py only: time another BUILD of the bf16 library in the same process tree
# (same-box A/B of kernel changes); never set in production
if os.environ.get('VEON_HIP_LIB'):
    LIB_PATHS['bf16'] = os.environ['VEON_HIP_LIB']
_libs = {}  # flavour -> loaded library


class VitBlockWeights(ctypes.Structure):
    """``veon_vit_block_weights`` of include/veon_hip.h."""
    _fields_ = [('ln1_w', ctypes.c_void_p), ('ln1_b', ctypes.c_void_p),
                ('w_qkv', ctypes.c_void_p), ('b_qkv', ctypes.c_void_p),
                ('w_proj', ctypes.c_void_p), ('b_proj', ctypes.c_void_p),
                ('gamma1', ctypes.c_void_p),
                ('ln2_w', ctypes.c_void_p), ('ln2_b', ctypes.c_void_p),
                ('w_fc1', ctypes.c_void_p), ('b_fc1', ctypes.c_void_p),
                ('w_fc2', ctypes.c_void_p), ('b_fc2', ctypes.c_void_p),
                ('gamma2', ctypes.c_void_p),
                ('ln1_eps', ctypes.c_float), ('ln2_eps', ctypes.c_float),
                ('mlp_dim', ctypes.c_int), ('act', ctypes.c_int),
                ('q_log2', ctypes.c_int)]


IMAGE_MAX_WINDOWS = 32


class ImageWindows(ctypes.Structure):
    """``veon_image_windows`` of include/veon_hip.h, passed by value."""
    _fields_ = [('n', ctypes.c_int), ('x0', ctypes.c_int * IMAGE_MAX_WINDOWS),
                ('y0', ctypes.c_int * IMAGE_MAX_WINDOWS),
                ('flip', ctypes.c_int * IMAGE_MAX_WINDOWS)]


LAYOUT_BZYXC = 0
LAYOUT_BCZYX = 1
FEAT_F32, FEAT_F16, FEAT_BF16 = 0, 1, 2


class VeonHipError(RuntimeError):
    pass


_C_TYPES = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
            'double': ctypes.c_double, 'unsigned': ctypes.c_uint,
            'veon_image_windows': ImageWindows}


def _ctype(decl, is_return=False):
    """ctypes type of one parameter (or of the return type) of a prototype of
    include/veon_hip.h; ValueError for anything the header's style does not allow."""
    if '*' in decl:
        if not is_return:
            return ctypes.c_void_p
        if decl.replace(' ', '') == 'constchar*':
            return ctypes.c_char_p
        raise ValueError(decl)
    words = [w for w in decl.split() if w != 'const']
    if is_return and words == ['void']:
        return None
    if not is_return and len(words) == 2:   # type + parameter name
        words = words[:1]
    if len(words) == 1 and words[0] in _C_TYPES:
        return _C_TYPES[words[0]]
    raise ValueError(decl)


def _parse_header(path):
    """{entry point: (restype, argtypes)} of every prototype ``ret veon_name(args);`` of
    the header (the style its opening comment states: C89 prototypes of scalar and
    pointer parameters, one typedef struct).  Every pointer is passed as c_void_p.  A
    statement that is not such a prototype raises: never a silent default."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)                        # comments
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)                       # preprocessor
    text = re.sub(r'extern\s+"C"\s*\{', ' ', text)
    text = re.sub(r'typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;', ' ', text, flags=re.S)
    table = {}
    for stmt in text.split(';'):
        stmt = ' '.join(stmt.split())
        if stmt in ('', '}'):            # '}' closes the extern "C" block
            continue
        m = re.fullmatch(r'(.+?)\b(veon_\w+) ?\((.*)\)', stmt)
        try:
            if m is None or m.group(2) in table:
                raise ValueError(stmt)
            args = m.group(3).strip()
            argtypes = [] if args == 'void' else [_ctype(a) for a in args.split(',')]
            table[m.group(2)] = (_ctype(m.group(1), is_return=True), argtypes)
        except ValueError:
            raise VeonHipError('%s: the binding cannot read the declaration %r' % (path, stmt))
    return table


# the C ABI, read once per process from the header the library is compiled against
_SIGNATURES = _parse_header(os.path.join(INCLUDE, 'veon_hip.h'))


def declared_symbols():
    """Every entry point include/veon_hip.h declares (checked by the CPU tests)."""
    return sorted(_SIGNATURES)


# Entry points declared outside veon_hip.h (include/ext/*.h, the same style): bound beside
# _SIGNATURES and exported by the same libraries, but not part of ``declared_symbols()``,
# over which the launch ledger of the tests closes.
EXT_HEADERS = (os.path.join(INCLUDE, 'ext', 'veon_hip_query.h'),)
_EXT_SIGNATURES = {}
for _path in EXT_HEADERS:
    for _name, _sig in _parse_header(_path).items():
        if _name in _SIGNATURES or _name in _EXT_SIGNATURES:
            raise VeonHipError('%s: %s is declared twice' % (_path, _name))
        _EXT_SIGNATURES[_name] = _sig


def ext_symbols():
    """Every entry point the headers under include/ext/ declare."""
    return sorted(_EXT_SIGNATURES)


def lib():
    """The native library of the process's half flavour (veon_amd/half.py):
    libveon_hip.so (bf16 operands) or libveon_hip_f16.so (fp16), the same entry
    points in both; raise (never fall back) when it is absent."""
    flavour = _half.name()
    loaded = _libs.get(flavour)
    if loaded is None:
        path = LIB_PATHS[flavour]
        if not os.path.exists(path):
            raise VeonHipError(
                'veon_amd: %s not found -- build it with `python -m veon_amd.build` '
                '(hipcc --offload-arch=gfx950). There is no CPU fallback.' % path)
        loaded = ctypes.CDLL(path)
        for name, (restype, argtypes) in list(_SIGNATURES.items()) + \
                list(_EXT_SIGNATURES.items()):
            fn = getattr(loaded, name)
            fn.restype, fn.argtypes = restype, argtypes
        if loaded.veon_half_mode() != (1 if flavour == 'fp16' else 0):
            raise VeonHipError('%s was not built for %s operands' % (path, flavour))
        _libs[flavour] = loaded
    return loaded


# number of native calls per entry point (every call ends in check()); the GPU
# tests assert on it so that a silent non-native path would be noticed
CALLS = {}


def check(status, what):
    CALLS[what] = CALLS.get(what, 0) + 1
    if status != 0:
        msg = lib().veon_status_string(status).decode()
        raise VeonHipError('%s failed: %s (status %d)' % (what, msg, status))


def require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise VeonHipError(
                'veon_amd HIP op called with a %s tensor: the op runs only on a '
                'ROCm device (no CPU path).' % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise VeonHipError('tensors on different devices: %s vs %s' % (dev, t.device))
    return dev


def require_half(*tensors):
    """Operands of the MFMA kernels must have THE half dtype of the process
    (veon_amd/half.py) -- a module built under the other flavour holds packed
    weights of the other type: raise, never reinterpret the bits."""
    want = _half.dtype()
    for t in tensors:
        if t is not None and t.dtype != want:
            raise VeonHipError(
                'half-precision operand is %s but this process runs the %s flavour of the '
                'library (VEON_HALF / veon_amd.half.set_half_dtype): build the module under '
                'the flavour it is used with' % (t.dtype, _half.name()))


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def host_array(values, ctype=ctypes.c_int64):
    """A small host array of ``ctype`` as a pointer argument of ``launch``.  The c_void_p
    keeps the array alive (ctypes.cast records its source in the result's ``_objects``)."""
    values = list(values)
    return ctypes.cast((ctype * len(values))(*values), ctypes.c_void_p)


def strides(t):
    """``t.stride()`` as the host ``int64_t[t.dim()]`` argument of the strided entry points."""
    return host_array(t.stride())


def stream_ptr(device):
    """PyTorch's current stream on ``device`` as a raw hipStream_t (no Stream
    object is built: this sits on every launch)."""
    idx = device.index
    if idx is None:
        idx = torch.cuda.current_device()
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def on_device(device):
    """``torch.cuda.device(device)`` unless it is the current device already
    (then a no-op context: the guard costs more than a small launch)."""
    if device.index is None or device.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(device)


def launch(name, device, *args):
    """Call entry point ``name`` on PyTorch's current stream of ``device``: a tensor
    argument becomes its device address, None becomes NULL, anything else is passed
    as it is; the stream goes last, as in every kernel entry point of the header."""
    fn = getattr(lib(), name)
    cargs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    with on_device(device):
        status = fn(*cargs, stream_ptr(device))
    check(status, name)
