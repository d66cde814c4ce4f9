"""The launch guard (tests/launch_guard.py) on the CPU: CPU tensors and fake "kernels",
Python functions that receive the relocated addresses and touch memory with
ctypes.memmove / memset strictly inside the slot and its bands, which the guard owns.
And the ledger: every stream-taking entry point of the header has a guarded row in
tests/test_launch_bounds_gpu.py, an arena test, or a written excuse."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import launch_guard as lg
from veon_amd import _lib

GELU = 'veon_gelu_bf16'            # (const void *y, void *h, int64_t n)
GELU_BWD = 'veon_gelu_bwd_bf16'    # (const void *dh, const void *y, void *dy, int64_t n)


def _run(kernel, name, *args, **kw):
    """One launch of ``name`` under the guard with ``kernel(name, device, *args)`` in the
    place of the native launch; -> the guard's log."""
    with lg.guarded(launch=kernel, **kw) as log:
        _lib.launch(name, None, *args)
    return log


def _poke(addr, value=7):
    ctypes.memset(addr, value, 1)


def test_write_one_byte_past_the_end_names_entry_argument_and_back_band():
    y, h = torch.zeros(37, 3, dtype=torch.bfloat16), torch.zeros(37, 3, dtype=torch.bfloat16)
    assert h.untyped_storage().nbytes() == 222          # the size asked for, not a rounded block

    def kernel(name, device, y_, h_, n):
        _poke(h_ + 222)
    with pytest.raises(AssertionError) as e:
        _run(kernel, GELU, y, h, 111)
    msg = str(e.value)
    assert GELU in msg and 'argument 1 (h)' in msg and 'back band' in msg and '[222]' in msg


def test_write_one_byte_before_the_start_names_the_front_band():
    y, h = torch.zeros(16), torch.zeros(16)

    def kernel(name, device, y_, h_, n):
        _poke(y_ - 1)
    with pytest.raises(AssertionError) as e:
        _run(kernel, GELU, y, h, 16)
    msg = str(e.value)
    assert GELU in msg and 'argument 0 (y)' in msg and 'front band' in msg and '[-1]' in msg


def test_last_band_byte_is_watched_and_the_slot_is_256_aligned():
    y, h = torch.zeros(5), torch.zeros(5)
    seen = {}

    def kernel(name, device, y_, h_, n):
        seen['y'], seen['h'] = y_, h_
        _poke(h_ + 20 + 4095)
    with pytest.raises(AssertionError, match='back band'):
        _run(kernel, GELU, y, h, 5)
    assert seen['y'] % 256 == 0 and seen['h'] % 256 == 0


def test_two_views_share_a_slot_keep_their_offset_and_are_copied_back_once():
    rows = torch.arange(40, dtype=torch.float32)
    tail = rows[12:]
    other = torch.zeros(3)
    seen = []

    def kernel(name, device, dh, y_, dy, n):
        seen.append((dh, y_, dy))
        ctypes.memmove(dy, (ctypes.c_float * 2)(5.0, 6.0), 8)            # rows[0:2]
        ctypes.memmove(dy + 4 * 39, (ctypes.c_float * 1)(9.0), 4)        # rows[39]
    log = _run(kernel, GELU_BWD, other, tail, rows, 3)
    dh, y_, dy = seen[0]
    assert y_ - dy == 12 * 4 and log.bytes == 40 * 4 + 3 * 4             # one slot for rows
    assert rows[:2].tolist() == [5.0, 6.0] and rows[39] == 9.0 and tail[-1] == 9.0
    assert torch.equal(rows[2:39], torch.arange(2, 39, dtype=torch.float32))


def test_an_off_alignment_view_keeps_its_offset():
    base = torch.zeros(64, dtype=torch.uint8)
    y, h = base[3:], torch.zeros(8)
    seen = []
    _run(lambda name, device, y_, h_, n: seen.append(y_), GELU, y, h, 8)
    assert seen[0] % 256 == 3


def test_a_const_only_storage_that_the_kernel_modifies_fails():
    y, h = torch.ones(8), torch.zeros(8)

    def kernel(name, device, y_, h_, n):
        _poke(y_ + 5)
    with pytest.raises(AssertionError) as e:
        _run(kernel, GELU, y, h, 8)
    assert 'argument 0 (y)' in str(e.value) and 'const' in str(e.value) and '[5]' in str(e.value)
    assert torch.equal(y, torch.ones(8))                 # and nothing was copied back


def test_a_storage_passed_both_const_and_non_const_is_not_flagged():
    buf = torch.zeros(16)

    def kernel(name, device, y_, h_, n):
        assert h_ - y_ == 32
        _poke(y_ + 1, 0x3F)
        _poke(h_, 1)
    _run(kernel, GELU, buf[:8], buf[8:], 8)
    assert buf.view(torch.uint8)[1] == 0x3F and buf.view(torch.uint8)[32] == 1


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_a_value_read_from_the_band_is_nan(dtype):
    y, h = torch.ones(6, dtype=dtype), torch.zeros(6, dtype=dtype)
    size = y.element_size()

    def kernel(name, device, y_, h_, n):
        ctypes.memmove(h_, y_ + size, 6 * size)          # reads one element past the end
    _run(kernel, GELU, y, h, 6)
    assert h[:5].tolist() == [1.0] * 5 and bool(torch.isnan(h[5]))


@pytest.mark.parametrize('dtype', [torch.int8, torch.int32, torch.int64])
def test_an_index_read_from_the_band_is_minus_one(dtype):
    y, h = torch.zeros(4, dtype=dtype), torch.zeros(4, dtype=dtype)
    size = y.element_size()

    def kernel(name, device, y_, h_, n):
        ctypes.memmove(h_, y_ - size, 4 * size)          # reads one element before the start
    _run(kernel, GELU, y, h, 4)
    assert h.tolist() == [-1, 0, 0, 0]


def test_results_of_an_in_bounds_kernel_reach_the_callers_tensors_and_the_log():
    y = torch.arange(10, dtype=torch.float32)
    h = torch.full((10,), -3.0)

    def kernel(name, device, y_, h_, n):
        assert name == GELU and device == 'dev' and n == 10
        ctypes.memmove(h_, y_, 40)
    with lg.guarded(launch=kernel) as log:
        _lib.launch(GELU, 'dev', y, h, 10)
        _lib.launch(GELU, 'dev', h, y, 10)
    assert torch.equal(h, torch.arange(10, dtype=torch.float32))
    assert log == [GELU, GELU] and log.unguarded == []
    assert log.seconds >= log.inner_seconds > 0.0


def test_none_scalars_and_host_arrays_pass_unchanged():
    strides = _lib.host_array([3, 2, 1])
    seen = []
    _run(lambda name, device, *a: seen.append(a), 'veon_occ_labels',
         torch.zeros(4), strides, 5, None, strides, *range(7), torch.zeros(4, dtype=torch.uint8),
         None, None, None)
    a = seen[0]
    assert a[1] is strides and a[2] == 5 and a[3] is None and a[-1] is None
    assert isinstance(a[0], int) and isinstance(a[12], int)


def test_launch_is_restored_after_an_exception_inside_the_block():
    before = _lib.launch
    with pytest.raises(KeyError):
        with lg.guarded(launch=lambda *a: None):
            assert _lib.launch is not before
            raise KeyError('x')
    assert _lib.launch is before

    def kernel(name, device, y_, h_, n):
        _poke(h_ + 4)
    with pytest.raises(AssertionError):
        _run(kernel, GELU, torch.zeros(1), torch.zeros(1), 1)
    assert _lib.launch is before


def test_the_size_limit_refuses():
    y, h = torch.zeros(100), torch.zeros(100)
    ran = []
    with pytest.raises(lg.GuardError, match='exceed'):
        _run(lambda *a: ran.append(a), GELU, y, h, 100, limit=799)
    assert not ran
    _run(lambda *a: ran.append(a), GELU, y, h, 100, limit=800)
    assert len(ran) == 1 and lg.LIMIT == 256 << 20


def test_the_default_path_refuses_a_tensor_that_is_not_on_the_device():
    before = dict(_lib.CALLS)
    with pytest.raises(lg.GuardError, match='not on the device'):
        with lg.guarded():
            _lib.launch(GELU, torch.device('cpu'), torch.zeros(8), torch.zeros(8), 8)
    assert _lib.CALLS == before


def test_unknown_entry_points_and_wrong_argument_counts_are_refused():
    with pytest.raises(lg.GuardError):
        _run(lambda *a: None, 'veon_no_such_kernel', torch.zeros(1))
    with pytest.raises(lg.GuardError):
        _run(lambda *a: None, GELU, torch.zeros(1), torch.zeros(1))
    with pytest.raises(lg.GuardError, match='not a pointer'):
        _run(lambda *a: None, GELU, torch.zeros(1), torch.zeros(1), torch.zeros(1))


def test_memory_torch_does_not_own_is_left_in_place_and_logged():
    foreign = torch.from_numpy(np.zeros(8, np.float32))
    h = torch.zeros(8)
    seen = []
    log = _run(lambda name, device, y_, h_, n: seen.append((y_, h_)), GELU, foreign, h, 8)
    assert seen[0][0] == foreign.data_ptr() and seen[0][1] != h.data_ptr()
    assert log.unguarded == [(GELU, 0, 'y')]


# ------------------------------------------------------------------ the const table
def test_every_prototype_parses_with_the_bindings_parameter_count():
    assert sorted(lg.PARAMS) == _lib.declared_symbols()
    for name, params in lg.PARAMS.items():
        assert len(params) == len(_lib._SIGNATURES[name][1]), name
        for (pname, is_ptr, is_const), ctype in zip(params, _lib._SIGNATURES[name][1]):
            assert is_ptr == (ctype is ctypes.c_void_p), (name, pname)
            assert is_ptr or not is_const
    assert len(lg.stream_entry_points()) >= 118


def _consts(name):
    return [(n, c) for n, p, c in lg.PARAMS[name] if p]


def test_hand_checked_const_patterns():
    assert _consts('veon_vit_gemm') == [
        ('a_bf16', True), ('w_bf16', True), ('bias', True), ('gamma', True),
        ('resid', False), ('out_bf16', False), ('stream', False)]
    assert _consts('veon_occ_labels') == [
        ('sem', True), ('sem_strides', True), ('bin', True), ('bin_strides', True),
        ('labels', False), ('gt', True), ('mask', True), ('hist', False), ('stream', False)]
    assert _consts('veon_optim_update') == [
        ('records', True), ('grad', True), ('exp_avg', False), ('exp_avg_sq', False),
        ('scal', True), ('host_scalars', True), ('stream', False)]
    assert _consts(GELU_BWD) == [('dh', True), ('y', True), ('dy', False), ('stream', False)]
    assert [n for n, p, c in lg.PARAMS['veon_vit_gemm'] if not p] == ['M', 'N', 'K', 'epilogue']


def test_the_parser_refuses_what_is_not_a_prototype(tmp_path):
    for text in ('int veon_a(const float *, void *stream);', 'int x;',
                 'int veon_a(int n); int veon_a(int n);'):
        path = tmp_path / 'h.h'
        path.write_text(text)
        with pytest.raises(ValueError):
            lg.parse_params(str(path))


# ------------------------------------------------------------------------ the ledger
REASONS = ('cannot be launched at a small shape',
           'touches no device memory through its arguments')


def test_ledger_closes_over_every_stream_taking_entry_point():
    from tests import test_launch_bounds_gpu as rows
    declared = set(lg.stream_entry_points())
    in_rows = set().union(*(r.entries for r in rows.ROWS))
    in_arena = set()
    here = os.path.dirname(os.path.abspath(__file__))
    for module, names in rows.ARENA_DIRECT.items():
        with open(os.path.join(here, module)) as f:
            text = f.read()
        for name in names:
            assert 'L.%s(' % name in text, (module, name)
        in_arena |= set(names)
    exempt = set(rows.EXEMPT)
    assert len(exempt) <= 6 and all(r in REASONS for r in rows.EXEMPT.values())
    assert not in_rows & in_arena, sorted(in_rows & in_arena)
    assert not in_rows & exempt and not in_arena & exempt
    union = in_rows | in_arena | exempt
    assert union - declared == set(), sorted(union - declared)
    assert declared - union == set(), sorted(declared - union)


def test_rows_name_existing_tests_and_have_unique_ids():
    import importlib
    from tests import test_launch_bounds_gpu as rows
    ids = [r.id for r in rows.ROWS]
    assert len(ids) == len(set(ids))
    for r in rows.ROWS:
        assert r.entries and r.flavour in ('bf16', 'fp16')
        if isinstance(r.target, tuple):
            assert callable(getattr(importlib.import_module(r.target[0]), r.target[1])), r.id


def test_every_size_function_has_a_row_at_exactly_its_size():
    from tests import test_launch_bounds_gpu as rows
    sized = {n for n, p in lg.PARAMS.items()
             if n.endswith(('_workspace_bytes', '_ints', '_stats_len', '_splitk_plan'))
             or n == 'veon_align_select_groups'}
    assert len(sized) >= 18 and not sized & set(lg.stream_entry_points())
    assert set(rows.EXACT_SIZE) == sized, sorted(sized ^ set(rows.EXACT_SIZE))
    ids = {r.id for r in rows.ROWS}
    assert set(rows.EXACT_SIZE.values()) <= ids, sorted(set(rows.EXACT_SIZE.values()) - ids)
