"""GPU checks of the native camera-input preparation (csrc/image_inputs.hip through
``veon_amd.image_inputs.prepare_images``).

The uint8 images are compared with the recordings of the reference's ``img_transform_core``
on Pillow (tests/golden/image_inputs_tiny.npz), byte for byte.  ``imgs`` and the ``midas``
output are compared, exactly, with the numpy restatements of tests/image_inputs_refs.py on
those images: mmcv was absent where the fixture was made, so these are restatements and
not recordings.  The depthanythingv2 tail is compared with the fp64 restatement of the
cubic definition (unpinned against cv2, absent too) within a bound computed here from the
restatement's own magnitude sums.  No test needs Pillow or the reference tree."""
import numpy as np
import pytest
import torch

from tests import image_inputs_refs as refs
from tests.conftest import load_golden
from veon_amd import _lib, image_inputs as ii

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H_ENTRY, V_ENTRY, C_ENTRY = ('veon_image_resample_h', 'veon_image_resample_v_finish',
                             'veon_image_cubic_norm')


@pytest.fixture(scope='module')
def golden():
    return load_golden('image_inputs_tiny')


def calls():
    return [_lib.CALLS.get(e, 0) for e in (H_ENTRY, V_ENTRY, C_ENTRY)]


def row_args(row):
    cfg = refs.TABLE[row]
    dw, dh = refs.depth_dims(cfg['cams'][0][0])
    return (cfg['resize_dims'], [c for c, _ in cfg['cams']], [f for _, f in cfg['cams']]), \
        (dh, dw)


def row_call(row, frames, **kw):
    args, depth_size = row_args(row)
    return ii.prepare_images(frames, *args, depth_size=depth_size, depth_norm='midas',
                             return_canvas=True, **kw)


def launches(row):
    """(horizontal, vertical + finish) launches of one call on a table row: the image and
    its depth resize, a pass that keeps its size skipped."""
    cfg = refs.TABLE[row]
    (dw, dh), c = refs.depth_dims(cfg['cams'][0][0]), cfg['cams'][0][0]
    return int(cfg['resize_dims'][0] != cfg['size'][1]) + int(dw != c[2] - c[0]), 2


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize('row,batch', [(r, 1) for r in sorted(refs.TABLE)] +
                         [(refs.BATCH2_ROW, 2)])
def test_table_rows_equal_reference(golden, row, batch):
    frames = refs.table_frames(row, batch)
    before = calls()
    res = row_call(row, torch.from_numpy(frames).to(DEV), norm='mmlab')
    n_h, n_v = launches(row)
    assert calls() == [before[0] + n_h, before[1] + n_v, before[2]]
    res = {k: v.cpu() for k, v in res.items()}
    assert res['imgs'].dtype == torch.float32 and res['canvas'].dtype == torch.uint8
    for b in range(batch):
        for n in range(2):
            key = 'r%d_b%d_c%d' % (row, b, n)
            assert torch.equal(res['canvas'][b, n], torch.from_numpy(golden[key + '_img']))
            assert torch.equal(res['depth_canvas'][b, n],
                               torch.from_numpy(golden[key + '_depth']))
            assert torch.equal(res['imgs'][b, n], torch.from_numpy(
                refs.normalize_ref(golden[key + '_img'], 'mmlab')))
            assert torch.equal(res['depth_img_inputs'][b, n], torch.from_numpy(
                refs.midas_ref(golden[key + '_depth'])))


def test_clipsan_and_custom_norm(golden):
    frames = torch.from_numpy(refs.table_frames(7)).to(DEV)
    args, _ = row_args(7)
    custom = ([1.5, 2.25, 100.0], [3.0, 7.0, 0.1])
    for norm in ('clipsan', custom):
        got = ii.prepare_images(frames, *args, norm=norm)
        assert sorted(got) == ['imgs']
        for n in range(2):
            assert torch.equal(got['imgs'][0, n].cpu(), torch.from_numpy(
                refs.normalize_ref(golden['r7_b0_c%d_img' % n], norm)))


def test_production_strip(golden):
    """900 x 1600 -> 792 x 1408, window (0, 280, 1408, 792): the production tables."""
    s = refs.STRIP
    frame = torch.from_numpy(refs.make_frame(s['seed'], *s['size']))[None, None].to(DEV)
    res = ii.prepare_images(frame, s['resize_dims'], s['crop'], s['flip'], depth_size=(256, 704),
                            depth_norm='midas', return_canvas=True)
    assert tuple(res['imgs'].shape) == (1, 1, 3, 512, 1408)
    canvas, depth = res['canvas'][0, 0].cpu(), res['depth_canvas'][0, 0].cpu()
    assert torch.equal(canvas[s['rows']][:, s['cols']], torch.from_numpy(golden['strip_img']))
    rows, cols = [r // 2 for r in s['rows'][::2]], [c // 2 for c in s['cols'][::2]]
    assert torch.equal(depth[rows][:, cols], torch.from_numpy(golden['strip_depth']))
    # the whole window against the mirror on the device, and imgs from the whole canvas
    mirror = ii.prepare_images_torch(frame, s['resize_dims'], s['crop'], s['flip'],
                                     depth_size=(256, 704), depth_norm='midas',
                                     return_canvas=True)
    for k in ('canvas', 'depth_canvas', 'imgs', 'depth_img_inputs'):
        assert torch.equal(res[k], mirror[k]), k
    assert torch.equal(res['imgs'][0, 0].cpu(),
                       torch.from_numpy(refs.normalize_ref(canvas.numpy(), 'mmlab')))


# ------------------------------------------------------------------ every element written
def test_prefilled_outputs_come_back_written():
    row = 1
    frames = torch.from_numpy(refs.table_frames(row)).to(DEV)
    want = row_call(row, frames)
    out = {k: torch.full_like(v, float('nan')) if v.dtype == torch.float32
           else torch.full_like(v, 0xAB) for k, v in want.items()}
    got = row_call(row, frames, out=out)
    for k, v in want.items():
        assert got[k] is out[k]
        assert torch.equal(got[k], v), k
    assert not bool(torch.isnan(out['imgs']).any())
    with pytest.raises(_lib.VeonHipError):
        row_call(row, frames, out={'imgs': torch.empty(1, 2, 3, 32, 63, device=DEV)})


def test_native_argument_checks():
    """The entry points refuse a window outside the image themselves."""
    src = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    canvas = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=DEV)
    for x0, y0, n in [(5, 0, 1), (0, 5, 1), (-1, 0, 1), (0, 0, 0), (0, 0, 33)]:
        win = _lib.ImageWindows()
        win.n, win.x0[0], win.y0[0] = n, x0, y0
        with pytest.raises(_lib.VeonHipError, match='status 1'):
            _lib.launch(V_ENTRY, src.device, src, 1, 8, 8, 0, 8, None, None, 0, win, 4, 4,
                        None, 1, canvas, None)


# ------------------------------------------------------------------ steady state
def test_second_call_uploads_nothing():
    row = 4
    first = torch.from_numpy(refs.table_frames(row)).to(DEV)
    second = torch.from_numpy(refs.table_frames(row)[:, ::-1].copy()).to(DEV)
    row_call(row, first)
    uploads = ii.UPLOADS
    tables = {k: tuple(t.data_ptr() for t in v) for k, v in ii._DEVICE_COEFFS.items()}
    luts = {k: v.data_ptr() for k, v in ii._DEVICE_LUTS.items()}
    got = row_call(row, second)
    assert ii.UPLOADS == uploads
    assert {k: tuple(t.data_ptr() for t in v) for k, v in ii._DEVICE_COEFFS.items()} == tables
    assert {k: v.data_ptr() for k, v in ii._DEVICE_LUTS.items()} == luts
    args, depth_size = row_args(row)
    want = ii.prepare_images_torch(second.cpu(), *args, depth_size=depth_size,
                                   depth_norm='midas', return_canvas=True)
    for k, v in want.items():
        assert torch.equal(got[k].cpu(), v), k


# ------------------------------------------------------------------ depthanythingv2 tail
def test_depthanything_tail_within_bound():
    """fp32 kernel against the fp64 restatement of the cubic definition (unpinned against
    cv2): |difference| <= sum |w_y| |w_x| |p| * 2^-24 * chain / std per output, the chain
    counted in ``refs.CUBIC_CHAIN``; bright frames, for which that bound covers the
    roundings after the sums (``refs.make_bright_frame``)."""
    h, w = 16, 44                                      # the aspect of 256 x 704
    frames = np.stack([refs.make_bright_frame(40 + n, h, w) for n in range(2)])[None]
    before = calls()
    res = ii.prepare_images(torch.from_numpy(frames).to(DEV), (w, h), (0, 0, w, h),
                            depth_norm='depthanythingv2')
    assert calls() == [before[0], before[1] + 1, before[2] + 1]
    got = res['depth_img_inputs'].cpu()
    assert tuple(got.shape) == (1, 2, 3, 252, 700) and got.dtype == torch.float32
    worst = 0.0
    for n in range(2):
        want, bound = refs.cubic_norm_ref(frames[0, n], 252, 700)
        err = np.abs(got[0, n].numpy().astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all())
    print('depthanythingv2 tail: worst error / bound = %.3f' % worst)


def test_depthanything_tail_after_depth_resize():
    """The chained path (window -> depth resize -> cubic tail) equals the tail on the
    recorded depth image, bit for bit: the same kernel on the same bytes."""
    frames = torch.from_numpy(refs.table_frames(1)).to(DEV)
    args, depth_size = row_args(1)
    res = ii.prepare_images(frames, *args, depth_size=depth_size,
                            depth_norm='depthanythingv2', return_canvas=True)
    dh, dw = depth_size
    alone = ii.prepare_images(res['depth_canvas'].contiguous(), (dw, dh), (0, 0, dw, dh),
                              depth_norm='depthanythingv2')
    assert tuple(res['depth_img_inputs'].shape[-2:]) == ii.depthanything_size(dh, dw)
    assert torch.equal(res['depth_img_inputs'], alone['depth_img_inputs'])
    mirror = ii.cubic_norm_torch(res['depth_canvas'])
    assert torch.allclose(res['depth_img_inputs'], mirror, rtol=0, atol=1e-5)


# ------------------------------------------------------------------ graph capture
def test_graph_capture_replays_on_new_bytes():
    row = 1
    first = torch.from_numpy(refs.table_frames(row))
    second = torch.from_numpy(refs.table_frames(row, 2)[1:])
    frames = first.to(DEV)
    out = {k: torch.empty_like(v) for k, v in row_call(row, frames).items()}

    def step():
        return row_call(row, frames, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                     # warm-up
    torch.cuda.current_stream().wait_stream(side)
    want_first = {k: v.clone() for k, v in step().items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                     # one linear chain
        step()
    for v in out.values():
        v.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    for k, v in want_first.items():
        assert torch.equal(out[k], v), k
    frames.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.clone() for k, v in out.items()}
    assert not torch.equal(got['canvas'], want_first['canvas'])
    eager = row_call(row, second.to(DEV))
    for k, v in eager.items():
        assert torch.equal(got[k], v), k


# ------------------------------------------------------------------ the four-pixel kernel
def test_aligned_windows_take_both_kernels_to_the_same_bytes():
    """Windows whose groups of four pixels start on a dword run the four-pixel kernel; the
    same frames at an odd address run the one-pixel kernel.  Both equal the mirror."""
    cases = [((45, 80), (72, 39), [(4, 3, 68, 35), (8, 0, 72, 32)], [True, False]),
             ((24, 32), (32, 24), [(4, 3, 28, 19), (8, 8, 32, 24)], [False, True])]
    for (h, w), resize_dims, crops, flips in cases:
        frames = torch.from_numpy(np.stack([refs.make_frame(70 + n, h, w) for n in range(2)])[None])
        want = ii.prepare_images_torch(frames, resize_dims, crops, flips, norm='clipsan',
                                       return_canvas=True)
        flat = torch.empty(frames.numel() + 1, dtype=torch.uint8, device=DEV)
        odd = flat[1:].view(frames.shape)
        odd.copy_(frames)
        assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
        for src in (frames.to(DEV), odd):
            got = ii.prepare_images(src, resize_dims, crops, flips, norm='clipsan',
                                    return_canvas=True)
            for k, v in want.items():
                assert torch.equal(got[k].cpu(), v), (k, src.data_ptr() % 4)
