"""CPU checks of the camera-input preparation's host module (veon_amd/image_inputs.py): the
resampling tables against an independent scalar derivation, the torch mirror against the
recorded output of the reference's ``img_transform_core`` on Pillow
(tests/golden/image_inputs_tiny.npz) and, where Pillow is installed, against a live
``Image.resize``; ``sample_augmentation`` and ``post_transform`` against the recorded
values; the normalisation tables; the argument checks; the ABI; ``PrepareImageInputs``.

The normalisations are compared with the numpy restatements of tests/image_inputs_refs.py,
not with recordings: mmcv and cv2 were absent where the fixture was made (unpinned)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import image_inputs_refs as refs
from tests.conftest import load_golden
from veon_amd import _lib, image_inputs as ii


@pytest.fixture(scope='module')
def golden():
    return load_golden('image_inputs_tiny')


def row_call(row, batch=1, **kw):
    cfg = refs.TABLE[row]
    frames = torch.from_numpy(refs.table_frames(row, batch))
    return ii.prepare_images(frames, cfg['resize_dims'], [c for c, _ in cfg['cams']],
                             [f for _, f in cfg['cams']], **kw)


# ------------------------------------------------------------------ tables
AXES = sorted(set((cfg['size'][1], cfg['resize_dims'][0]) for cfg in refs.TABLE.values()) |
              set((cfg['size'][0], cfg['resize_dims'][1]) for cfg in refs.TABLE.values()) |
              set(refs.RATIOS))


@pytest.mark.parametrize('n_in,n_out', AXES)
def test_resize_coeffs_equal_independent_tables(n_in, n_out):
    bounds, kk = ii.resize_coeffs(n_in, n_out)
    want_bounds, want_kk = refs.coeffs_ref(n_in, n_out)
    assert bounds.dtype == torch.int32 and kk.dtype == torch.int32
    assert np.array_equal(bounds.numpy(), want_bounds)
    assert np.array_equal(kk.numpy(), want_kk)
    assert ii.resize_coeffs(n_in, n_out)[1] is kk                    # cached
    # 32 bits suffice, as the issue states: 255 * sum |k| stays below 2^31 - 2^21
    assert 255 * int(np.abs(want_kk.astype(np.int64)).sum(1).max()) < 2 ** 31 - 2 ** 21


def test_tap_counts():
    assert ii.resize_coeffs(128, 16)[1].shape[1] == 33               # 8:1, the run-time count
    assert ii.resize_coeffs(1600, 1408)[1].shape[1] == 7
    assert ii.resize_coeffs(40, 53)[1].shape[1] == 5


# ------------------------------------------------------------------ the reference's images
@pytest.mark.parametrize('row', sorted(refs.TABLE))
def test_mirror_equals_recorded_images(golden, row):
    batch = 2 if row == refs.BATCH2_ROW else 1
    cfg = refs.TABLE[row]
    dw, dh = refs.depth_dims(cfg['cams'][0][0])
    res = row_call(row, batch, depth_size=(dh, dw), depth_norm='midas', return_canvas=True)
    for b in range(batch):
        for n in range(2):
            key = 'r%d_b%d_c%d' % (row, b, n)
            assert np.array_equal(res['canvas'][b, n].numpy(), golden[key + '_img'])
            assert np.array_equal(res['depth_canvas'][b, n].numpy(), golden[key + '_depth'])


def test_mirror_equals_recorded_strip(golden):
    s = refs.STRIP
    frame = torch.from_numpy(refs.make_frame(s['seed'], *s['size']))
    img = ii.transform_core_torch(frame, s['resize_dims'], s['crop'], s['flip'])
    assert tuple(img.shape) == (512, 1408, 3)
    assert np.array_equal(img[s['rows']][:, s['cols']].numpy(), golden['strip_img'])
    depth = ii.pil_resize_torch(img, refs.depth_dims(s['crop']))
    rows, cols = [r // 2 for r in s['rows'][::2]], [c // 2 for c in s['cols'][::2]]
    assert np.array_equal(depth[rows][:, cols].numpy(), golden['strip_depth'])


def test_restatement_equals_recorded_images(golden):
    """The refs' own numpy restatement (the GPU tests' second yardstick) is Pillow's too."""
    for row, cfg in refs.TABLE.items():
        frames = refs.table_frames(row)[0]
        for n, (crop, flip) in enumerate(cfg['cams']):
            got = refs.transform_ref(frames[n], cfg['resize_dims'], crop, flip)
            assert np.array_equal(got, golden['r%d_b0_c%d_img' % (row, n)])


def test_mirror_equals_live_pillow():
    Image = pytest.importorskip('PIL.Image')
    for row, cfg in refs.TABLE.items():
        frame = refs.table_frames(row)[0, 0]
        want = np.array(Image.fromarray(frame).resize(cfg['resize_dims']))
        got = ii.pil_resize_torch(torch.from_numpy(frame), cfg['resize_dims'])
        assert np.array_equal(got.numpy(), want), row


def test_both_clamps_occur(golden):
    hit = [k for k in golden if k.endswith('_img') and (golden[k] == 0).any()
           and (golden[k] == 255).any()]
    assert len(hit) >= 12


# ------------------------------------------------------------------ augmentation
def aug_row(aug):
    resize, resize_dims, crop, flip, rotate = aug
    return [resize, *resize_dims, *crop, float(flip), rotate]


@pytest.mark.parametrize('name,config', [('veon', refs.VEON_DATA_CONFIG),
                                         ('aug', refs.AUG_DATA_CONFIG)])
def test_sample_augmentation_equals_reference(golden, name, config):
    test = ii.sample_augmentation(config, 900, 1600, is_train=False)
    assert np.array_equal(np.array([aug_row(test)], np.float64), golden['aug_%s_test' % name])
    rng = np.random.RandomState(refs.AUG_SEED)       # the stream of np.random.seed(AUG_SEED)
    train = [aug_row(ii.sample_augmentation(config, 900, 1600, is_train=True, rng=rng))
             for _ in range(refs.AUG_DRAWS)]
    assert np.array_equal(np.array(train, np.float64), golden['aug_%s_train' % name])
    if name == 'veon':
        assert test[1:] == ((1408, 792), (0, 280, 1408, 792), False, 0)
        assert all(t[1:8] == [1408, 792, 0, 280, 1408, 792, 0.0] for t in train)


def test_sample_augmentation_module_rng(golden):
    np.random.seed(refs.AUG_SEED)
    step = ii.PrepareImageInputs(refs.AUG_DATA_CONFIG, is_train=True)
    train = [aug_row(step.sample_augmentation(900, 1600)) for _ in range(refs.AUG_DRAWS)]
    assert np.array_equal(np.array(train, np.float64), golden['aug_aug_train'])


@pytest.mark.parametrize('row', sorted(refs.TABLE))
def test_post_transform_equals_reference(golden, row):
    cfg = refs.TABLE[row]
    for n, (crop, flip) in enumerate(cfg['cams']):
        rot, tran = ii.post_transform(cfg['resize_dims'][0] / cfg['size'][1], crop, flip, 0)
        assert rot.dtype == torch.float32 and tuple(rot.shape) == (3, 3)
        assert tuple(tran.shape) == (3,)
        assert np.array_equal(rot[:2, :2].numpy(), golden['r%d_c%d_post_rot' % (row, n)])
        assert np.array_equal(tran[:2].numpy(), golden['r%d_c%d_post_tran' % (row, n)])
        assert torch.equal(rot[2], torch.tensor([0., 0., 1.])) and float(tran[2]) == 0.0
        assert torch.equal(rot[:2, 2], torch.zeros(2))


# ------------------------------------------------------------------ normalisation
@pytest.mark.parametrize('norm', ['mmlab', 'clipsan', ([1.5, 2.25, 100.0], [3.0, 7.0, 0.1])])
def test_norm_lut_equals_restatement(norm):
    ramp = np.arange(256, dtype=np.uint8)
    img = np.stack([ramp, ramp[::-1], np.roll(ramp, 37)], -1)[None]        # (1, 256, 3)
    got = ii.apply_lut_torch(torch.from_numpy(img), ii.norm_lut(norm))
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), refs.normalize_ref(img, norm))


def test_midas_lut_equals_restatement():
    ramp = np.arange(256, dtype=np.uint8)
    img = np.stack([ramp, ramp[::-1], np.roll(ramp, 37)], -1)[None]
    got = ii.apply_lut_torch(torch.from_numpy(img), ii.norm_lut('midas'))
    assert np.array_equal(got.numpy(), refs.midas_ref(img))
    assert float(got.min()) == -1.0 and float(got.max()) == 1.0


@pytest.mark.parametrize('row', [1, 5])
def test_prepare_images_outputs(row):
    cfg = refs.TABLE[row]
    dw, dh = refs.depth_dims(cfg['cams'][0][0])
    res = row_call(row, norm='clipsan', depth_size=(dh, dw), depth_norm='midas',
                   return_canvas=True)
    frames = refs.table_frames(row)[0]
    for n, (crop, flip) in enumerate(cfg['cams']):
        canvas = refs.transform_ref(frames[n], cfg['resize_dims'], crop, flip)
        assert np.array_equal(res['imgs'][0, n].numpy(), refs.normalize_ref(canvas, 'clipsan'))
        depth = refs.pil_resize_ref(canvas, (dw, dh))
        assert np.array_equal(res['depth_img_inputs'][0, n].numpy(), refs.midas_ref(depth))
    assert 'canvas' not in row_call(row)


def test_depthanything_size_and_tail():
    assert ii.depthanything_size(256, 704) == (252, 700)
    assert ii.depthanything_size(518, 518, target=518) == (518, 518)
    img = refs.make_bright_frame(5, 16, 44)
    oh, ow = 14, 42
    want, bound = refs.cubic_norm_ref(img, oh, ow)
    got = ii.cubic_norm_torch(torch.from_numpy(img), (oh, ow))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, oh, ow)
    assert bool((np.abs(got.numpy().astype(np.float64) - want) <= bound).all())
    exact = ii.cubic_norm_torch(torch.from_numpy(img), (oh, ow), dtype=torch.float64)
    assert np.abs(exact.numpy() - want).max() < 1e-6      # fp32 mean / std against fp64 ones


# ------------------------------------------------------------------ argument checks
def test_value_errors():
    frames = torch.zeros(1, 2, 24, 32, 3, dtype=torch.uint8)
    ok = dict(resize_dims=(32, 24), crop=(5, 3, 29, 19))
    ii.prepare_images(frames, **ok)
    with pytest.raises(ValueError, match='rotate'):
        ii.prepare_images(frames, rotate=5.0, **ok)
    for crop in [(-1, 3, 23, 19), (5, 3, 33, 19), (5, 9, 29, 25), (5, -2, 29, 14)]:
        with pytest.raises(ValueError, match='leaves the resized image'):
            ii.prepare_images(frames, (32, 24), crop)
    with pytest.raises(ValueError, match='uint8'):
        ii.prepare_images(frames.float(), **ok)
    with pytest.raises(ValueError, match='contiguous'):
        ii.prepare_images(frames.transpose(2, 3), **ok)
    with pytest.raises(ValueError, match='one per camera'):
        ii.prepare_images(frames, (32, 24), [(5, 3, 29, 19)] * 3)
    many = torch.zeros(1, 33, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='at most 32 cameras'):
        ii.prepare_images(many, (4, 4), [(0, 0, 2, 2)] * 33)
    ii.prepare_images(many, (4, 4), (0, 0, 2, 2))                      # one window: no limit
    with pytest.raises(ValueError, match='one size'):
        ii.prepare_images(frames, (32, 24), [(5, 3, 29, 19), (0, 0, 8, 8)])
    with pytest.raises(ValueError, match='unknown normalisation'):
        ii.prepare_images(frames, norm='other', **ok)


# ------------------------------------------------------------------ ABI
def test_abi_declares_the_entry_points():
    i, p, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    want = {
        'veon_image_resample_h': [p, i, i, i, i, i, i, p, p, i, p, p],
        'veon_image_resample_v_finish': [p, i, i, i, i, i, p, p, i, _lib.ImageWindows, i, i, p,
                                         i, p, p, p],
        'veon_image_cubic_norm': [p, i, i, i, i, i, i, f, f, f, f, f, f, p, p],
    }
    for name, argtypes in want.items():
        assert name in _lib.declared_symbols()
        restype, got = _lib._SIGNATURES[name]
        assert restype is ctypes.c_int and got == argtypes
    assert ctypes.sizeof(_lib.ImageWindows) == 4 * (1 + 3 * 32)
    with open(_lib.os.path.join(_lib.INCLUDE, 'veon_hip.h')) as fh:
        text = fh.read()
    assert '#define VEON_ABI_VERSION 2' in text
    assert '#define VEON_IMAGE_MAX_WINDOWS %d' % _lib.IMAGE_MAX_WINDOWS in text


# ------------------------------------------------------------------ the pipeline step
CAMS = ['CAM_A', 'CAM_B', 'CAM_C']
SMALL_CONFIG = {'cams': CAMS, 'Ncams': 3, 'input_size': (32, 64), 'depth_input_size': (16, 32),
                'resize': (0.0, 0.11), 'rot': (0.0, 0.0), 'flip': True, 'crop_h': (0.0, 0.0),
                'resize_test': 0.0}


def synthetic_info(seed, token):
    rng = np.random.RandomState(seed)
    cams = {}
    for k, name in enumerate(CAMS):
        q = rng.randn(4)
        cams[name] = dict(frame=refs.make_frame(seed * 10 + k, 45, 80),
                          cam_intrinsic=(np.eye(3) * (k + 2)).tolist(),
                          sensor2ego_rotation=(q / np.linalg.norm(q)).tolist(),
                          sensor2ego_translation=rng.randn(3).tolist(),
                          ego2global_rotation=[1.0, 0.0, 0.0, 0.0],
                          ego2global_translation=[float(seed), 2.0, 3.0])
    return dict(token=token, cams=cams)


@pytest.mark.parametrize('is_train', [False, True])
def test_pipeline_step_sequential(is_train):
    results = dict(curr=synthetic_info(1, 'tok0'), adjacent=[synthetic_info(2, 'tok1')])
    step = ii.PrepareImageInputs(SMALL_CONFIG, is_train=is_train, sequential=True,
                                 img_norm_method='clipsan', use_depth_input=True,
                                 depth_img_norm_method='midas')
    np.random.seed(7)
    out = step(results)
    imgs, sensor2egos, ego2globals, intrins, post_rots, post_trans = out['img_inputs']
    assert tuple(imgs.shape) == (6, 3, 32, 64) and imgs.dtype == torch.float32
    assert tuple(sensor2egos.shape) == (6, 4, 4) and tuple(ego2globals.shape) == (6, 4, 4)
    assert tuple(intrins.shape) == (6, 3, 3)
    assert tuple(post_rots.shape) == (6, 3, 3) and tuple(post_trans.shape) == (6, 3)
    assert tuple(out['depth_img_inputs'].shape) == (6, 3, 16, 32)
    # the matrices: current cameras, then the adjacent frame's, with the current augmentation
    assert torch.equal(post_rots[3:], post_rots[:3]) and torch.equal(post_trans[3:], post_trans[:3])
    assert torch.equal(intrins[3:], intrins[:3])
    assert [float(m[0, 3]) for m in ego2globals] == [1.0] * 3 + [2.0] * 3
    assert list(out['cam_names']) == CAMS
    # the images: camera-major, the current frame then the adjacent one
    assert out['unique_tokens'] == ['%s-%s' % (t, c) for c in CAMS for t in ('tok0', 'tok1')]
    assert len(out['canvas']) == 6 and out['canvas'][0].shape == (32, 64, 3)
    # every image is the reference sequence on its own frame with the camera's augmentation
    np.random.seed(7)
    for k, name in enumerate(CAMS):
        resize, resize_dims, crop, flip, rotate = ii.sample_augmentation(
            SMALL_CONFIG, 45, 80, is_train)
        rot, tran = ii.post_transform(resize, crop, flip, rotate)
        assert torch.equal(post_rots[k], rot) and torch.equal(post_trans[k], tran)
        for j, info in enumerate([results['curr'], results['adjacent'][0]]):
            canvas = refs.transform_ref(info['cams'][name]['frame'], resize_dims, crop, flip)
            assert np.array_equal(out['canvas'][2 * k + j], canvas)
            assert np.array_equal(imgs[2 * k + j].numpy(), refs.normalize_ref(canvas, 'clipsan'))
            depth = refs.pil_resize_ref(canvas, (32, 16))
            assert np.array_equal(out['depth_img_inputs'][2 * k + j].numpy(),
                                  refs.midas_ref(depth))
    rot = sensor2egos[0][:3, :3].double()
    assert torch.allclose(rot @ rot.T, torch.eye(3, dtype=torch.float64), atol=1e-6)
    assert abs(float(torch.det(rot)) - 1.0) < 1e-6


def test_pipeline_step_single_frame_and_errors():
    results = dict(curr=synthetic_info(3, 'tok'))
    imgs, *_, post_rots, post_trans = ii.PrepareImageInputs(SMALL_CONFIG).get_inputs(results)
    assert tuple(imgs.shape) == (3, 3, 32, 64) and tuple(post_rots.shape) == (3, 3, 3)
    assert 'depth_img_inputs' not in results
    with pytest.raises(ValueError):
        ii.PrepareImageInputs(SMALL_CONFIG, img_norm_method='midas2')
    bad = dict(curr=synthetic_info(3, 'tok'))
    bad['curr']['cams']['CAM_A']['frame'] = np.zeros((45, 80, 3), np.float32)
    with pytest.raises(ValueError, match='uint8'):
        ii.PrepareImageInputs(SMALL_CONFIG).get_inputs(bad)


def test_quaternion_rotation_matrix():
    assert np.array_equal(ii.quaternion_rotation_matrix(1, 0, 0, 0), np.eye(3))
    c = np.sqrt(0.5)
    want = np.array([[0., -1., 0.], [1., 0., 0.], [0., 0., 1.]])          # 90 degrees about z
    assert np.allclose(ii.quaternion_rotation_matrix(c, 0, 0, c), want, atol=1e-15)
    assert np.allclose(ii.quaternion_rotation_matrix(2 * c, 0, 0, 2 * c), want, atol=1e-15)
