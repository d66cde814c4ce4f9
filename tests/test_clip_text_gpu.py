"""The native text tower (``veon_vit_block`` under the causal mask as a broadcast bias) on
the MI355X, in both half flavours.

Yardstick: the float64 restatement of tests/clip_text_refs.py.  Bound: the native error is
at most TWICE the error of the torch mirror under autocast in the same half dtype -- the
project's standing margin for half roundings taken in another order (as in
tests/test_optim_step.py); both figures are printed."""
import warnings

import pytest
import torch

from tests import clip_text_refs as refs
from tests.helpers import flavour, fp16_twin  # noqa: F401  (autouse fixture)
from veon_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN = 2.0
TOWERS = {
    'w128': (dict(embed_dim=64, ctx=77, vocab=300, width=128, heads=2, layers=2),
             (1, 2, 8, 19, 76)),
    'w512': (dict(embed_dim=64, ctx=77, vocab=300, width=512, heads=8, layers=1),
             (4, 11, 40)),
}


def _case(name):
    cfg, eots = TOWERS[name]
    enc = refs.tower(**cfg).to(DEV)
    tokens = refs.tokens_with_eot(eots, cfg['ctx'], cfg['vocab'])
    return enc, tokens, refs.encode_text_fp64(enc, tokens)


def _autocast_error(enc, tokens, want, dtype):
    with torch.autocast('cuda', dtype=dtype):
        got = enc.encode_text(tokens, trim=False, native=False)
    return refs.rel_err(got.float(), want)


@pytest.mark.parametrize('name', sorted(TOWERS))
def test_native_error_within_twice_the_autocast_mirror(name, flavour):
    enc, tokens, want = _case(name)
    before = _lib.CALLS.get('veon_vit_block', 0)
    trimmed = enc.encode_text(tokens, native=True)
    whole = enc.encode_text(tokens, trim=False, native=True)
    layers = len(enc.transformer.resblocks)
    assert _lib.CALLS.get('veon_vit_block', 0) == before + 2 * layers
    assert trimmed.dtype == torch.float32 and trimmed.shape == want.shape
    mirror = refs.rel_err(enc.encode_text(tokens, native=False), want)
    base = _autocast_error(enc, tokens, want, flavour)
    e_trim, e_whole = refs.rel_err(trimmed, want), refs.rel_err(whole, want)
    gap = refs.rel_err(trimmed, whole.double())
    print('%s %s: native trimmed %.3g, untrimmed %.3g, autocast mirror %.3g (ratios %.2f, '
          '%.2f), trimmed vs untrimmed %.3g, fp32 mirror %.3g'
          % (name, flavour, e_trim, e_whole, base, e_trim / base, e_whole / base, gap, mirror))
    assert mirror <= 1e-5 and base > 0.0
    assert e_trim <= MARGIN * base and e_whole <= MARGIN * base
    assert gap <= MARGIN * base


test_native_error_within_twice_the_autocast_mirror_fp16 = fp16_twin(
    test_native_error_within_twice_the_autocast_mirror)


def _sync_warnings(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
    found = [w for w in rec if 'called a synchroniz' in str(w.message).lower()]
    for w in found:
        print('synchronising call at %s:%d: %s' % (w.filename, w.lineno, w.message))
    return len(found), out


def test_cpu_tokens_make_no_synchronising_call():
    """Tokens on the host give the trimmed length there: the call only enqueues work.
    Tokens on the device cost the documented read-back, which also shows the mode is live."""
    enc, tokens, want = _case('w128')
    enc.encode_text(tokens)                      # packs the weights, builds the mask
    assert not tokens.is_cuda
    n_host, out = _sync_warnings(lambda: enc.encode_text(tokens, normalize=True))
    on_device = tokens.to(DEV)
    n_dev, out_dev = _sync_warnings(lambda: enc.encode_text(on_device, normalize=True))
    print('synchronisation warnings: host tokens %d, device tokens %d' % (n_host, n_dev))
    assert n_host == 0 and n_dev == 1
    assert torch.equal(out, out_dev)
    assert refs.rel_err(out, torch.nn.functional.normalize(want, dim=-1)) < 0.05
