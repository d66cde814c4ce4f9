"""The text tower's torch form (the CPU path and the yardstick of the native one):
against a float64 restatement from ``nn.MultiheadAttention``, against
``transformers.CLIPTextModelWithProjection`` with the same weights, trimmed against
untrimmed, and open_clip's state-dict names."""
import pytest
import torch

from tests import clip_text_refs as refs
from veon_amd.models.semantic_net.clip_text import PRESETS, ClipTextEncoder, OvClassifier

TINY = dict(embed_dim=32, ctx=12, vocab=64, width=64, heads=1, layers=2)
EOTS = (11, 1, 5, 2)      # a prompt that fills every position, the empty prompt, two others


def _tiny():
    return refs.tower(**TINY), refs.tokens_with_eot(EOTS, TINY['ctx'], TINY['vocab'])


def test_mirror_equals_the_float64_restatement():
    enc, tokens = _tiny()
    want = refs.encode_text_fp64(enc, tokens)
    for trim in (True, False):
        got = enc.encode_text(tokens, trim=trim)
        assert got.dtype == torch.float32 and got.shape == (len(EOTS), TINY['embed_dim'])
        err = refs.rel_err(got, want)
        print('trim=%s: relative error %.3g' % (trim, err))
        assert err <= 1e-5
    unit = enc.encode_text(tokens, normalize=True)
    assert refs.rel_err(unit, torch.nn.functional.normalize(want, dim=-1)) <= 1e-5


def test_trimmed_equals_untrimmed():
    enc, tokens = _tiny()
    full = enc.encode_text(tokens, trim=False)
    assert refs.rel_err(enc.encode_text(tokens), full) <= 1e-5
    for i, e in enumerate(EOTS):      # each prompt alone: L = its own EOT position + 1
        assert refs.rel_err(enc.encode_text(tokens[i:i + 1]), full[i:i + 1]) <= 1e-5
    assert enc.encode_text(tokens[:0]).shape == (0, TINY['embed_dim'])


def test_equals_transformers_clip_text_model():
    tf = pytest.importorskip('transformers')
    enc, tokens = _tiny()
    cfg = tf.CLIPTextConfig(
        vocab_size=TINY['vocab'], hidden_size=TINY['width'],
        intermediate_size=4 * TINY['width'], projection_dim=TINY['embed_dim'],
        num_hidden_layers=TINY['layers'], num_attention_heads=TINY['heads'],
        max_position_embeddings=TINY['ctx'], hidden_act='quick_gelu',
        # eos_token_id == 2 selects the pooled row by argmax of the ids, as CLIP does
        pad_token_id=1, bos_token_id=0, eos_token_id=2)
    model = tf.CLIPTextModelWithProjection(cfg).eval()
    sd = enc.state_dict()
    D = TINY['width']
    new = {'text_model.embeddings.token_embedding.weight': sd['token_embedding.weight'],
           'text_model.embeddings.position_embedding.weight': sd['positional_embedding'],
           'text_model.final_layer_norm.weight': sd['ln_final.weight'],
           'text_model.final_layer_norm.bias': sd['ln_final.bias'],
           'text_projection.weight': sd['text_projection'].t()}
    for i in range(TINY['layers']):
        src, dst = 'transformer.resblocks.%d.' % i, 'text_model.encoder.layers.%d.' % i
        for j, name in enumerate(('q_proj', 'k_proj', 'v_proj')):
            new[dst + 'self_attn.%s.weight' % name] = sd[src + 'attn.in_proj_weight'][j * D:(j + 1) * D]
            new[dst + 'self_attn.%s.bias' % name] = sd[src + 'attn.in_proj_bias'][j * D:(j + 1) * D]
        for a, b in (('attn.out_proj', 'self_attn.out_proj'), ('ln_1', 'layer_norm1'),
                     ('ln_2', 'layer_norm2'), ('mlp.c_fc', 'mlp.fc1'), ('mlp.c_proj', 'mlp.fc2')):
            for w in ('weight', 'bias'):
                new[dst + b + '.' + w] = sd[src + a + '.' + w]
    missing, unexpected = model.load_state_dict({k: v.clone() for k, v in new.items()},
                                                strict=False)
    assert not unexpected and all('position_ids' in k for k in missing), (missing, unexpected)
    with torch.no_grad():
        want = model(input_ids=tokens, attention_mask=torch.ones_like(tokens)).text_embeds
    err = refs.rel_err(enc.encode_text(tokens, trim=False), want)
    print('relative error against transformers: %.3g' % err)
    assert err <= 1e-5


def test_open_clip_state_dict_loads_strictly():
    enc = ClipTextEncoder(32, 12, 64, 64, 1, 2)
    names = ['positional_embedding', 'text_projection', 'logit_scale',
             'token_embedding.weight', 'ln_final.weight', 'ln_final.bias']
    for i in range(2):
        names += ['transformer.resblocks.%d.%s' % (i, s) for s in (
            'ln_1.weight', 'ln_1.bias', 'attn.in_proj_weight', 'attn.in_proj_bias',
            'attn.out_proj.weight', 'attn.out_proj.bias', 'ln_2.weight', 'ln_2.bias',
            'mlp.c_fc.weight', 'mlp.c_fc.bias', 'mlp.c_proj.weight', 'mlp.c_proj.bias')]
    assert sorted(enc.state_dict()) == sorted(names)
    # a whole CLIP archive: the visual tower and OpenAI's three shape scalars beside it
    whole = {k: torch.randn_like(v) for k, v in enc.state_dict().items()}
    whole.update({'visual.conv1.weight': torch.zeros(1), 'visual.proj': torch.zeros(1),
                  'input_resolution': torch.tensor(224), 'context_length': torch.tensor(12),
                  'vocab_size': torch.tensor(64)})
    enc.load_state_dict(ClipTextEncoder.text_state_dict(whole), strict=True)
    assert torch.equal(enc.text_projection, whole['text_projection'])
    assert tuple(enc.attn_mask.shape) == (12, 12) and 'attn_mask' not in enc.state_dict()
    assert bool(torch.isinf(enc.attn_mask[0, 1])) and float(enc.attn_mask[1, 0]) == 0.0
    for name, (width, heads, embed) in {'ViT-B/16': (512, 8, 512),
                                        'ViT-L/14-336': (768, 12, 768)}.items():
        p = PRESETS[name]
        assert (p['width'], p['heads'], p['embed_dim'], p['layers']) == (width, heads, embed, 12)
        assert p['width'] // p['heads'] == 64


class _WordTokenizer:
    """word -> id by a fixed table (the classifier's arithmetic needs no BPE)."""
    WORDS = 'a photo of the car sedan bus tree there is in scene'.split()

    def __call__(self, texts):
        out = torch.zeros((len(texts), 12), dtype=torch.long)
        for i, t in enumerate(texts):
            ids = [62] + [1 + self.WORDS.index(w) for w in t.split()] + [63]
            out[i, :len(ids)] = torch.tensor(ids)
        return out


def test_classifier_follows_the_reference_arithmetic():
    enc = refs.tower(**TINY)
    templates = ('a photo of a {}', 'there is the {} in the scene')
    clf = OvClassifier(enc, _WordTokenizer(), templates)
    assert not clf.training and not clf.train().training
    assert not any(p.requires_grad for p in clf.parameters())
    words = ['car', 'sedan', 'bus']
    tok = _WordTokenizer()
    per = [torch.nn.functional.normalize(refs.encode_text_fp64(
        enc, tok([t.format(w) for w in words])), dim=-1) for t in templates]
    mean = torch.nn.functional.normalize(torch.stack(per).mean(0), dim=-1)
    scale = enc.logit_scale.detach().double().exp()
    rows = torch.cat([mean, clf.bg_embed.detach().double()])
    want = scale * torch.nn.functional.normalize(rows, dim=-1)
    got = clf.classifier_weight(words)
    assert got.shape == (4, TINY['embed_dim']) and refs.rel_err(got, want) <= 1e-5
    assert sorted(clf.cache) == sorted(words)
    # cached words are not encoded again; a repeated word costs one row
    again = clf.retrieval_embedding(['bus', 'tree', 'bus'])
    assert refs.rel_err(again[0:1], want[2:3]) <= 1e-5 and torch.equal(again[0], again[2])
    assert again.shape == (3, TINY['embed_dim']) and 'tree' in clf.cache


def test_native_caches_are_dropped_when_the_weights_may_have_changed():
    from veon_amd.models._native_cache import invalidate_all
    enc = ClipTextEncoder(32, 12, 64, 64, 1, 1).eval()
    events = {'train': lambda: enc.train(False), 'load': lambda: enc.load_state_dict(enc.state_dict()),
              'apply': lambda: enc.float(), 'by hand': enc.invalidate_hip_cache,
              'walk': lambda: invalidate_all(torch.nn.Sequential(enc))}
    for name, event in events.items():
        packed, masks = enc._hip_cache, enc._mask_cache
        packed['x'], masks[3] = 1, 2
        event()
        assert enc._hip_cache == {} and enc._mask_cache == {}, name
        assert enc._hip_cache is not packed and enc._mask_cache is not masks, name
