"""The text side of the open-vocabulary path: CLIP's text tower, its byte-level BPE
tokenizer and the classifier built from them.

In the reference this is third-party ``open_clip`` (the text transformer and
``open_clip.tokenizer``) behind two thin wrappers, ``PredefinedOvClassifier`` and
``LearnableBgOvClassifier`` (mmdet3d/models/semantic_net/clip_utils/classifier.py:11-118),
whose ``encode_text`` (:47-60) is restated here on this package's
``ResidualAttentionBlock``:

    ClipTextEncoder   token + positional embedding, the blocks under the causal mask,
                      ``ln_final``, the row at the EOT token, ``text_projection`` -- with
                      open_clip's parameter names, so the non-``visual.`` part of an
                      OpenAI / open_clip CLIP state dict loads with ``strict=True``
    SimpleTokenizer   CLIP's BPE from a merges file in the published
                      ``bpe_simple_vocab_16e6`` format (the file is the user's)
    OvClassifier      templates -> embeddings -> classifier rows and retrieval rows

The fp32 torch form is the definition (and the CPU path).  On a ROCm device under
``no_grad`` the blocks run as ``veon_vit_block`` with the causal mask as a broadcast
(L, L) additive bias (``clip_blocks.run_blocks``): no new attention kernel.

Trimmed sequence (exact).  Under a causal mask row i depends on rows <= i only, so the
pooled EOT row never sees the padding behind it: the tower runs on ``L = max(eot) + 1``
positions instead of 77 ("a photo of a traffic cone" is 8).  Tokens that arrive as a CPU
tensor give L on the host, without any synchronisation; tokens already on the device cost
ONE read-back of ``max(eot)``.  ``trim=False`` keeps all positions.
"""
import gzip
import html
import re

import torch
import torch.nn as nn
import torch.nn.functional as F

from .clip_blocks import ResidualAttentionBlock, hip_blocks_ok, run_blocks

# (width, heads, layers, embed_dim) of the two towers the reference's configs use; both
# have head dimension 64
PRESETS = {'ViT-B/16': dict(width=512, heads=8, layers=12, embed_dim=512),
           'ViT-L/14-336': dict(width=768, heads=12, layers=12, embed_dim=768)}

CHUNK = 1024   # prompts per pass of the tower: any vocabulary x template count fits


class _Transformer(nn.Module):
    """Holder of ``resblocks`` (open_clip's ``transformer.resblocks.{i}.*`` names)."""

    def __init__(self, width, heads, layers, quick_gelu):
        super().__init__()
        self.resblocks = nn.ModuleList(
            [ResidualAttentionBlock(width, heads, 4.0, quick_gelu) for _ in range(layers)])


class ClipTextEncoder(nn.Module):
    def __init__(self, embed_dim, context_length=77, vocab_size=49408, width=512, heads=8,
                 layers=12, quick_gelu=True):
        super().__init__()
        self.context_length, self.vocab_size, self.width = context_length, vocab_size, width
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
        self.transformer = _Transformer(width, heads, layers, quick_gelu)
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * 2.6592600369383606)   # ln(1 / 0.07)
        mask = torch.full((context_length, context_length), float('-inf')).triu_(1)
        self.register_buffer('attn_mask', mask, persistent=False)
        # open_clip's initialisation (CLIP.init_parameters)
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        nn.init.normal_(self.text_projection, std=width ** -0.5)
        self._hip_cache = {}
        self._mask_cache = {}

    # The packed weights and the trimmed masks are dropped whenever the parameters may have
    # changed or moved: the three nn.Module events, forwarded by hand.  Rebound, not
    # cleared: ``run_blocks`` holds the dict object it was handed.
    def invalidate_hip_cache(self):
        self._hip_cache, self._mask_cache = {}, {}

    def train(self, mode=True):
        self.invalidate_hip_cache()
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_hip_cache()
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):   # .to() / .cuda() / .half()
        self.invalidate_hip_cache()
        return super()._apply(fn, *args, **kwargs)

    @classmethod
    def from_preset(cls, name, **kw):
        return cls(**dict(PRESETS[name], **kw))

    @staticmethod
    def text_state_dict(state_dict):
        """The entries of a whole CLIP state dict this module takes: everything outside
        ``visual.``, without the three shape scalars an OpenAI archive carries."""
        drop = ('input_resolution', 'context_length', 'vocab_size')
        return {k: v for k, v in state_dict.items()
                if not k.startswith('visual.') and k not in drop}

    def _native(self, x):
        blocks = list(self.transformer.resblocks)
        return (x.dtype == torch.float32 and not self.training
                and hip_blocks_ok(blocks, x, self.width))

    def _tower(self, tokens, eot, L, native):
        """tokens (n, >= L) and eot (n,) on the parameters' device -> (n, embed_dim)."""
        x = self.token_embedding(tokens[:, :L]) + self.positional_embedding[:L]
        blocks = list(self.transformer.resblocks)
        if native is None:
            native = self._native(x)
        elif native and not self._native(x):
            raise RuntimeError('the native text tower needs a ROCm device, eval mode, fp32 '
                               'parameters and head dimension 64')
        if native:
            mask = self._mask_cache.get(L)
            if mask is None:
                mask = self._mask_cache[L] = self.attn_mask[:L, :L].float().contiguous()
            x = x.contiguous()
            out = run_blocks(blocks, x.permute(1, 0, 2), [mask] * len(blocks),
                             self._hip_cache, keep=set(), stream=x)[-1]
            x = out.permute(1, 0, 2)
        else:
            mask = self.attn_mask[:L, :L]
            x = x.permute(1, 0, 2)
            for blk in blocks:
                x = blk(x, attn_mask=mask)
            x = x.permute(1, 0, 2)
        x = x[torch.arange(x.shape[0], device=x.device), eot]
        return self.ln_final(x) @ self.text_projection

    @torch.no_grad()
    def encode_text(self, tokens, normalize=False, trim=True, native=None):
        """tokens (n, context_length) integer ids -> (n, embed_dim) fp32 on the
        parameters' device; the arithmetic of classifier.py:47-60 (``ln_final`` is
        per row, so it is applied to the pooled rows only: the same values).
        ``native``: None = the MFMA blocks wherever they apply (a ROCm device, eval mode,
        head dimension 64), False = the torch form also there, True = raise where they do
        not apply."""
        dev = self.positional_embedding.device
        n = tokens.shape[0]
        eot = tokens.argmax(dim=-1)
        if not trim:
            L = tokens.shape[1]
        elif n == 0:
            L = 1
        else:
            L = int(eot.max()) + 1    # the one read-back when the tokens live on the device
        # (a pageable host tensor is staged by the copy itself: nothing to wait for)
        tokens, eot = tokens.to(dev, non_blocking=True), eot.to(dev, non_blocking=True)
        parts = [self._tower(tokens[i:i + CHUNK], eot[i:i + CHUNK], L, native)
                 for i in range(0, n, CHUNK)]
        x = torch.cat(parts) if parts else tokens.new_zeros((0, self.text_projection.shape[1]),
                                                            dtype=torch.float32)
        return F.normalize(x, dim=-1) if normalize else x


# ------------------------------------------------------------------------- tokenizer
def _bytes_to_unicode():
    """The published byte -> printable character table of GPT-2 / CLIP's BPE."""
    bs = list(range(ord('!'), ord('~') + 1)) + list(range(0xa1, 0xac + 1)) \
        + list(range(0xae, 0xff + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def _token_pattern():
    alt = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|"
    try:
        import regex
        return regex.compile(alt + r"[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+", regex.IGNORECASE)
    except ImportError:     # the same classes as far as ``re`` can name them
        return re.compile(alt + r"[^\W\d_]+|\d|(?:[^\s\w]|_)+", re.IGNORECASE)


class SimpleTokenizer:
    """CLIP's byte-level BPE.  ``bpe_path``: a merges file in the published
    ``bpe_simple_vocab_16e6`` format (``.txt`` or ``.txt.gz``: a header line, then one
    merge "left right" per line; at most the first 48894 merges are used, as by CLIP).
    The vocabulary is the 256 byte characters, the same with ``</w>``, the merges, and the
    two specials; SOT = size - 2 and EOT = size - 1 (49406 / 49407 with the published
    file).

    Cleaning: ``html.unescape`` twice, whitespace collapsed, lower case.  CLIP also runs
    ``ftfy.fix_text`` first; that is applied only when ``ftfy`` can be imported (it is not
    a dependency of this package, and prompts of plain ASCII are unchanged by it).  The
    token pattern uses the ``regex`` module when it can be imported, else the nearest
    ``re`` classes."""

    MAX_MERGES = 49152 - 256 - 2

    def __init__(self, bpe_path, context_length=77):
        opener = gzip.open if str(bpe_path).endswith('.gz') else open
        with opener(bpe_path, 'rb') as f:
            lines = f.read().decode('utf-8').split('\n')
        merges = [tuple(m.split()) for m in lines[1:1 + self.MAX_MERGES]]
        merges = [m for m in merges if len(m) == 2]
        self.byte_encoder = _bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + '</w>' for v in vocab] + [''.join(m) for m in merges]
        vocab += ['<|startoftext|>', '<|endoftext|>']
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {'<|startoftext|>': '<|startoftext|>', '<|endoftext|>': '<|endoftext|>'}
        self.pat = _token_pattern()
        self.vocab_size = len(vocab)
        self.sot, self.eot = self.vocab_size - 2, self.vocab_size - 1
        self.context_length = context_length

    @staticmethod
    def clean(text):
        try:
            import ftfy
            text = ftfy.fix_text(text)
        except ImportError:
            pass
        text = html.unescape(html.unescape(text))
        return re.sub(r'\s+', ' ', text.strip()).strip().lower()

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + '</w>',)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.bpe_ranks.get(p, float('inf')))
            if best not in self.bpe_ranks:
                break
            first, second = best
            new, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == first and word[i + 1] == second:
                    new.append(first + second)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        out = self.cache[token] = ' '.join(word)
        return out

    def encode(self, text):
        ids = []
        for token in self.pat.findall(self.clean(text)):
            token = ''.join(self.byte_encoder[b] for b in token.encode('utf-8'))
            ids.extend(self.encoder[t] for t in self.bpe(token).split(' '))
        return ids

    def decode(self, ids):
        inv = {v: k for k, v in self.byte_encoder.items()}
        text = ''.join(self.decoder[int(i)] for i in ids)
        return bytearray(inv[c] for c in text).decode('utf-8', errors='replace') \
            .replace('</w>', ' ')

    def __call__(self, texts, context_length=None):
        """-> (n, context_length) int64 on the CPU: SOT, the text's ids, EOT, zeros; a text
        that does not fit is cut and keeps EOT in the last slot."""
        if isinstance(texts, str):
            texts = [texts]
        ctx = context_length or self.context_length
        out = torch.zeros((len(texts), ctx), dtype=torch.long)
        for i, text in enumerate(texts):
            ids = [self.sot] + self.encode(text) + [self.eot]
            if len(ids) > ctx:
                ids = ids[:ctx]
                ids[-1] = self.eot
            out[i, :len(ids)] = torch.tensor(ids)
        return out

    tokenize = __call__


# ------------------------------------------------------------------------ classifier
class OvClassifier(nn.Module):
    """``PredefinedOvClassifier`` + ``LearnableBgOvClassifier`` (classifier.py:11-118):
    per template tokenise -> encode -> normalise, mean over the templates, renormalise; a
    per-word cache; the learnable background row ``bg_embed``.  Always in eval mode, every
    parameter frozen."""

    def __init__(self, text_encoder, tokenizer, templates=('a photo of {}',),
                 cache_feature=True):
        super().__init__()
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.templates = list(templates)
        # (the reference sizes it by text_projection.shape[0], the tower's width, which
        # equals the embedding size in both of its towers; the rows it joins have the
        # embedding size)
        dim = text_encoder.text_projection.shape[1]
        self.bg_embed = nn.Parameter(torch.randn(1, dim) * dim ** -0.5)
        self.cache_feature = cache_feature
        self.cache = {}
        for p in self.parameters():
            p.requires_grad = False
        super().train(False)

    def train(self, mode=True):
        return super().train(False)

    @property
    def logit_scale(self):
        return self.text_encoder.logit_scale

    def forward(self, category_names):
        bucket = []
        for template in self.templates:
            tokens = self.tokenizer([template.format(noun) for noun in category_names])
            bucket.append(self.text_encoder.encode_text(tokens, normalize=True))
        embed = torch.stack(bucket).mean(dim=0)
        return embed / embed.norm(dim=-1, keepdim=True)

    def clear_cache(self):
        self.cache = {}

    def get_classifier_by_vocabulary(self, vocabulary, add_bg=True):
        vocabulary = list(vocabulary)
        if self.cache_feature:
            new_words = [w for w in dict.fromkeys(vocabulary) if w not in self.cache]
            if new_words:
                self.cache.update(dict(zip(new_words, self(new_words))))
            embed = torch.stack([self.cache[w] for w in vocabulary])
        else:
            embed = self(vocabulary)
        if add_bg:
            embed = torch.cat([embed, self.bg_embed.to(embed.device)], dim=0)
        return F.normalize(embed, p=2, dim=-1)

    @torch.no_grad()
    def classifier_weight(self, vocabulary):
        """(len(vocabulary) + 1, C): ``prepare_vocabulary`` of san_in_veon_temporal.py:
        261-266 -- ``logit_scale.exp()`` times the rows, the background row last."""
        return (self.logit_scale.exp() * self.get_classifier_by_vocabulary(vocabulary)) \
            .clone().detach()

    @torch.no_grad()
    def retrieval_embedding(self, prompts):
        """(len(prompts), C): san_in_veon_temporal.py:268-273, no background row."""
        return (self.logit_scale.exp()
                * self.get_classifier_by_vocabulary(prompts, add_bg=False)).clone()
