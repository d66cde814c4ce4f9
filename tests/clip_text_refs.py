"""Shared by the text-tower tests: seeded towers, token rows with the EOT token at chosen
positions, and the float64 restatement of ``encode_text`` (clip_utils/classifier.py:47-60)
built from ``torch.nn.MultiheadAttention`` -- none of the package's own block code."""
import torch
import torch.nn as nn

from veon_amd.models.semantic_net.clip_text import ClipTextEncoder


def tower(embed_dim, ctx, vocab, width, heads, layers, seed=0):
    """A seeded ``ClipTextEncoder`` in eval mode whose LayerNorms and biases are not at
    their initial 1 / 0 (a swapped weight and bias would otherwise go unnoticed)."""
    torch.manual_seed(seed)
    enc = ClipTextEncoder(embed_dim, ctx, vocab, width, heads, layers).eval()
    with torch.no_grad():
        enc.token_embedding.weight.normal_(0, 0.5)
        enc.positional_embedding.normal_(0, 0.2)
        for name, p in enc.named_parameters():
            if name.endswith('.bias'):
                p.normal_(0, 0.1)
            elif '.ln_' in name or name.startswith('ln_final'):
                p.uniform_(0.5, 1.5)
    return enc


def tokens_with_eot(eot_positions, ctx, vocab, seed=1):
    """(n, ctx) int64: SOT = vocab - 2 first, random ids below it, EOT = vocab - 1 (the
    highest id, so ``argmax`` finds it) at the given position of each row, zeros behind."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros((len(eot_positions), ctx), dtype=torch.long)
    for i, e in enumerate(eot_positions):
        assert 1 <= e < ctx
        out[i, 0] = vocab - 2
        out[i, 1:e] = torch.randint(1, vocab - 2, (e - 1,), generator=g)
        out[i, e] = vocab - 1
    return out


def encode_text_fp64(enc, tokens):
    """classifier.py:47-60 in float64 on the CPU, all ``tokens.shape[1]`` positions."""
    sd = {k: v.detach().cpu().double() for k, v in enc.state_dict().items()}
    width = sd['positional_embedding'].shape[1]
    heads = enc.transformer.resblocks[0].n_head
    tokens = tokens.cpu()
    L = tokens.shape[1]
    mask = torch.full((L, L), float('-inf'), dtype=torch.float64).triu_(1)
    x = sd['token_embedding.weight'][tokens] + sd['positional_embedding'][:L]
    x = x.permute(1, 0, 2)
    for i in range(len(enc.transformer.resblocks)):
        p = 'transformer.resblocks.%d.' % i
        mha = nn.MultiheadAttention(width, heads).double()
        mha.load_state_dict({k[len(p + 'attn.'):]: v for k, v in sd.items()
                             if k.startswith(p + 'attn.')})
        with torch.no_grad():
            h = nn.functional.layer_norm(x, (width,), sd[p + 'ln_1.weight'],
                                         sd[p + 'ln_1.bias'], 1e-5)
            x = x + mha(h, h, h, need_weights=False, attn_mask=mask)[0]
            h = nn.functional.layer_norm(x, (width,), sd[p + 'ln_2.weight'],
                                         sd[p + 'ln_2.bias'], 1e-5)
            h = h @ sd[p + 'mlp.c_fc.weight'].t() + sd[p + 'mlp.c_fc.bias']
            h = h * torch.sigmoid(1.702 * h)
            x = x + h @ sd[p + 'mlp.c_proj.weight'].t() + sd[p + 'mlp.c_proj.bias']
    x = x.permute(1, 0, 2)
    x = nn.functional.layer_norm(x, (width,), sd['ln_final.weight'], sd['ln_final.bias'], 1e-5)
    return x[torch.arange(x.shape[0]), tokens.argmax(dim=-1)] @ sd['text_projection']


def rel_err(got, want):
    """max |got - want| / max |want|, in float64."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max())
