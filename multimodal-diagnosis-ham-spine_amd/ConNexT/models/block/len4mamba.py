"""MultimodalMamba, KANMultiheadAttention and MultimodalMambaWithKANAttention (reference ConNexT/models/block/len4mamba.py)
with the reference's constructor and forward signatures, defaults and state-dict keys, on the hamspine kernels.  The
reference imports `mamba_ssm.Mamba`; here the block is hamspine.nn.Mamba(d_state=128) (same parameters and keys, HIP conv1d /
selective-scan kernels).

Dtype policy.  The inputs are f32 post-tower features.  The four projections, the token sequence with its positional
encoding, the KAN attention (the KAN kernels are f32 only) and the LayerNorms run in f32.  Mamba runs in the compute dtype
(hamspine.set_compute_dtype): in bf16 mode its input is cast once, and its out_proj GEMM writes f32 with the residual added in
the epilogue.  The output is (B, P + 3, proj_dim) f32.

`positional_encoding` is a plain attribute as in the reference (not a buffer, not in the state dict); a device copy of the
rows in use is kept next to it and redone when the attribute is reassigned.  torch.cat, the broadcast add of the encoding
and `img.permute(0, 2, 1)` are hs_token_seq_assemble_* and hs_transpose_batched_f32; both residual adds ride in a GEMM
epilogue."""
import math

import torch
import torch.nn as nn

import hamspine
from hamspine import functional as F
from hamspine import ssm
from hamspine.convnext_ops import attention_core
from hamspine.nn import Mamba
from hamspine.nn.layers import LayerNorm, Linear

from .kan1 import KAN1


def _sinusoid_table(max_len, d_model):
    """(1, max_len, d_model) f32: column 2i is sin(t w_i), column 2i + 1 is cos(t w_i), w_i = 10000^(-2i / d_model), for row t
    (the table of len4mamba.py:117-123)"""
    t = torch.arange(max_len, dtype=torch.float32)[:, None]
    w = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * (-math.log(10000.0) / d_model))[None, :]
    table = torch.empty(1, max_len, d_model)
    table[0, :, 0::2] = torch.sin(t * w)
    table[0, :, 1::2] = torch.cos(t * w)
    return table


class _TokenSequence(nn.Module):
    """The part the two blocks share (len4mamba.py:86-106,147-168): four projections to proj_dim, the sequence
    [text; image tokens; first; last] and the sinusoidal positional encoding."""

    def _init_sequence(self, text_dim, img_dim, hidden_dim, proj_dim):
        self.proj_text = Linear(text_dim, proj_dim)
        self.proj_img = Linear(img_dim, proj_dim)
        self.proj_first = Linear(hidden_dim, proj_dim)
        self.proj_last = Linear(hidden_dim, proj_dim)
        self.positional_encoding = self._create_positional_encoding(max_len=2048, d_model=proj_dim)
        self._pe_dev = None         # (source tensor, device copy of its first rows)

    def _create_positional_encoding(self, max_len=1024, d_model=256):
        return _sinusoid_table(max_len, d_model)

    def _pe_on(self, device, length):
        """the first `length` rows of `positional_encoding` on `device`, f32; zeros where the attribute is None (the reference
        then adds nothing).  The device copy is redone when the attribute, the device or the length changes."""
        pe = self.positional_encoding
        if pe is not None and length > pe.shape[1]:
            raise ValueError(f"sequence length {length} exceeds the positional encoding's max_len {pe.shape[1]}")
        c = self._pe_dev
        if c is None or c[0] is not pe or c[1].device != device or c[1].shape[0] != length:
            rows = (torch.zeros(length, self.proj_text.out_features) if pe is None else pe[0, :length])
            self._pe_dev = c = (pe, rows.to(device=device, dtype=torch.float32).contiguous())
        return c[1]

    def _sequence(self, text, img, first_hidden, last_hidden):
        """text (B, Tt), img (B, C, P), first / last (B, Hd), f32 -> (B, P + 3, proj_dim) f32"""
        text, img, first_hidden, last_hidden = (t if t.dtype == torch.float32 else t.float()
                                                for t in (text, img, first_hidden, last_hidden))
        img_rows = ssm.transpose_batched(img)                               # (B, P, C)
        return ssm.token_seq_assemble(self.proj_text(text), self.proj_img(img_rows), self.proj_first(first_hidden),
                                      self.proj_last(last_hidden), self._pe_on(img.device, img.shape[2] + 3))

    def _mamba_input(self, x):
        cd = hamspine.compute_dtype()
        return x if cd == torch.float32 else F.axpby(x, None, 1.0, 0.0, out_dtype=cd)


class KANMultiheadAttention(nn.Module):
    def __init__(self, embed_dim, num_heads=8, dropout=0.0):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.dropout = dropout
        assert embed_dim % num_heads == 0, "embed_dim must be divisible by num_heads"
        self.head_dim = embed_dim // num_heads
        self.q_proj = KAN1([embed_dim, embed_dim])
        self.k_proj = KAN1([embed_dim, embed_dim])
        self.v_proj = KAN1([embed_dim, embed_dim])
        self.out_proj = Linear(embed_dim, embed_dim)

    def attend(self, x, residual=None):
        """out_proj(attention(KAN_q(x), KAN_k(x), KAN_v(x))) (+ residual in the GEMM epilogue); x (B, L, D) f32"""
        if x.dtype != torch.float32:
            x = x.float()
        q, k, v = self.q_proj(x), self.k_proj(x), self.v_proj(x)
        ctx = attention_core(q, k, v, self.num_heads, self.head_dim ** -0.5,
                             dropout_p=self.dropout if self.training else 0.0)
        return self.out_proj(ctx, residual=residual)

    def forward(self, x, mask=None):
        if mask is not None:
            raise NotImplementedError("KANMultiheadAttention: an attention mask is not implemented (no caller in the reference "
                                      "passes one, len4mamba.py:109)")
        return self.attend(x)


class MultimodalMambaWithKANAttention(_TokenSequence):
    def __init__(self, text_dim=768, img_dim=640, hidden_dim=3584, proj_dim=256, num_heads=4):
        super().__init__()
        self._init_sequence(text_dim, img_dim, hidden_dim, proj_dim)
        self.attn = KANMultiheadAttention(embed_dim=proj_dim, num_heads=num_heads)
        self.mamba = Mamba(d_model=proj_dim, d_state=128, d_conv=4, expand=2)
        self.norm1 = LayerNorm(proj_dim)
        self.norm2 = LayerNorm(proj_dim)

    def forward(self, text, img, first_hidden, last_hidden):
        seq = self._sequence(text, img, first_hidden, last_hidden)
        attn_output = self.norm1(self.attn.attend(seq, residual=seq))
        mamba_output = self.mamba(self._mamba_input(attn_output), residual=attn_output, out_dtype=torch.float32)
        return self.norm2(mamba_output)


class MultimodalMamba(_TokenSequence):
    def __init__(self, text_dim=768, img_dim=1568, hidden_dim=3584, proj_dim=256):
        super().__init__()
        self._init_sequence(text_dim, img_dim, hidden_dim, proj_dim)
        self.mamba = Mamba(d_model=proj_dim, d_state=128, d_conv=4, expand=2)

    def forward(self, text, img, first_hidden, last_hidden):
        seq = self._sequence(text, img, first_hidden, last_hidden)
        return self.mamba(self._mamba_input(seq), residual=seq, out_dtype=torch.float32)
