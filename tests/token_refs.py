"""Test infrastructure: torch restatement of what ``Cnn_9layers_Conformer``
(pytorch/models.py:2019-2189) adds to the two Conformer models of
tests/conformer_refs.py, written from the model's description.  CPU only;
nothing here imports the library.  Every function takes whatever dtype its
state dict and input carry: float32 is the reference's arithmetic, float64 the
yardstick of tests/test_gpu_token.py.

  7 -> 8    block 4's conv2 + folded BatchNorm + ReLU with all 8 frequency bins
            kept (no pool, no frequency mean), every (frame, bin) pixel a token
            in (t, f) order, behind the tag token linear_emb(ones)
  8 -> 20   the encoder's input layer on the Ts = 8 T3 + 1 tokens: token 0 gets
            pe[0], pixel token i gets pe[i + 1] (conformer_refs.input_layer on
            the token rows)
  20 -> 32  conformer_refs' encoder steps, unchanged
  9 -> 44   classifier = Linear(144, C) on every token; the outputs are its rows:
            token 0 clipwise, tokens 1.. framewise, logits

Capture ids (include/sedx.h): 7 [B, T3, 8, 512] (block 4 conv1's output), 8
[B, Ts, 512], 20 .. 32 and 9 [B, Ts, 144], 44 [B * Ts, nac].
"""
import numpy as np
import torch
import torch.nn.functional as F

import conformer_refs as CR
from oracle import sed_oracle as O
from sedx import synth

TOKEN, REG, GRU = 'Cnn_9layers_Conformer', 'Cnn_9layers_Gru_Reg', 'Cnn_9layers_Gru_FrameAtt'
SEEDS = synth.TOKEN_GOLDEN_SEEDS
KEYS = ('framewise_output', 'clipwise_output')
P16 = CR.P16
ACT_IDS = CR.ACT_IDS
STEPS = [(7, 8), (8, 20)] + [(i, i + 1) for i in range(20, 32)]
LOGITS = 44
MAX_TOKENS = CR.MAX_LEN


def geometry(T):
    """Feature frames -> (T3, tokens, framewise frames)."""
    T3 = T // 8
    return T3, 8 * T3 + 1, 8 * T3


def nac(C):
    return (C + 63) // 64 * 64


def state(dtype, classes_num=25, seed=None):
    """``synth.make_state_dict`` of the token model plus the encoder's constant buffers."""
    sd = {}
    for k, v in synth.make_state_dict(TOKEN, classes_num=classes_num,
                                      seed=SEEDS[TOKEN] if seed is None else seed).items():
        t = torch.from_numpy(np.asarray(v))
        sd[k] = t.to(dtype) if t.is_floating_point() else t
    sd['encoder.input_layer.4.pe'] = CR.pe_table(dtype)
    for b in range(CR.BLOCKS):
        sd['encoder.conformer_blocks.%d.mhsa.pos_emb.inv_freq' % b] = CR.inv_freq(dtype)
    return sd


def tag_token(sd):
    """linear_emb on a tensor of ones: [512]."""
    w = sd['linear_emb.weight']
    one = torch.ones(1, 1, dtype=w.dtype, device=w.device)
    return F.linear(one, sd['linear_emb.weight'], sd['linear_emb.bias'])[0]


def tag_token_fp32(sd32):
    """The host fold: fl(w[c][0] + b[c]), one fp32 rounding."""
    w = sd32['linear_emb.weight'].numpy().astype(np.float32)[:, 0]
    return (w + sd32['linear_emb.bias'].numpy().astype(np.float32)).astype(np.float32)


def tokens(sd, x7):
    """Capture 7 [B, T3, 8, 512] (block 4 conv1's output, channels last) -> capture 8 [B, 8 T3 + 1, 512]."""
    x = x7.permute(0, 3, 1, 2)                                               # [B, 512, T3, 8]
    y = F.relu(O._bn(sd, 'conv_block4.bn2', F.conv2d(x, O._t(sd['conv_block4.conv2.weight']).to(x.dtype), padding=1)))
    B, C, T3, Fq = y.shape
    y = y.reshape(B, C, T3 * Fq).permute(0, 2, 1)                             # token t * 8 + f
    tag = tag_token(sd).to(y.dtype)[None, None, :].expand(B, 1, C)
    return torch.cat([tag, y], dim=1)


def step(sd, src, x):
    """The step from capture id ``src`` to the next one."""
    if src == 7:
        return tokens(sd, x)
    if x.shape[1] > MAX_TOKENS:
        raise ValueError('sequence longer than the positional table')
    return CR.step(sd, src, x)                                               # 8: the input layer on the token rows


def classifier(sd, x):
    """x [B, Ts, 144] (the encoder output) -> logits [B, Ts, C]."""
    return F.linear(x, sd['classifier.weight'], sd['classifier.bias'])


def split(logits):
    return {'framewise_output': logits[:, 1:, :], 'clipwise_output': logits[:, 0, :]}


def head(sd, x):
    return split(classifier(sd, x))
