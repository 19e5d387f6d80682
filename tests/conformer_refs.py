"""Test infrastructure: torch restatement of the eval-mode forwards of
``Cnn_9layers_Conformer_FrameAtt`` and ``Cnn_9layers_Conformer_FrameAvg``
(pytorch/models.py:1189-1410, :1412-1625; pytorch/models_2020/conformer/),
written from the model's description: one function per captured step (input
layer, Macaron feed-forward, relative-position attention, convolution module,
final norm, each head), on the oracle's own ``logmel`` and ``cnn``
(``oracle.sed_oracle``, imported, not edited).  Every function takes whatever
dtype its state dict and input carry: float32 is the reference's arithmetic,
float64 the yardstick of tests/test_gpu_conformer.py.  CPU only by default
(the functions run wherever their tensors live); nothing here imports the
library.

Capture ids (include/sedx.h, sedx_set_capture), all [B, T3, 144]:
  20           input layer output
  21 + 4b + j  block b: after ffn1 (j = 0), mhsa (1), conv module (2), the
               block output = norm(ffn2 step) (3); 32 is the encoder output (9)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sed_oracle as O
from sedx import synth

CATT, CAVG = 'Cnn_9layers_Conformer_FrameAtt', 'Cnn_9layers_Conformer_FrameAvg'
MODELS = (CATT, CAVG)
IDS = {CATT: 'catt', CAVG: 'cavg'}
SEEDS = synth.CONFORMER_GOLDEN_SEEDS
KEYS = ('framewise_output', 'clipwise_output', 'embedding')
P16 = (16000, 512, 160, 64, 25, 7000)
D, FF, HEADS, BLOCKS, KERNEL, MAX_LEN = 144, 576, 4, 3, 7, 5000
ACT_IDS = tuple(range(20, 33))                   # the 13 captured encoder activations
STEPS = [(8, 20)] + [(i, i + 1) for i in range(20, 32)]


def pe_table(dtype=torch.float32):
    """embedding.py:19-24: [1, 5000, 144], computed in float32 like the buffer."""
    pe = torch.zeros(MAX_LEN, D)
    position = torch.arange(0, MAX_LEN, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, D, 2, dtype=torch.float32) * -(math.log(10000.0) / D))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.unsqueeze(0).to(dtype)


def inv_freq(dtype=torch.float32):
    """attention.py:132 (a float32 buffer)."""
    return (1 / (10000 ** (torch.arange(0.0, D, 2.0) / D))).to(dtype)


def state(mt, classes_num=25, seed=None, dtype=torch.float32):
    """``synth.make_state_dict`` as torch tensors of ``dtype``, plus the
    constant buffers the model constructor provides (``pe``, ``inv_freq``)."""
    sd = {}
    for k, v in synth.make_state_dict(mt, classes_num=classes_num,
                                      seed=SEEDS[mt] if seed is None else seed).items():
        t = torch.from_numpy(np.asarray(v))
        sd[k] = t.to(dtype) if t.is_floating_point() else t
    sd['encoder.input_layer.4.pe'] = pe_table(dtype)
    for b in range(BLOCKS):
        sd['encoder.conformer_blocks.%d.mhsa.pos_emb.inv_freq' % b] = inv_freq(dtype)
    return sd


def full_state(mt, classes_num=25, seed=None, preset='16k'):
    return O.full_state(state(mt, classes_num, seed), preset)


def _ln(sd, p, x):
    return F.layer_norm(x, (D,), sd[p + '.weight'], sd[p + '.bias'], 1e-5)


def _blk(b):
    return 'encoder.conformer_blocks.%d.' % b


# ---------------------------------------------------------------------------
# steps: x [B, T3, 144] unless noted
# ---------------------------------------------------------------------------
def input_layer(sd, x):
    """x [B, T3, 512] -> Linear, LayerNorm, ReLU, x sqrt(144) + pe[t]."""
    T = x.shape[1]
    if T > MAX_LEN:
        raise ValueError('sequence longer than the positional table')
    y = F.linear(x, sd['encoder.input_layer.0.weight'], sd['encoder.input_layer.0.bias'])
    y = F.relu(_ln(sd, 'encoder.input_layer.1', y))
    return y * math.sqrt(D) + sd['encoder.input_layer.4.pe'][:, :T].to(y.dtype)


def ffn(sd, b, name, x):
    """x = 0.5 ffn(x) + x; ffn = LN, Linear(144, 576), Swish, Linear(576, 144)."""
    p = _blk(b) + name + '.feed_forward_module.'
    y = F.linear(_ln(sd, p + '0', x), sd[p + '1.weight'], sd[p + '1.bias'])
    y = y * torch.sigmoid(y)
    return 0.5 * F.linear(y, sd[p + '4.weight'], sd[p + '4.bias']) + x


def rel_shift(bd0):
    """``_rel_shift`` in closed form on bd0 [..., T, T] (query i, position j):
       j <= i      bd0[i][j + T - 1 - i]
       j == i + 1  0
       j >= i + 2  bd0[i + 1][j - i - 2]     (the next query's row)."""
    T = bd0.shape[-1]
    i = torch.arange(T, device=bd0.device)[:, None]
    j = torch.arange(T, device=bd0.device)[None, :]
    lo, hi = j <= i, j >= i + 2
    row = torch.where(hi, i + 1, i.expand(T, T)).clamp(max=T - 1)
    col = torch.where(lo, j + T - 1 - i, j - i - 2).clamp(min=0, max=T - 1)
    out = bd0[..., row, col]
    return torch.where(lo | hi, out, torch.zeros((), dtype=bd0.dtype, device=bd0.device))


def rel_shift_pad_view(bd0):
    """The pad-and-view evaluation (a zero column in front, viewed as
    [T + 1, T], first row dropped) on bd0 [T, T]: what the closed form restates."""
    T = bd0.shape[0]
    padded = torch.cat([torch.zeros(T, 1, dtype=bd0.dtype), bd0], dim=1)     # [T, T + 1]
    return padded.reshape(T + 1, T)[1:].reshape(T, T)


def rel_positions(sd, b, T, dtype, device=None):
    """r [T, 144] = [sin(p f), cos(p f)], p = T - 1 - j."""
    pos = torch.arange(T - 1, -1, -1.0, dtype=dtype, device=device)
    s = torch.outer(pos, sd[_blk(b) + 'mhsa.pos_emb.inv_freq'].to(dtype))
    return torch.cat([s.sin(), s.cos()], dim=-1)


def mhsa(sd, b, x):
    """x + o_net(attention), pre-LayerNorm, relative positions (Transformer-XL)."""
    p = _blk(b) + 'mhsa.'
    B, T, _ = x.shape
    dh = D // HEADS
    w = F.linear(_ln(sd, p + 'layer_norm', x), sd[p + 'qkv_net.weight'])
    q, k, v = (t.reshape(B, T, HEADS, dh) for t in torch.chunk(w, 3, dim=-1))
    rk = F.linear(rel_positions(sd, b, T, x.dtype, x.device), sd[p + 'r_net.weight']).reshape(T, HEADS, dh)
    ac = torch.einsum('bind,bjnd->bnij', q + sd[p + 'r_w_bias'], k)
    bd = rel_shift(torch.einsum('bind,jnd->bnij', q + sd[p + 'r_r_bias'], rk))
    prob = torch.softmax((ac + bd) * (1 / (dh ** 0.5)), dim=-1)
    vec = torch.einsum('bnij,bjnd->bind', prob, v).reshape(B, T, D)
    return x + F.linear(vec, sd[p + 'o_net.weight'])


def conv_module(sd, b, x):
    """x + pointwise(Swish(BN(depthwise(GLU(pointwise(LN(x)))))))."""
    p = _blk(b) + 'conv.conv.'
    y = _ln(sd, p + '0', x).transpose(1, 2)                                   # [B, 144, T]
    y = F.conv1d(y, sd[p + '1.conv.weight'], sd[p + '1.conv.bias'])
    y = y[:, :D] * torch.sigmoid(y[:, D:])
    y = F.conv1d(y, sd[p + '3.conv.weight'], sd[p + '3.conv.bias'], padding=KERNEL // 2, groups=D)
    y = F.batch_norm(y, sd[p + '5.running_mean'], sd[p + '5.running_var'], sd[p + '5.weight'], sd[p + '5.bias'],
                     False, 0.0, 1e-5)
    y = y * torch.sigmoid(y)
    y = F.conv1d(y, sd[p + '8.conv.weight'], sd[p + '8.conv.bias'])
    return y.transpose(1, 2) + x


def final_norm(sd, b, x):
    return _ln(sd, _blk(b) + 'norm', x)


def step(sd, src, x):
    """The step from capture id ``src`` (8: x [B, T3, 512]) to the next id."""
    if src == 8:
        return input_layer(sd, x)
    b, j = divmod(src - 20, 4)
    if j == 0:
        return ffn(sd, b, 'ffn1', x)
    if j == 1:
        return mhsa(sd, b, x)
    if j == 2:
        return conv_module(sd, b, x)
    return final_norm(sd, b, ffn(sd, b, 'ffn2', x))


def encoder(sd, x, acts=None):
    """x [B, T3, 512] -> [B, T3, 144]; ``acts`` (a dict) receives the 13
    activations under their capture ids."""
    for src, dst in STEPS:
        x = step(sd, src, x)
        if acts is not None:
            acts[dst] = x
    return x


def interpolate_pad(x, ratio=8):
    """x8 frame repeat, then (unless that gives 1000 frames) the last frame
    repeated up to the next multiple of 100."""
    B, T, C = x.shape
    fw = x[:, :, None, :].repeat(1, 1, ratio, 1).reshape(B, T * ratio, C)
    if fw.shape[1] != 1000:
        n = O.roundup(fw.shape[1])
        fw = torch.cat([fw, fw[:, -1:, :].repeat(1, n - fw.shape[1], 1)], dim=1)
    return fw


def head(sd, mt, x):
    """x [B, T3, 144] (the encoder output) -> the three outputs."""
    emb = x.transpose(1, 2)
    if mt == CATT:
        clipwise, _, cla = O.att_block(sd, emb)
        return {'framewise_output': interpolate_pad(cla.transpose(1, 2)), 'clipwise_output': clipwise,
                'embedding': emb}
    fw = interpolate_pad(torch.sigmoid(F.linear(x, sd['fc.weight'], sd['fc.bias'])))
    return {'framewise_output': fw, 'clipwise_output': torch.mean(fw, dim=1), 'embedding': emb}


def forward(sd, mt, wave=None, features=None, return_acts=False):
    """Eval-mode forward.  ``wave`` [B, L] or ``features`` [B, 1, T, 64];
    ``sd`` holds the frontend tensors and '_hop' (``full_state``)."""
    with torch.no_grad():
        x = O.logmel(sd, O._t(wave).float()) if features is None else O._t(features)
        x, acts = O.cnn(sd, x)
        x = encoder(sd, x.transpose(1, 2), acts)
        out = head(sd, mt, x)
    return (out, acts) if return_acts else out


def predict_windows(sd, mt, audio, sample_rate, sample_duration=5, overlap_value=1.0, overlap=True):
    """predict.py:297-349 around ``forward``, through the oracle's own loop
    control, merge and avg_merge."""
    audio_duration = len(audio) / float(sample_rate)
    n_win = int(sample_rate * sample_duration)
    merged, prev = None, None
    stride = O.driver_stride('predict', sample_duration, overlap_value, overlap)
    for num_segment, start in enumerate(O.window_starts(audio_duration, sample_duration, stride), start=1):
        s = int(start * sample_rate)
        seg = O.pad_truncate_sequence(audio[s:int(sample_duration * sample_rate) + s], n_win)
        seg = torch.Tensor(np.asarray(seg))[None, :]
        curr = forward(sd, mt, wave=seg)['framewise_output'].numpy()
        if num_segment == 1:
            merged = curr
        elif num_segment == 2:
            merged = O.merge(prev, curr, sample_duration, num_segment, overlap_value)
        else:
            merged = O.merge(merged, curr, sample_duration, num_segment, overlap_value)
        prev = curr
    return O.avg_merge(merged, sample_duration, overlap_value)
