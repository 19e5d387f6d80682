"""Test infrastructure: torch restatement of the forwards of the five other
9-layer models, built from the oracle's own layer functions
(``oracle.sed_oracle``: logmel, cnn, gru_bidirectional, multihead, att_block;
imported, not edited) plus the fc / sigmoid / interpolate / mean-or-max head.
Every function takes whatever dtype its state dict and input carry: float32
is the reference's own arithmetic, float64 the high-precision yardstick of
tests/test_gpu_family.py.  CPU only; nothing here imports the library.

  Cnn_9layers_FrameMax               pytorch/models.py:255-295
  Cnn_9layers_FrameAvg               :340-380
  Cnn_9layers_FrameAtt               :423-461
  Cnn_9layers_Gru_FrameAvg           :512-561
  Cnn_9layers_Transformer_FrameAvg   :929-978
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import sed_oracle as O
from sedx import synth

FMAX, FAVG, FATT = 'Cnn_9layers_FrameMax', 'Cnn_9layers_FrameAvg', 'Cnn_9layers_FrameAtt'
GAVG, TAVG = 'Cnn_9layers_Gru_FrameAvg', 'Cnn_9layers_Transformer_FrameAvg'
FAMILY = (FMAX, FAVG, FATT, GAVG, TAVG)
FC_MODELS = (FMAX, FAVG, GAVG, TAVG)
IDS = {FMAX: 'fmax', FAVG: 'favg', FATT: 'fatt', GAVG: 'gavg', TAVG: 'tavg'}
SEEDS = synth.GOLDEN_SEEDS
KEYS = ('framewise_output', 'clipwise_output', 'embedding')
P16 = (16000, 512, 160, 64, 25, 7000)


def ctor_args(mt, classes_num=25, preset=P16):
    """Constructor arguments of the reference class: seven for the CNN-only
    models (models.py:214-215, :299-300, :384-385), eight otherwise."""
    return preset + ((classes_num,) if synth.MODEL_PARTS[mt][0] is None else (classes_num, 'logmel'))


def state(mt, classes_num=25, seed=None, dtype=torch.float32):
    """``synth.make_state_dict`` as torch tensors of ``dtype``."""
    sd = {}
    for k, v in synth.make_state_dict(mt, classes_num=classes_num,
                                      seed=SEEDS[mt] if seed is None else seed).items():
        t = torch.from_numpy(np.asarray(v))
        sd[k] = t.to(dtype) if t.is_floating_point() else t
    return sd


def full_state(mt, classes_num=25, seed=None, preset='16k'):
    return O.full_state(state(mt, classes_num, seed), preset)


def interpolate(x, ratio=8):
    """models.py:84-95: every frame repeated ``ratio`` times."""
    B, T, C = x.shape
    return x[:, :, None, :].repeat(1, 1, ratio, 1).reshape(B, T * ratio, C)


def seq_layer(sd, mt, x):
    """The head's input from the CNN output: x [B, 512, T/8] -> [B, T/8, 512]
    (models.py:543-545 GRU, :960-962 MultiHead; the CNN-only models
    transpose only, :283, :368)."""
    x = x.transpose(1, 2)
    seq = synth.MODEL_PARTS[mt][0]
    if seq == 'gru':
        return O.gru_bidirectional(sd, x)
    if seq == 'mha':
        return O.multihead(sd, x)
    return x.contiguous()


def head(sd, mt, x):
    """x [B, T/8, 512] (the head's input) -> the three outputs.
    fc models (models.py:282-293, :367-378, :548-559, :965-976):
      framewise = interpolate(sigmoid(fc(x)), 8); clipwise = max over the
      frames (FrameMax, :288) or mean (:373, :554, :971); embedding = x
      transposed.
    Cnn_9layers_FrameAtt (:449-459): AttBlock; framewise = interpolate(cla),
      no padding; embedding = cla."""
    if mt == FATT:
        clipwise, _, cla = O.att_block(sd, x.transpose(1, 2))
        return {'framewise_output': O.framewise_from_cla(cla, False), 'clipwise_output': clipwise,
                'embedding': cla}
    fw = interpolate(torch.sigmoid(F.linear(x, O._t(sd['fc.weight']), O._t(sd['fc.bias']))), 8)
    clipwise = torch.max(fw, dim=1)[0] if mt == FMAX else torch.mean(fw, dim=1)
    return {'framewise_output': fw, 'clipwise_output': clipwise, 'embedding': x.transpose(1, 2)}


def absbound_head(sd, mt, x):
    """Per-element magnitude sums S of the fc projection of the head's input
    ``x`` [B, T/8, 512], laid out as framewise and clipwise (the bound of the
    split-bf16 mode, as oracle.layer_refs.absbound_head: the sigmoid is
    1/4-Lipschitz, the max / mean over frames does not expand the largest
    frame's error)."""
    s = F.linear(x.abs(), O._t(sd['fc.weight']).abs(), O._t(sd['fc.bias']).abs())
    return {'framewise_output': interpolate(s, 8), 'clipwise_output': s.amax(dim=1)}


def forward(sd, mt, wave=None, features=None, return_acts=False):
    """Eval-mode forward of one of the five models.  ``wave`` [B, L] or
    ``features`` [B, 1, T, 64]; ``sd`` holds the frontend tensors and '_hop'
    (``O.full_state``)."""
    with torch.no_grad():
        x = O.logmel(sd, O._t(wave).float()) if features is None else O._t(features)
        x, acts = O.cnn(sd, x)
        x = seq_layer(sd, mt, x)
        acts['seq_out'] = x
        out = head(sd, mt, x)
    return (out, acts) if return_acts else out


def predict_windows(sd, mt, audio, sample_rate, sample_duration=5, overlap_value=1.0, overlap=True):
    """predict.py:297-349 around ``forward``, through the oracle's own loop
    control, merge and avg_merge (``O.predict_windows`` with the model call
    swapped: its ``forward`` knows the two FrameAtt models only)."""
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
