"""Drop-in model classes for the reference's hot path (pytorch/models.py).

``Cnn_9layers_Gru_FrameAtt`` and ``Cnn_9layers_Transformer_FrameAtt`` keep the
reference constructor ``(sample_rate, window_size, hop_size, mel_bins, fmin,
fmax, classes_num, feature_type)``, ``forward(input, mixup_lambda=None,
timeshift=False, spec_augment=True)`` and the exact state_dict keys/shapes
(so ``model.load_state_dict(torch.load(path)['model'])`` works unchanged).
The reference's five other models on the same 9-layer trunk
(``Cnn_9layers_FrameMax``, ``Cnn_9layers_FrameAvg``, ``Cnn_9layers_FrameAtt``:
seven constructor arguments, ``forward(input, mixup_lambda=None)``;
``Cnn_9layers_Gru_FrameAvg``, ``Cnn_9layers_Transformer_FrameAvg``) follow the
same rule, and so do the two Conformer models on that trunk
(``Cnn_9layers_Conformer_FrameAtt``, ``Cnn_9layers_Conformer_FrameAvg``:
``(..., classes_num, cnn_kwargs=None, encoder_kwargs=None,
encoder_type="Conformer", pooling="token", layer_init="pytorch")`` and
``forward(x, mixup_lambda=None, timeshift=False, spec_augment=True,
mask=None)``), and the two models on the 14-layer trunk
(``Cnn_14layers_Gru_FrameAtt``, ``Cnn_14layers_Transformer_FrameAtt``: eight
constructor arguments, 25 classes; ``Cnn_14layers_Conformer_FrameAtt``: the
Conformer constructor after ``feature_type``, 25 classes, 144-wide embedding,
every sequence frame repeated ``1000 // seq_len`` times; ``Cnn_9layers_Conformer``: the Conformer
constructor, every (frame, frequency bin) pixel of block 4 a token behind a learned tag token,
``forward(x, mixup_lambda=None, timeshift=False, mask=None)`` returning LOGITS under the reference's
two keys; ``Cnn_9layers_Gru_Reg``: ``Cnn_9layers_Gru_FrameAtt`` without the framewise padding, 25
classes), and ``Cnn14_DecisionLevelAtt`` (the PANNs
architecture: seven constructor arguments, up to 527 classes,
``forward(input, mixup_lambda=None)`` returning the reference's two keys, no
``'embedding'``), and the three transfer-learning models on the VGGish trunk
(``VGGish_FrameAtt``, ``VGGish_Gru_FrameAtt``, ``VGGish_FrameAvg``: ten
constructor arguments with ``checkpoint_path`` and ``freeze``, 25 classes, always
1000 output frames).  The submodules are parameter containers; the whole eval-mode forward runs in
libsedx (HIP kernels for gfx950) through the C ABI in include/sedx.h.  There
is no CPU or eager-PyTorch fallback: a non-HIP input raises.

Usage mirrors the reference call sites (pytorch/predict.py:229-242, 311-313):

    Model = getattr(sedx.models, model_type)
    model = Model(16000, 512, 160, 64, 25, 7000, 25, 'logmel')
    model.load_state_dict(checkpoint['model'])
    model.to('cuda').eval()
    with torch.no_grad():
        out = model(waveform_on_gpu)      # {'framewise_output', 'clipwise_output', 'embedding'}
"""
import ctypes
import math
import threading
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .stft import Spectrogram, LogmelFilterBank

__all__ = ['Cnn_9layers_Gru_FrameAtt', 'Cnn_9layers_Transformer_FrameAtt',
           'Cnn_14layers_Gru_FrameAtt', 'Cnn_14layers_Transformer_FrameAtt', 'Cnn14_DecisionLevelAtt',
           'Cnn_14layers_Conformer_FrameAtt', 'Cnn_9layers_Conformer', 'Cnn_9layers_Gru_Reg',
           'VGGish', 'VGGish_FrameAtt', 'VGGish_Gru_FrameAtt', 'VGGish_FrameAvg',
           'Cnn_9layers_FrameMax', 'Cnn_9layers_FrameAvg', 'Cnn_9layers_FrameAtt',
           'Cnn_9layers_Gru_FrameAvg', 'Cnn_9layers_Transformer_FrameAvg',
           'Cnn_9layers_Conformer_FrameAtt', 'Cnn_9layers_Conformer_FrameAvg', 'ConformerEncoder', 'ConvBlock',
           'AttBlock', 'MultiHead', 'interpolate', 'pad_framewise_output', 'roundup',
           'init_layer', 'init_bn', 'init_gru']

# sedx_model (include/sedx.h)
MODEL_IDS = {'Cnn_9layers_Gru_FrameAtt': 0, 'Cnn_9layers_Transformer_FrameAtt': 1,
             'Cnn_9layers_FrameMax': 2, 'Cnn_9layers_FrameAvg': 3, 'Cnn_9layers_FrameAtt': 4,
             'Cnn_9layers_Gru_FrameAvg': 5, 'Cnn_9layers_Transformer_FrameAvg': 6,
             'Cnn_9layers_Conformer_FrameAtt': 7, 'Cnn_9layers_Conformer_FrameAvg': 8,
             'Cnn_14layers_Gru_FrameAtt': 10, 'Cnn_14layers_Transformer_FrameAtt': 11,   # 9 is not assigned
             'Cnn14_DecisionLevelAtt': 13,                                              # nor is 12
             'VGGish_FrameAtt': 15, 'VGGish_Gru_FrameAtt': 16, 'VGGish_FrameAvg': 17,   # nor is 14
             'Cnn_14layers_Conformer_FrameAtt': 19,                                     # nor is 18
             'Cnn_9layers_Conformer': 21, 'Cnn_9layers_Gru_Reg': 22}                    # nor is 20
FEATURE_IDS = {'logmel': 0, 'gamma': 1}


# ---------------------------------------------------------------------------
# reference helpers (pytorch/models.py:20-95)
# ---------------------------------------------------------------------------
def init_layer(layer):
    """models.py:20-26"""
    nn.init.xavier_uniform_(layer.weight)
    if getattr(layer, 'bias', None) is not None:
        layer.bias.data.fill_(0.)


def init_bn(bn):
    """models.py:29-32"""
    bn.bias.data.fill_(0.)
    bn.weight.data.fill_(1.)


def init_gru(rnn):
    """models.py:35-60: U(+-sqrt(3/fan_in)) per gate block, orthogonal n-gate
    recurrent block, zero biases -- of the forward-direction tensors only
    (``weight_ih_l{i}`` etc.); the ``_reverse`` tensors keep nn.GRU's own
    initialisation, as in the reference."""
    def _concat_init(tensor, init_funcs):
        length, fan_out = tensor.shape
        fan_in = length // len(init_funcs)
        for i, fn in enumerate(init_funcs):
            fn(tensor[i * fan_in:(i + 1) * fan_in, :])

    def _inner_uniform(tensor):
        fan_in = nn.init._calculate_correct_fan(tensor, 'fan_in')
        nn.init.uniform_(tensor, -math.sqrt(3 / fan_in), math.sqrt(3 / fan_in))

    for i in range(rnn.num_layers):
        _concat_init(getattr(rnn, 'weight_ih_l%d' % i), [_inner_uniform] * 3)
        nn.init.constant_(getattr(rnn, 'bias_ih_l%d' % i), 0)
        _concat_init(getattr(rnn, 'weight_hh_l%d' % i),
                     [_inner_uniform, _inner_uniform, nn.init.orthogonal_])
        nn.init.constant_(getattr(rnn, 'bias_hh_l%d' % i), 0)


def roundup(x):
    """models.py:62-63"""
    return x if x % 100 == 0 else x + 100 - x % 100


def pad_framewise_output(framewise_output, frames_num):
    """models.py:65-81 (tensor helper; the model forward does this natively)."""
    pad = framewise_output[:, -1:, :].repeat(1, frames_num - framewise_output.shape[1], 1)
    return torch.cat((framewise_output, pad), dim=1)


def interpolate(x, ratio):
    """models.py:84-95 (tensor helper; the model forward does this natively)."""
    b, t, c = x.shape
    return x[:, :, None, :].repeat(1, 1, ratio, 1).reshape(b, t * ratio, c)


# ---------------------------------------------------------------------------
# parameter containers with the reference module names
# ---------------------------------------------------------------------------
class ConvBlock(nn.Module):
    """models.py:98-141 (weights only; conv+BN+ReLU+pool run in libsedx)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, out_channels, (3, 3), (1, 1), (1, 1), bias=False)
        self.conv2 = nn.Conv2d(out_channels, out_channels, (3, 3), (1, 1), (1, 1), bias=False)
        self.bn1 = nn.BatchNorm2d(out_channels)
        self.bn2 = nn.BatchNorm2d(out_channels)
        init_layer(self.conv1)
        init_layer(self.conv2)
        init_bn(self.bn1)
        init_bn(self.bn2)

    def forward(self, input, pool_size=(2, 2), pool_type='avg'):
        raise RuntimeError('ConvBlock is fused into the native model forward (libsedx)')


class AttBlock(nn.Module):
    """models.py:144-175 (weights only)."""

    def __init__(self, n_in, n_out, activation='linear', temperature=1.):
        super().__init__()
        self.activation = activation
        self.temperature = temperature
        self.att = nn.Conv1d(n_in, n_out, kernel_size=1, stride=1, padding=0, bias=True)
        self.cla = nn.Conv1d(n_in, n_out, kernel_size=1, stride=1, padding=0, bias=True)
        self.bn_att = nn.BatchNorm1d(n_out)
        init_layer(self.att)
        init_layer(self.cla)
        init_bn(self.bn_att)

    def forward(self, x):
        raise RuntimeError('AttBlock is fused into the native model forward (libsedx)')


class MultiHead(nn.Module):
    """models.py:823-877 (weights only)."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.1):
        super().__init__()
        if (n_head, d_k, d_v) != (8, 64, 64) or d_model not in (512, 2048):
            raise ValueError('the native MHA implements the reference shapes (8 heads, 512 or 2048, 64, 64)')
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = nn.Linear(d_model, n_head * d_k)
        self.w_ks = nn.Linear(d_model, n_head * d_k)
        self.w_vs = nn.Linear(d_model, n_head * d_v)
        nn.init.normal_(self.w_qs.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_k)))
        nn.init.normal_(self.w_ks.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_k)))
        nn.init.normal_(self.w_vs.weight, mean=0, std=np.sqrt(2.0 / (d_model + d_v)))
        for m in (self.w_qs, self.w_ks, self.w_vs):
            m.bias.data.fill_(0)
        self.layer_norm = nn.LayerNorm(d_model)
        self.fc = nn.Linear(n_head * d_v, d_model)
        nn.init.xavier_normal_(self.fc.weight)
        self.fc.bias.data.fill_(0)

    def forward(self, q, k, v, mask=None):
        raise RuntimeError('MultiHead is fused into the native model forward (libsedx)')


# ---------------------------------------------------------------------------
# Conformer encoder containers (pytorch/models_2020/conformer/): the module
# tree of the reference, so the state_dict has its keys, shapes and order
# ---------------------------------------------------------------------------
def _fused(name):
    def forward(self, *args, **kwargs):
        raise RuntimeError('%s is fused into the native model forward (libsedx)' % name)
    return forward


class _Slot(nn.Module):
    """A parameter-free position of an nn.Sequential (Swish, GLU, Permute)."""
    forward = _fused('the Conformer encoder')


class _PositionalEncoding(nn.Module):
    """models_2020/transformer/embedding.py:8-31: the ``pe`` buffer
    [1, max_len, d_model], sin on the even columns, cos on the odd."""

    def __init__(self, d_model, dropout_rate, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout_rate)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float32).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float32) * -(math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.max_len = max_len
        self.xscale = math.sqrt(d_model)
        self.register_buffer('pe', pe.unsqueeze(0))

    forward = _fused('PositionalEncoding')


class _MacaronFeedForward(nn.Module):
    """conformer/macaron_feed_forward.py: LN, Linear, Swish, Dropout, Linear, Dropout."""

    def __init__(self, d_model, d_ff, dropout):
        super().__init__()
        self.feed_forward_module = nn.Sequential(nn.LayerNorm(d_model), nn.Linear(d_model, d_ff), _Slot(),
                                                 nn.Dropout(dropout), nn.Linear(d_ff, d_model),
                                                 nn.Dropout(dropout))

    forward = _fused('MacaronFeedForward')


class _PositionalEmbedding(nn.Module):
    """conformer/attention.py:126-133: the ``inv_freq`` buffer."""

    def __init__(self, demb):
        super().__init__()
        self.demb = demb
        self.register_buffer('inv_freq', 1 / (10000 ** (torch.arange(0.0, demb, 2.0) / demb)))

    forward = _fused('PositionalEmbedding')


class _RelMultiHeadAttn(nn.Module):
    """conformer/attention.py:145-172 (pre_lnorm=True; weights only)."""

    def __init__(self, n_head, d_model, dropout):
        super().__init__()
        self.n_head, self.d_model, self.d_head = n_head, d_model, d_model // n_head
        self.qkv_net = nn.Linear(d_model, 3 * n_head * self.d_head, bias=False)
        self.drop = nn.Dropout(dropout)
        self.dropatt = nn.Dropout(0)
        self.o_net = nn.Linear(n_head * self.d_head, d_model, bias=False)
        self.layer_norm = nn.LayerNorm(d_model)
        self.pos_emb = _PositionalEmbedding(d_model)
        self.r_w_bias = nn.Parameter(torch.zeros(n_head, self.d_head))
        self.r_r_bias = nn.Parameter(torch.zeros(n_head, self.d_head))
        self.r_net = nn.Linear(d_model, n_head * self.d_head, bias=False)

    forward = _fused('RelMultiHeadAttn')


class _Conv1dBox(nn.Module):
    """conformer/convolution.py:5-28: a Conv1d under the name ``conv``."""

    def __init__(self, cin, cout, kernel_size, padding, groups):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, kernel_size, 1, padding, groups=groups)

    forward = _fused('ConvolutionModule')


class _ConvolutionModule(nn.Module):
    """conformer/convolution.py:38-55: LN, pointwise, GLU, depthwise, Permute,
    BatchNorm1d, Permute, Swish, pointwise, Dropout."""

    def __init__(self, d_model, dropout, kernel_size):
        super().__init__()
        self.conv = nn.Sequential(nn.LayerNorm(d_model), _Conv1dBox(d_model, 2 * d_model, 1, 0, 1), _Slot(),
                                  _Conv1dBox(d_model, d_model, kernel_size, int(kernel_size / 2), d_model),
                                  _Slot(), nn.BatchNorm1d(d_model), _Slot(), _Slot(),
                                  _Conv1dBox(d_model, d_model, 1, 0, 1), nn.Dropout(dropout))

    forward = _fused('ConvolutionModule')


class _ConformerBlock(nn.Module):
    """conformer/conformer_block.py:7-14."""

    def __init__(self, d_model, d_ff, n_head, dropout, kernel_size):
        super().__init__()
        self.ffn1 = _MacaronFeedForward(d_model, d_ff, dropout)
        self.mhsa = _RelMultiHeadAttn(n_head, d_model, dropout)
        self.conv = _ConvolutionModule(d_model, dropout, kernel_size)
        self.ffn2 = _MacaronFeedForward(d_model, d_ff, dropout)
        self.norm = nn.LayerNorm(d_model)

    forward = _fused('ConformerBlock')


class ConformerEncoder(nn.Module):
    """conformer/conformer_encoder.py:7-29 (weights only).  The native encoder
    implements the reference's one shape: (512, 144, 3 blocks, 576, 4 heads,
    kernel 7), with idim 2048 on the 14-layer trunk."""

    def __init__(self, idim, adim=144, dropout_rate=0.1, elayers=3, eunits=576, aheads=4, kernel_size=7):
        super().__init__()
        if idim not in (512, 2048) or (adim, elayers, eunits, aheads, kernel_size) != (144, 3, 576, 4, 7):
            raise ValueError('the native Conformer encoder implements the reference shape '
                             '(idim 512 or 2048, adim 144, elayers 3, eunits 576, aheads 4, kernel_size 7)')
        self.input_layer = nn.Sequential(nn.Linear(idim, adim), nn.LayerNorm(adim), nn.Dropout(dropout_rate),
                                         nn.ReLU(), _PositionalEncoding(adim, dropout_rate))
        self.conformer_blocks = nn.Sequential(*[_ConformerBlock(adim, eunits, aheads, dropout_rate, kernel_size)
                                                for _ in range(elayers)])

    forward = _fused('ConformerEncoder')


# ---------------------------------------------------------------------------
# native handle management
# ---------------------------------------------------------------------------
class _Native(object):
    def __init__(self, cfg, device_index):
        L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(L.sedx_create(ctypes.byref(cfg), device_index, ctypes.byref(h)), None,
                   'sedx_create(model=%d, feature=%d)' % (cfg.model_type, cfg.feature_type))
        self.h = h
        self.device_index = device_index
        self.signature = None
        self.precision = 'winograd'   # the library default (sedx_set_precision)

    def load(self, state_dict):
        L = _lib.lib()
        for k, v in state_dict.items():
            if k.endswith('num_batches_tracked'):
                continue
            a = np.ascontiguousarray(v.detach().to('cpu', torch.float32).numpy())
            shape = (ctypes.c_int64 * a.ndim)(*a.shape)
            _lib.check(L.sedx_load_param(self.h, k.encode(), a.ctypes.data_as(ctypes.c_void_p),
                                         shape, a.ndim), self.h, 'load_param(%s)' % k)
        _lib.check(L.sedx_finalize_weights(self.h), self.h, 'finalize_weights')

    def __del__(self):
        try:
            if self.h:
                _lib.lib().sedx_destroy(self.h)
        except Exception:
            pass


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


# generation of the module tree anywhere in the process: bumped whenever a
# parameter, buffer or submodule is registered (setattr of an nn.Parameter /
# register_buffer / add_module), so _SedModel._signature re-walks its
# state_dict only after such a change
_REG_GEN = [0]


def _bump_reg_gen(*_args):
    _REG_GEN[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_bump_reg_gen)
torch.nn.modules.module.register_module_buffer_registration_hook(_bump_reg_gen)
torch.nn.modules.module.register_module_module_registration_hook(_bump_reg_gen)


class _HandleCache(dict):
    """device index -> _Native, shared by a model and its DataParallel
    replicas.  ``torch.nn.DataParallel`` (pytorch/predict.py:239,
    pytorch/main_strong.py:541) re-replicates the module on every forward
    (``Module._replicate_for_data_parallel``: a shallow ``__dict__`` copy, so
    this object is shared) and hands each replica parameters freshly broadcast
    to its device, i.e. new ``data_ptr``s every call.  The replicas' weights
    are copies of the source module's, so a replica's handle is keyed on the
    SOURCE module's parameters (``source``) and the per-device handle is
    packed once, not once per call.  ``lock`` serialises handle creation and
    packing across DataParallel's per-device threads.  Copies and pickles of
    a model start with an empty cache (a handle owns device memory)."""

    def __init__(self, owner=None):
        super().__init__()
        self.lock = threading.Lock()
        self.source = weakref.ref(owner) if owner is not None else None

    def __reduce__(self):
        return (_HandleCache, ())


class _SedModel(nn.Module):
    """Shared construction (the 9-layer CNN trunk) + native forward of every
    model class below.  ``classes_num`` is the class count of the outputs and
    of the native handle."""

    _model_name = None
    # 'embedding' is cla (batch, classes, seq) for the AttBlock models that
    # return it (models.py:459, :686); every other model returns the head's
    # 512-channel input (batch, 512, seq)
    _embedding_cla = False
    _embedding_width = 512     # 144 after the Conformer encoder
    _has_embedding = True      # False: the reference's forward returns no 'embedding' (Cnn14_DecisionLevelAtt)
    _cnn9_trunk = True         # False: the class registers its own trunk (the VGGish models)

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type='logmel'):
        super().__init__()
        if mel_bins != 64:
            raise ValueError('mel_bins must be 64 (bn0 = BatchNorm2d(64), models.py:607)')
        self.feature_type = feature_type
        self.sample_rate, self.window_size, self.hop_size = sample_rate, window_size, hop_size
        self.mel_bins, self.fmin, self.fmax, self.classes_num = mel_bins, fmin, fmax, classes_num
        self.spectrogram_extractor = Spectrogram(n_fft=window_size, hop_length=hop_size,
                                                 win_length=window_size, window='hann',
                                                 center=True, pad_mode='reflect',
                                                 freeze_parameters=True)
        self.logmel_extractor = LogmelFilterBank(sr=sample_rate, n_fft=window_size,
                                                 n_mels=mel_bins, fmin=fmin, fmax=fmax, ref=1.0,
                                                 amin=1e-10, top_db=None, freeze_parameters=True)
        self.bn0 = nn.BatchNorm2d(64)
        if self._cnn9_trunk:
            self.conv_block1 = ConvBlock(1, 64)
            self.conv_block2 = ConvBlock(64, 128)
            self.conv_block3 = ConvBlock(128, 256)
            self.conv_block4 = ConvBlock(256, 512)
        self._natives = _HandleCache(self)
        self.precision = 'winograd'
        self.pipelined = False
        self.tuning = {}           # sedx_set_tuning knob -> value, applied to every handle

    def _config(self):
        cfg = _lib.SedxConfig()
        cfg.model_type = MODEL_IDS[self._model_name]
        if self.feature_type not in FEATURE_IDS:
            raise ValueError('feature_type %r not supported (logmel | gamma)' % self.feature_type)
        cfg.feature_type = FEATURE_IDS[self.feature_type]
        cfg.sample_rate = int(self.sample_rate)
        cfg.window_size = int(self.window_size)
        cfg.hop_size = int(self.hop_size)
        cfg.mel_bins = int(self.mel_bins)
        cfg.fmin = float(self.fmin)
        cfg.fmax = float(self.fmax if self.fmax is not None else self.sample_rate // 2)
        cfg.classes_num = int(self.classes_num)
        return cfg

    def _signature(self):
        """What the packed weights of a handle were made from: every
        state_dict tensor's key, shape, storage and version counter (an
        in-place update — load_state_dict, optimizer-free edits — bumps the
        version).  The state_dict walk (~75 tensors, ~0.1-0.2 ms of Python per
        call) runs again only when a parameter, buffer or submodule was
        registered anywhere since (torch's global registration hooks bump
        _REG_GEN); otherwise the cached tensor list is re-read for storage and
        version only, so a one-clip forward does not wait on it."""
        # (keyed on the object too: a DataParallel replica is a shallow
        # __dict__ copy whose parameter dicts are replaced without
        # registration, so it must not reuse its source's cache)
        c = self.__dict__.get('_sig_cache')
        if c is None or c[0] != _REG_GEN[0] or c[1] != id(self):
            sd = self.state_dict(keep_vars=True)
            c = (_REG_GEN[0], id(self), tuple(sd.keys()), tuple(sd.values()),
                 tuple(tuple(v.shape) for v in sd.values()))
            self.__dict__['_sig_cache'] = c
        _, _, keys, tensors, shapes = c
        return keys, shapes, tuple([(t.data_ptr(), t._version) for t in tensors])

    def _weights_source(self):
        """The module whose parameters a handle is packed from: the source
        module for a DataParallel replica (its own parameters are broadcast
        copies of the source's, re-made every call), else the module itself."""
        if getattr(self, '_is_replica', False):
            ref = getattr(self._natives, 'source', None)
            src = ref() if ref is not None else None
            if src is not None:
                return src
        return self

    def native(self, device):
        """The libsedx handle for ``device`` with the current weights packed."""
        if device.type != 'cuda':
            raise RuntimeError('sedx runs on HIP devices only (got a %s tensor); there is no CPU '
                               'fallback' % device.type)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._natives.lock:
            return self._native_locked(idx)

    def _native_locked(self, idx):
        nat = self._natives.get(idx)
        if nat is None:
            nat = _Native(self._config(), idx)
            self._natives[idx] = nat
        src = self._weights_source()
        sig = src._signature()
        if nat.signature != sig:
            nat.load(src.state_dict())
            nat.signature = sig
        if nat.precision != self.precision:
            _lib.check(_lib.lib().sedx_set_precision(nat.h, _lib.PRECISION[self.precision]), nat.h,
                       'set_precision')
            nat.precision = self.precision
        for knob, value in self.tuning.items():
            if getattr(nat, 'tuning', {}).get(knob) != value:
                _lib.check(_lib.lib().sedx_set_tuning(nat.h, knob, value), nat.h, 'set_tuning')
                nat.tuning = dict(getattr(nat, 'tuning', {}))
                nat.tuning[knob] = value
        if getattr(nat, 'pipelined', False) != self.pipelined:
            _lib.check(_lib.lib().sedx_set_pipelined(nat.h, int(self.pipelined)), nat.h, 'set_pipelined')
            nat.pipelined = self.pipelined
        return nat

    def set_precision(self, mode):
        """GEMM arithmetic (conv stack, GRU / MHA projections and recurrence,
        AttBlock projection): 'winograd' (default; fp32 operands, transforms
        and accumulation, block 1's conv2 and blocks 2-4 as Winograd
        F(4x4,3x3) — _lib.TUNE_WINO_F43 0 / 1 select F(2x2,3x3) in every layer
        / in block 1 only; error vs float64 max <= 2.5e-5, rms <= 1.7e-6 per
        layer), 'exact'
        (fp32 direct convolution, the reference's operation order), 'x3'
        (opt-in; 3xbf16-split MFMA, fp32 accumulate, ~1e-6 from fp32) or 'f16'
        (opt-in, reduced precision: the packed 3x3 conv layers with both
        operands rounded to fp16 on the f16 matrix pipe, fp32 accumulation and
        epilogue, everything else as 'exact'; outputs move by ~5e-5 on
        synthetic weights — include/sedx.h, SEDX_PRECISION_F16)."""
        if mode not in _lib.PRECISION:
            raise ValueError('precision must be one of %s' % sorted(_lib.PRECISION))
        self.precision = mode
        return self

    def set_tuning(self, knob, value):
        """An implementation choice of the library (sedx_set_tuning: _lib.TUNE_*)."""
        self.tuning[int(knob)] = int(value)
        return self

    def set_pipelined(self, on=True):
        """Several batches in flight on different streams: run the conv
        stacks in issue order so one batch's GRU / MHA + head overlap the next
        batch's conv stack (sedx_set_pipelined).  on = 2: also issue block 1's
        conv1 ahead of that wait."""
        self.pipelined = int(on) if on in (0, 1, 2) else bool(on)
        return self

    def check_error(self):
        """Raise if an earlier forward failed asynchronously (a GRU hand-off
        spin ran out: its outputs are NaN; sedx_check_error).  Call once the
        outputs in question are complete (after a sync or a copy to the
        host); the drivers in sedx.inference call it after every batch they
        copy back."""
        L = _lib.lib()
        for nat in list(self._natives.values()):
            _lib.check(L.sedx_check_error(nat.h), nat.h, 'asynchronous GRU failure')

    def _check_eval(self, mixup_lambda, timeshift):
        if self.training:
            raise RuntimeError('sedx models are inference-only: call model.eval() first '
                               '(training-mode SpecAugment/mixup/timeshift are out of scope)')
        if mixup_lambda is not None or timeshift:
            pass  # ignored in eval, as in the reference (models.py:647-661)

    def output_geometry(self, length):
        L = _lib.lib()
        with self._natives.lock:
            nat = self._natives.get(next(iter(self._natives))) if self._natives else None
            if nat is None:
                nat = _Native(self._config(), torch.cuda.current_device() if torch.cuda.is_available() else 0)
                self._natives[nat.device_index] = nat
        fr, sl = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.sedx_output_geometry(nat.h, int(length), ctypes.byref(fr), ctypes.byref(sl)),
                   nat.h, 'output_geometry')
        return fr.value, sl.value

    def forward(self, input, mixup_lambda=None, timeshift=False, spec_augment=True):
        """Input: (batch_size, data_length) waveform [logmel] or
        (batch_size, 64, frames) features [gamma].  Eval mode only.  An int16
        waveform (the reference's HDF5 packing) is dequantised x / 32767 inside
        the frontend (int16_to_float32, utils/utilities.py:78-79)."""
        self._check_eval(mixup_lambda, timeshift)
        if not isinstance(input, torch.Tensor) or input.device.type != 'cuda':
            raise RuntimeError('sedx forward needs a tensor on a HIP device (no CPU fallback)')
        i16 = input.dtype == torch.int16 and self.feature_type != 'gamma'
        x = input.contiguous() if i16 else input.to(torch.float32).contiguous()
        nat = self.native(x.device)
        L = _lib.lib()
        if self.feature_type == 'gamma':
            if x.dim() != 3 or x.shape[1] != 64:
                raise ValueError('gamma input must be (batch, 64, frames)')
            B, length = x.shape[0], x.shape[2]
        else:
            if x.dim() != 2:
                raise ValueError('input must be (batch_size, data_length)')
            B, length = x.shape
        fr, sl = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.sedx_output_geometry(nat.h, length, ctypes.byref(fr), ctypes.byref(sl)),
                   nat.h, 'output_geometry')
        C = self.classes_num
        dev = x.device
        fw = torch.empty((B, fr.value, C), dtype=torch.float32, device=dev)
        clip = torch.empty((B, C), dtype=torch.float32, device=dev)
        emb_shape = (B, C, sl.value) if self._embedding_cla else (B, self._embedding_width, sl.value)
        emb = torch.empty(emb_shape, dtype=torch.float32, device=dev) if self._has_embedding else None
        wsz = ctypes.c_size_t()
        _lib.check(L.sedx_workspace_size(nat.h, B, length, ctypes.byref(wsz)), nat.h, 'workspace_size')
        ws = torch.empty(wsz.value, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        fn = L.sedx_forward_features if self.feature_type == 'gamma' else (
            L.sedx_forward_i16 if i16 else L.sedx_forward)
        _lib.check(fn(nat.h, _ptr(x), B, length, _ptr(fw), _ptr(clip), _ptr(emb), _ptr(ws),
                      wsz.value, stream), nat.h, 'forward')
        if emb is None:
            return {'framewise_output': fw, 'clipwise_output': clip}
        return {'framewise_output': fw, 'clipwise_output': clip, 'embedding': emb}

    def forward_audio(self, wave):
        """The forward from a (batch_size, data_length) float waveform,
        whatever the model's features (sedx_forward_audio): ``forward(wave)``
        on a log-mel model; on a gamma model the gammatone frontend runs
        inside the forward (clips already pad_truncate'd, as for
        ``inference.gamma_features``) and the outputs equal
        ``forward(gamma_features(model, wave))`` bit for bit.  Eval mode only."""
        self._check_eval(None, False)
        if not isinstance(wave, torch.Tensor) or wave.device.type != 'cuda':
            raise RuntimeError('sedx forward needs a tensor on a HIP device (no CPU fallback)')
        if self.feature_type != 'gamma':
            return self.forward(wave)
        x = wave.to(torch.float32).contiguous()
        if x.dim() != 2:
            raise ValueError('input must be (batch_size, data_length)')
        nat = self.native(x.device)
        L = _lib.lib()
        B, length = x.shape
        fr, sl = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.sedx_audio_geometry(nat.h, length, None, ctypes.byref(fr), ctypes.byref(sl)),
                   nat.h, 'audio_geometry')
        C = self.classes_num
        dev = x.device
        fw = torch.empty((B, fr.value, C), dtype=torch.float32, device=dev)
        clip = torch.empty((B, C), dtype=torch.float32, device=dev)
        emb_shape = (B, C, sl.value) if self._embedding_cla else (B, self._embedding_width, sl.value)
        emb = torch.empty(emb_shape, dtype=torch.float32, device=dev) if self._has_embedding else None
        wsz = ctypes.c_size_t()
        _lib.check(L.sedx_audio_workspace_size(nat.h, B, length, ctypes.byref(wsz)), nat.h, 'audio_workspace_size')
        ws = torch.empty(wsz.value, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(L.sedx_forward_audio(nat.h, _ptr(x), B, length, _ptr(fw), _ptr(clip), _ptr(emb), _ptr(ws),
                                        wsz.value, stream), nat.h, 'forward_audio')
        if emb is None:
            return {'framewise_output': fw, 'clipwise_output': clip}
        return {'framewise_output': fw, 'clipwise_output': clip, 'embedding': emb}


class Cnn_9layers_Gru_FrameAtt(_SedModel):
    """pytorch/models.py:564-688."""
    _model_name = 'Cnn_9layers_Gru_FrameAtt'
    _embedding_cla = True

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         feature_type)
        self.gru = nn.GRU(input_size=512, hidden_size=256, num_layers=1, bias=True,
                          batch_first=True, bidirectional=True)
        self.att_block = AttBlock(n_in=512, n_out=classes_num, activation='sigmoid')
        init_bn(self.bn0)
        init_gru(self.gru)


class Cnn_9layers_Gru_Reg(_SedModel):
    """pytorch/models.py:2788-2889: ``Cnn_9layers_Gru_FrameAtt`` with
    ``AttBlock(512, 25)`` -- 25 classes whatever ``classes_num`` is (:2827) --
    and without ``pad_framewise_output`` (:2882): the framewise output is the
    ``8 * (T // 8)`` interpolated frames (7777 samples: 48, where
    ``Cnn_9layers_Gru_FrameAtt`` pads to 100).  ``forward(input,
    mixup_lambda=None, timeshift=False)``; embedding = cla (batch, 25, seq)."""
    _model_name = 'Cnn_9layers_Gru_Reg'
    _embedding_cla = True

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, 25, feature_type)
        self.gru = nn.GRU(input_size=512, hidden_size=256, num_layers=1, bias=True,
                          batch_first=True, bidirectional=True)
        self.att_block = AttBlock(n_in=512, n_out=25, activation='sigmoid')
        init_bn(self.bn0)
        init_gru(self.gru)

    def forward(self, input, mixup_lambda=None, timeshift=False):
        return super().forward(input, mixup_lambda=mixup_lambda, timeshift=timeshift)


class Cnn_9layers_Transformer_FrameAtt(_SedModel):
    """pytorch/models.py:981-1077 (always logmel: the reference has no
    feature-type branch)."""
    _model_name = 'Cnn_9layers_Transformer_FrameAtt'

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type='logmel'):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         'logmel')
        self.multihead = MultiHead(8, 512, 64, 64, 0.2)
        self.att_block = AttBlock(n_in=512, n_out=classes_num, activation='sigmoid')
        init_bn(self.bn0)


class _CnnOnlyModel(_SedModel):
    """The CNN-only classes: seven constructor arguments (no feature_type,
    always logmel) and ``forward(input, mixup_lambda=None)``
    (models.py:214-215, :255)."""

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         'logmel')

    def forward(self, input, mixup_lambda=None):
        return super().forward(input, mixup_lambda=mixup_lambda)


class Cnn_9layers_FrameMax(_CnnOnlyModel):
    """pytorch/models.py:213-295: sigmoid(fc) per frame, clipwise = max over
    the frames; embedding = block 4's frequency mean."""
    _model_name = 'Cnn_9layers_FrameMax'

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num)
        self.fc = nn.Linear(512, classes_num, bias=True)
        init_bn(self.bn0)
        init_layer(self.fc)


class Cnn_9layers_FrameAvg(_CnnOnlyModel):
    """pytorch/models.py:298-380: as FrameMax with clipwise = mean over the frames."""
    _model_name = 'Cnn_9layers_FrameAvg'

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num)
        self.fc = nn.Linear(512, classes_num, bias=True)
        init_bn(self.bn0)
        init_layer(self.fc)


class Cnn_9layers_FrameAtt(_CnnOnlyModel):
    """pytorch/models.py:383-461.  The reference builds ``AttBlock(n_out=25)``
    whatever ``classes_num`` is (:416), so the model has 25 classes: the
    state_dict, the native handle and the outputs are 25-class, and
    ``classes_num`` reads 25."""
    _model_name = 'Cnn_9layers_FrameAtt'
    _embedding_cla = True

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, 25)
        self.att_block = AttBlock(n_in=512, n_out=25, activation='sigmoid')
        init_bn(self.bn0)


class Cnn_9layers_Gru_FrameAvg(_SedModel):
    """pytorch/models.py:466-561: bi-GRU, sigmoid(fc), mean; the framewise
    output is the 8 * seq_len frames (no padding to a multiple of 100, :551).
    ``feature_type`` is accepted and ignored, as in the reference (:512-518:
    no gamma branch)."""
    _model_name = 'Cnn_9layers_Gru_FrameAvg'

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         'logmel')
        self.gru = nn.GRU(input_size=512, hidden_size=256, num_layers=1, bias=True,
                          batch_first=True, bidirectional=True)
        self.fc = nn.Linear(512, classes_num, bias=True)
        init_bn(self.bn0)
        init_gru(self.gru)
        init_layer(self.fc)


class Cnn_9layers_Transformer_FrameAvg(_SedModel):
    """pytorch/models.py:880-978: MultiHead, sigmoid(fc), mean (always logmel)."""
    _model_name = 'Cnn_9layers_Transformer_FrameAvg'

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         'logmel')
        self.multihead = MultiHead(8, 512, 64, 64, 0.2)
        self.fc = nn.Linear(512, classes_num, bias=True)
        init_bn(self.bn0)
        init_layer(self.fc)


class _ConformerModel(_SedModel):
    """The two Conformer classes (pytorch/models.py:1189-1300, :1412-1515):
    the reference constructor and ``forward(x, mixup_lambda=None,
    timeshift=False, spec_augment=True, mask=None)``; always logmel.  The
    encoder and the 144-wide head run fp32 in every precision mode.  The
    sequence holds at most 5000 frames (the ``pe`` table)."""
    _embedding_width = 144
    _head_classes = None       # the handle's class count when it is not classes_num
    _trunk_width = 512         # the encoder's input: 2048 on the 14-layer trunk (conv_block5, conv_block6)

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 cnn_kwargs=None, encoder_kwargs=None, encoder_type='Conformer', pooling='token',
                 layer_init='pytorch'):
        if encoder_type == 'Transformer':
            raise ValueError('encoder_type="Transformer" (models_2020/transformer) is not implemented natively; '
                             'only the Conformer encoder is')
        if encoder_type != 'Conformer':
            raise ValueError("Choose encoder_type in ['Transformer', 'Conformer']")
        if pooling != 'token':
            raise ValueError('pooling=%r: the reference forward uses none of its pooling branches, and only '
                             'the default module tree (pooling="token") is mirrored' % (pooling,))
        if layer_init.lower() != 'pytorch':
            raise ValueError('layer_init=%r: load a state_dict instead (inference-only model)' % (layer_init,))
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax,
                         self._head_classes or classes_num, 'logmel')
        self.pooling = pooling
        self.encoder_kwargs = {'adim': 144, 'aheads': 4, 'dropout_rate': 0.1, 'elayers': 3, 'eunits': 576,
                               'kernel_size': 7}
        if self._trunk_width == 2048:
            self.conv_block5 = ConvBlock(512, 1024)
            self.conv_block6 = ConvBlock(1024, 2048)
        self.encoder = ConformerEncoder(self._trunk_width, **self.encoder_kwargs)
        self._build_head(classes_num)
        # unused in the forward of the FrameAtt / FrameAvg classes (models.py:1290, :1505, :1727); the head and
        # the tag token of Cnn_9layers_Conformer (:2115, :2123)
        self.classifier = nn.Linear(144, classes_num)
        self.linear_emb = nn.Linear(1, self._trunk_width)

    def forward(self, x, mixup_lambda=None, timeshift=False, spec_augment=True, mask=None):
        if mask is not None:
            raise ValueError('mask must be None: the native encoder implements the unmasked forward')
        return super().forward(x, mixup_lambda=mixup_lambda, timeshift=timeshift, spec_augment=spec_augment)


class Cnn_9layers_Conformer_FrameAtt(_ConformerModel):
    """pytorch/models.py:1189-1410: trunk, Conformer encoder, ``AttBlock(144,
    25)`` -- 25 classes whatever ``classes_num`` is (:1288), like
    ``Cnn_9layers_FrameAtt``; framewise padded to a multiple of 100 with its
    last frame; embedding = the encoder output (batch, 144, seq)."""
    _model_name = 'Cnn_9layers_Conformer_FrameAtt'
    _head_classes = 25

    def _build_head(self, classes_num):
        self.att_block = AttBlock(n_in=144, n_out=25, activation='sigmoid')


class Cnn_9layers_Conformer_FrameAvg(_ConformerModel):
    """pytorch/models.py:1412-1625: trunk, Conformer encoder, sigmoid(fc);
    framewise padded to a multiple of 100 with its last frame, clipwise = the
    mean over the padded frames (:1575)."""
    _model_name = 'Cnn_9layers_Conformer_FrameAvg'

    def _build_head(self, classes_num):
        self.fc = nn.Linear(144, classes_num, bias=True)


class Cnn_9layers_Conformer(_ConformerModel):
    """pytorch/models.py:2019-2214, the DCASE-2020-style token model.  Block 4 is
    not pooled and its 8 frequency bins are kept: every (frame, bin) pixel is a
    512-wide token, in (t, f) order, behind the tag token ``linear_emb(ones)``;
    the Conformer encoder runs on those ``8 * (T // 8) + 1`` tokens (1001 for a
    10 s clip) and ``classifier = Linear(144, classes_num)`` reads both outputs off
    them: ``clipwise_output`` (batch, classes) is token 0, ``framewise_output``
    (batch, 8 * (T // 8), classes) the others.  Both are LOGITS (no sigmoid, no
    interpolation, no padding) and there is no ``'embedding'``, as in the
    reference.  ``cnn_kwargs`` and ``encoder_kwargs`` are accepted and ignored
    (the reference overwrites both).  ``forward(x, mixup_lambda=None,
    timeshift=False, mask=None)``: no ``spec_augment`` argument, ``mask`` must be
    ``None``.  Fewer than 8 input frames and more than 5000 tokens raise.  The
    encoder and the classifier run fp32 in every precision mode."""
    _model_name = 'Cnn_9layers_Conformer'
    _has_embedding = False

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 cnn_kwargs=None, encoder_kwargs=None, encoder_type='Conformer', pooling='token',
                 layer_init='pytorch'):
        if encoder_type != 'Conformer':
            raise ValueError('encoder_type=%r: only encoder_type="Conformer" is implemented natively' % (encoder_type,))
        if pooling != 'token':
            raise ValueError('pooling=%r: only pooling="token" (the tag token and the token head) is implemented '
                             'natively' % (pooling,))
        if str(layer_init).lower() != 'pytorch':
            raise ValueError('layer_init=%r: only layer_init="pytorch" is supported; load a state_dict instead '
                             '(inference-only model)' % (layer_init,))
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         cnn_kwargs=cnn_kwargs, encoder_kwargs=encoder_kwargs)

    def _build_head(self, classes_num):
        pass   # classifier, built by the base class at the constructor's class count

    def forward(self, x, mixup_lambda=None, timeshift=False, mask=None):
        return super().forward(x, mixup_lambda=mixup_lambda, timeshift=timeshift, mask=mask)


class Cnn_14layers_Conformer_FrameAtt(_ConformerModel):
    """pytorch/models.py:1627-1801: the 14-layer trunk (blocks 1-5 pooled 2x2,
    block 6's frequency mean: ``data_length // hop // 32`` sequence frames of
    2048 channels), ``ConformerEncoder(2048, 144, ...)``, ``AttBlock(144, 25)``
    -- 25 classes whatever ``classes_num`` is (:1725).  ``feature_type`` is
    accepted and ignored (always logmel).  Every sequence frame is repeated
    ``1000 // seq_len`` times; unless that gives 1000 frames the last one is
    repeated up to the next multiple of 100 (10 s: 31 x 32 = 992 -> 1000; a 5 s
    window: 15 x 66 = 990 -> 1000).  Fewer than 32 input frames raise as in the
    reference; more than 1000 sequence frames raise (the reference returns an
    empty framewise tensor).  embedding = the encoder output (batch, 144,
    seq).  Block 4's conv2, blocks 5-6, the encoder and the head run fp32 in
    every precision mode."""
    _model_name = 'Cnn_14layers_Conformer_FrameAtt'
    _head_classes = 25
    _trunk_width = 2048

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num, feature_type,
                 cnn_kwargs=None, encoder_kwargs=None, encoder_type='Conformer', pooling='token',
                 layer_init='pytorch'):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         cnn_kwargs=cnn_kwargs, encoder_kwargs=encoder_kwargs, encoder_type=encoder_type,
                         pooling=pooling, layer_init=layer_init)

    def _build_head(self, classes_num):
        self.att_block = AttBlock(n_in=144, n_out=25, activation='sigmoid')


class _Deep14Model(_SedModel):
    """The 14-layer trunk (pytorch/models.py:720-725, :1109-1114): blocks 1-4,
    then ``conv_block5`` (512 -> 1024) and ``conv_block6`` (1024 -> 2048), five
    2x2 pools: ``data_length // hop // 32`` sequence frames of 2048 channels,
    x32 frame repeat, framewise padded to a multiple of 100 with its last frame
    unless it has 1000 frames.  ``AttBlock(2048, 25)``: 25 classes whatever
    ``classes_num`` is (:730, :1123).  ``feature_type`` is accepted and ignored,
    as the reference's forward ignores it (always logmel).  Block 4's conv2,
    blocks 5-6, the sequence layer and the head run fp32 in every precision
    mode; ``set_precision`` selects blocks 1-3 and block 4's conv1."""
    _embedding_width = 2048

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, 25, 'logmel')
        self.conv_block5 = ConvBlock(512, 1024)
        self.conv_block6 = ConvBlock(1024, 2048)


class Cnn_14layers_Gru_FrameAtt(_Deep14Model):
    """pytorch/models.py:691-791: ``nn.GRU(2048, 1024, bidirectional)``;
    embedding = cla (batch, 25, seq)."""
    _model_name = 'Cnn_14layers_Gru_FrameAtt'
    _embedding_cla = True

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         feature_type)
        self.gru = nn.GRU(input_size=2048, hidden_size=1024, num_layers=1, bias=True,
                          batch_first=True, bidirectional=True)
        self.att_block = AttBlock(n_in=2048, n_out=25, activation='sigmoid')
        init_bn(self.bn0)
        init_gru(self.gru)


class Cnn_14layers_Transformer_FrameAtt(_Deep14Model):
    """pytorch/models.py:1080-1184: ``MultiHead(8, 2048, 64, 64)``; embedding =
    its output (batch, 2048, seq)."""
    _model_name = 'Cnn_14layers_Transformer_FrameAtt'

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                 feature_type):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         feature_type)
        self.multihead = MultiHead(8, 2048, 64, 64, 0.2)
        self.att_block = AttBlock(n_in=2048, n_out=25, activation='sigmoid')
        init_bn(self.bn0)


class Cnn14_DecisionLevelAtt(_SedModel):
    """pytorch/models.py:2685-2783, the PANNs architecture: the 14-layer trunk,
    ``max_pool1d(3, 1, 1) + avg_pool1d(3, 1, 1)`` over the
    ``data_length // hop // 32`` sequence frames, ``fc1 = Linear(2048, 2048)`` +
    ReLU and ``AttBlock(2048, classes_num)`` at the constructor's class count
    (up to 527: AudioSet at 32 kHz is ``(32000, 1024, 320, 64, 50, 14000,
    527)``).  Seven constructor arguments (always logmel) and
    ``forward(input, mixup_lambda=None)`` returning ``framewise_output``
    (batch, T - 1, classes: every sequence frame x32, then the last frame
    repeated) and ``clipwise_output`` only.  An input of fewer than 32 frames, or
    of a multiple of 32 frames (``T = data_length // hop + 1``), raises as the
    reference does.  Block 4's conv2, blocks 5-6, the pooling, ``fc1`` and the
    head run fp32 in every precision mode."""
    _model_name = 'Cnn14_DecisionLevelAtt'
    _has_embedding = False

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num,
                         'logmel')
        self.conv_block5 = ConvBlock(512, 1024)
        self.conv_block6 = ConvBlock(1024, 2048)
        self.fc1 = nn.Linear(2048, 2048, bias=True)
        self.att_block = AttBlock(n_in=2048, n_out=classes_num, activation='sigmoid')
        init_bn(self.bn0)
        init_layer(self.fc1)

    def forward(self, input, mixup_lambda=None):
        return super().forward(input, mixup_lambda=mixup_lambda)


class VGGish(nn.Module):
    """pytorch/models.py:2219-2267 (weights only): ``features`` is the conv
    trunk, six 3x3 convs with bias and ReLU and four 2x2 max pools; ``fc`` is the
    embedding stack that the three models below drop.  A fresh instance holds
    the 290 MB of ``fc`` weights a VGGish checkpoint holds."""

    def __init__(self):
        super().__init__()
        self.features = _vggish_features()
        self.fc = nn.Sequential(
            nn.Linear(512 * 24, 4096), nn.ReLU(inplace=True),
            nn.Linear(4096, 4096), nn.ReLU(inplace=True),
            nn.Linear(4096, 128), nn.ReLU(inplace=True))

    def forward(self, x):
        raise RuntimeError('VGGish is a parameter container: its trunk runs inside the native model forward')


def _vggish_features():
    """VGGish.features (models.py:2230-2250): the Sequential indices 0, 3, 6, 8,
    11 and 13 are the convs."""
    return nn.Sequential(
        nn.Conv2d(1, 64, 3, stride=1, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(2, stride=2),
        nn.Conv2d(64, 128, 3, stride=1, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(2, stride=2),
        nn.Conv2d(128, 256, 3, stride=1, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(256, 256, 3, stride=1, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(2, stride=2),
        nn.Conv2d(256, 512, 3, stride=1, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(512, 512, 3, stride=1, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(2, stride=2))


class _VGGishModel(_SedModel):
    """The three transfer-learning classes (pytorch/models.py:2284-2592): the
    reference's ten constructor arguments and ``forward(input,
    mixup_lambda=None, timeshift=False, spec_augment=True)``.  The trunk is
    ``VGGish.features`` on the raw log-mel (``bn0`` is in the state_dict and is
    never applied), four flooring 2x2 max pools: ``T // 16`` sequence frames of
    512 channels for ``T = data_length // hop + 1``.  The head has 25 outputs
    whatever ``classes_num`` is (:2323, :2425, :2526) and ``feature_type`` is
    ignored.  Every class builds ``nn.GRU(512, 256, bidirectional)``; only
    ``VGGish_Gru_FrameAtt`` calls it.  The framewise output always has 1000
    frames.  The trunk runs fp32 in every precision mode.

    ``checkpoint_path`` is loaded as the reference does (``init_weights``:
    ``torch.load`` of a full ``VGGish().state_dict()``, ``features.*`` kept as
    ``vggish.0.*``, ``fc.*`` dropped).  ``checkpoint_path=None`` skips the load
    (an extension, for callers that load a full state_dict afterwards).
    ``freeze`` sets ``requires_grad = False`` on the trunk's parameters."""
    _cnn9_trunk = False

    def __init__(self, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num, feature_type,
                 checkpoint_path, freeze=False):
        super().__init__(sample_rate, window_size, hop_size, mel_bins, fmin, fmax, 25, 'logmel')
        self.checkpoint_path = checkpoint_path
        self.freeze = freeze
        feature_sample_rate = 1.0 / (hop_size / sample_rate)
        self.example_window_length = int(round(0.96 * feature_sample_rate))
        self.example_hop_length = int(round(0.96 * feature_sample_rate))
        self.gru = nn.GRU(input_size=512, hidden_size=256, num_layers=1, bias=True,
                          batch_first=True, bidirectional=True)
        self.vggish = nn.Sequential(_vggish_features())   # keys vggish.0.<index>.*
        self._build_head()
        self.init_weights()

    def init_weights(self):
        init_bn(self.bn0)
        if self.checkpoint_path is not None:
            checkpoint = torch.load(self.checkpoint_path, map_location='cpu')
            full = {'features.' + k for k in self.vggish[0].state_dict()}
            missing = sorted(full - set(checkpoint))
            unexpected = sorted(k for k in checkpoint if k not in full and not k.startswith('fc.'))
            if missing or unexpected:   # VGGish().load_state_dict(checkpoint) is strict
                raise RuntimeError('VGGish checkpoint: missing keys %s, unexpected keys %s' % (missing, unexpected))
            self.vggish[0].load_state_dict({k[len('features.'):]: v for k, v in checkpoint.items()
                                            if k.startswith('features.')})
        if self.freeze:
            for param in self.vggish.parameters():
                param.requires_grad = False


class VGGish_FrameAtt(_VGGishModel):
    """pytorch/models.py:2284-2383: trunk, ``AttBlock(512, 25)``; every sequence
    frame x12, then the last frame up to 1000; embedding = cla (batch, 25, seq).
    16 <= T < 1344 (at most 83 sequence frames), as the reference."""
    _model_name = 'VGGish_FrameAtt'
    _embedding_cla = True

    def _build_head(self):
        self.att_block = AttBlock(n_in=512, n_out=25, activation='sigmoid')


class VGGish_Gru_FrameAtt(_VGGishModel):
    """pytorch/models.py:2386-2485: as ``VGGish_FrameAtt`` with the bi-GRU between
    the trunk and the head."""
    _model_name = 'VGGish_Gru_FrameAtt'
    _embedding_cla = True

    def _build_head(self):
        self.att_block = AttBlock(n_in=512, n_out=25, activation='sigmoid')


class VGGish_FrameAvg(_VGGishModel):
    """pytorch/models.py:2487-2592: trunk, ``sigmoid(Linear(512, 25))``; every
    sequence frame x(1000 // seq), then the last frame up to 1000; clipwise = the
    mean over the 1000 padded frames; embedding = the trunk's output (batch, 512,
    seq).  Up to 1000 sequence frames (beyond, the reference returns an empty
    tensor and NaN; this class raises)."""
    _model_name = 'VGGish_FrameAvg'

    def _build_head(self):
        self.fc = nn.Linear(512, 25, bias=True)
