"""CPU-only checks of the two Conformer models (Cnn_9layers_Conformer_FrameAtt,
_FrameAvg): the torch restatement (tests/conformer_refs.py) against the
goldens the reference produced (tools/make_golden_conformer.py), the closed
form of the relative shift, the mirror classes' state_dict, the synthetic
weights, and what sedx_create / sedx_load_param / sedx_output_geometry accept.
No GPU work: creation, load_param and the geometry query are host-only."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import conformer_refs as CR
from sedx import synth

TOL = 1e-3          # the project's bar against the reference (tests/test_gpu_parity.py)
MODEL_IDS = [CR.IDS[mt] for mt in CR.MODELS]
EINVAL, EKEY = 1, 5


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


def _waves(kind):
    if kind == 'short':
        return synth.make_waveforms(2, seconds=5280 / 16000., sample_rate=16000, seed=11)
    if kind == 'ragged':
        return synth.make_waveforms(1, seconds=7777 / 16000., sample_rate=16000, seed=12)
    return synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', CR.MODELS, ids=MODEL_IDS)
def test_restatement_matches_goldens(mt, golden_dir):
    """Outputs of the three inputs and the 13 encoder activations of ``short``."""
    g = np.load(os.path.join(golden_dir, 'conformer_%s.npz' % mt))
    sd = CR.full_state(mt)
    for kind in ('short', 'ragged', 'clip10s'):
        out, acts = CR.forward(sd, mt, wave=_waves(kind), return_acts=True)
        for k in CR.KEYS:
            ref = g['%s_%s' % (kind, k)]
            got = out[k].numpy()[:1] if kind == 'clip10s' else out[k].numpy()
            e = err(got, ref)
            print(mt, kind, k, ref.shape, 'max|d| = %.3g' % e)
            assert e <= TOL
        if kind == 'short':
            assert g['short_framewise_output'].shape == (2, 100, 25)
            assert g['short_embedding'].shape == (2, 144, 4)
            e = err(acts['cnn_out'].numpy(), g['short_cnn_out'])
            print(mt, 'cnn_out max|d| = %.3g' % e)
            assert e <= TOL
            for i in CR.ACT_IDS:
                e = err(acts[i].numpy(), g['short_act_%d' % i])
                print(mt, 'act', i, 'max|d| = %.3g' % e)
                assert e <= TOL
        if kind == 'ragged':
            assert g['ragged_framewise_output'].shape == (1, 100, 25) and g['ragged_embedding'].shape == (1, 144, 6)
        if kind == 'clip10s':
            assert g['clip10s_framewise_output'].shape == (1, 1000, 25)
            assert g['clip10s_embedding'].shape == (1, 144, 125)


@pytest.mark.parametrize('T', [1, 2, 3, 9])
def test_closed_form_shift_equals_pad_and_view(T):
    x = torch.from_numpy(np.random.default_rng(T).standard_normal((T, T)))
    a, b = CR.rel_shift(x), CR.rel_shift_pad_view(x)
    assert torch.equal(a, b)
    if T >= 2:
        assert float(a[0, 1]) == 0.0                      # j = i + 1
    if T >= 3:
        assert float(a[0, 2]) == float(x[1, 0])           # j >= i + 2 reads the next query's row
    assert float(a[T - 1, 0]) == float(x[T - 1, 0])       # the last row is not shifted
    batched = CR.rel_shift(x[None, None].repeat(2, 3, 1, 1))
    assert torch.equal(batched[1, 2], b)


def test_restatement_float64_agrees_with_float32():
    w = _waves('short')
    for mt in CR.MODELS:
        s32 = CR.full_state(mt)
        s64 = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
               for k, v in s32.items()}
        with torch.no_grad():
            x32, _ = CR.O.cnn(s32, CR.O.logmel(s32, torch.from_numpy(w)))
            a32, a64 = {}, {}
            o32 = CR.head(s32, mt, CR.encoder(s32, x32.transpose(1, 2), a32))
            o64 = CR.head(s64, mt, CR.encoder(s64, x32.double().transpose(1, 2), a64))
        for i in CR.ACT_IDS:
            assert a64[i].dtype == torch.float64
            e = err(a32[i].numpy(), a64[i].numpy())
            assert e <= 1e-5 * max(1.0, float(a64[i].abs().max())), (mt, i, e)
        for k in CR.KEYS:
            assert o64[k].dtype == torch.float64
            assert err(o32[k].numpy(), o64[k].numpy()) <= 1e-5 * max(1.0, float(o64[k].abs().max())), (mt, k)


def test_frameavg_clipwise_is_the_mean_over_the_padded_frames():
    sd = CR.state(CR.CAVG, dtype=torch.float64)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 4, 144)))
    o = CR.head(sd, CR.CAVG, x)
    fw = o['framewise_output']
    assert fw.shape == (1, 100, 25)
    assert torch.equal(fw[:, 32:], fw[:, 31:32].expand(1, 68, 25))
    assert torch.allclose(o['clipwise_output'], fw.mean(dim=1), rtol=0, atol=1e-15)
    assert not torch.allclose(o['clipwise_output'], fw[:, :32].mean(dim=1), rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------
# mirror classes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', CR.MODELS, ids=MODEL_IDS)
def test_state_dict_equals_the_reference(mt, golden_dir):
    from sedx import models
    meta = json.load(open(os.path.join(golden_dir, 'conformer_meta.json')))[mt]
    assert (meta['entries'], meta['elements']) == {CR.CATT: (179, 7285220), CR.CAVG: (172, 7281494)}[mt]
    sd = getattr(models, mt)(*CR.P16, 25).state_dict()
    got = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()]
    assert got == meta['keys']
    assert sum(v.numel() for v in sd.values()) == meta['elements']
    assert torch.equal(sd['encoder.input_layer.4.pe'], CR.pe_table())
    assert torch.equal(sd['encoder.conformer_blocks.2.mhsa.pos_emb.inv_freq'], CR.inv_freq())


def test_constructor_forward_and_errors():
    from sedx import models
    for mt in CR.MODELS:
        cls = getattr(models, mt)
        assert list(inspect.signature(cls.__init__).parameters)[1:] == [
            'sample_rate', 'window_size', 'hop_size', 'mel_bins', 'fmin', 'fmax', 'classes_num', 'cnn_kwargs',
            'encoder_kwargs', 'encoder_type', 'pooling', 'layer_init']
        assert list(inspect.signature(cls.forward).parameters)[1:] == [
            'x', 'mixup_lambda', 'timeshift', 'spec_augment', 'mask']
        with pytest.raises(ValueError, match='Transformer'):
            cls(*CR.P16, 25, encoder_type='Transformer')
        with pytest.raises(ValueError, match='pooling'):
            cls(*CR.P16, 25, pooling='attention')
        m = cls(*CR.P16, 25).eval()
        with pytest.raises(ValueError, match='mask'):
            m(torch.zeros(1, 5280), mask=torch.ones(1, 4, 4))
        with pytest.raises(RuntimeError, match='eval'):
            m.train()(torch.zeros(1, 5280))
        assert models.MODEL_IDS[mt] == {CR.CATT: 7, CR.CAVG: 8}[mt]
    m = models.Cnn_9layers_Conformer_FrameAtt(*CR.P16, 10)
    assert m.classes_num == 25 and tuple(m.state_dict()['att_block.cla.weight'].shape) == (25, 144, 1)
    assert tuple(m.state_dict()['classifier.weight'].shape) == (10, 144)
    m = models.Cnn_9layers_Conformer_FrameAvg(*CR.P16, 10)
    assert m.classes_num == 10 and tuple(m.state_dict()['fc.weight'].shape) == (10, 144)


# ---------------------------------------------------------------------------
# synth
# ---------------------------------------------------------------------------
def test_synth_weights():
    from sedx import models
    assert synth.CONFORMER_GOLDEN_SEEDS == {CR.CATT: 7, CR.CAVG: 8}
    assert synth.MODEL_PARTS[CR.CATT] == ('conformer', 'att') and synth.MODEL_PARTS[CR.CAVG] == ('conformer', 'fc')
    assert not set(synth.CONFORMER_GOLDEN_SEEDS) & set(synth.GOLDEN_SEEDS)
    for mt, C in ((CR.CATT, 25), (CR.CAVG, 25), (CR.CAVG, 7)):
        w = synth.make_state_dict(mt, classes_num=C, seed=3)
        m = getattr(models, mt)(*CR.P16, C)
        sd = m.state_dict()
        for k, v in w.items():
            sd[k] = torch.from_numpy(np.asarray(v))
        m.load_state_dict(sd, strict=True)
        # every tensor but the constant buffers is drawn, in state_dict order
        left = [k for k in m.state_dict() if k not in w]
        assert all(k.startswith(('spectrogram_extractor.', 'logmel_extractor.')) or k.endswith(('.pe', '.inv_freq'))
                   for k in left), left
        order = [k for k in m.state_dict() if k in w]
        assert order == list(w)
        for k, v in w.items():
            if k.endswith('num_batches_tracked'):
                continue
            assert np.unique(v).size > 1 or v.size == 1, k            # nothing left at a constant
        p = 'encoder.conformer_blocks.1.'
        for k in (p + 'mhsa.r_w_bias', p + 'mhsa.r_r_bias'):
            assert w[k].shape == (4, 36) and np.abs(w[k]).max() <= 0.1 and np.unique(w[k]).size > 100, k
        for k in (p + 'norm.weight', p + 'mhsa.layer_norm.weight', 'encoder.input_layer.1.weight',
                  p + 'ffn1.feed_forward_module.0.weight', p + 'conv.conv.0.weight'):
            assert 0.5 <= w[k].min() < w[k].max() <= 1.5 and np.unique(w[k]).size > 100, k
        assert np.abs(w[p + 'norm.bias']).max() <= 0.2 and np.unique(w[p + 'norm.bias']).size > 100
        assert np.unique(w[p + 'conv.conv.5.running_var']).size > 100
    # trunk first: the trunk tensors of one seed are the other models'
    a, b = synth.make_state_dict(CR.CATT, seed=9), synth.make_state_dict('Cnn_9layers_FrameAvg', seed=9)
    for k in b:
        if k.startswith(('bn0.', 'conv_block')):
            assert np.array_equal(a[k], b[k]), k
    c = synth.make_state_dict(CR.CAVG, seed=9)
    for k in a:
        if k.startswith('encoder.'):
            assert np.array_equal(a[k], c[k]), k


# ---------------------------------------------------------------------------
# sedx_create / sedx_load_param / sedx_output_geometry
# ---------------------------------------------------------------------------
def _cfg(model_type, feature_type=0, classes_num=25):
    from sedx import _lib
    c = _lib.SedxConfig()
    c.model_type, c.feature_type = model_type, feature_type
    c.sample_rate, c.window_size, c.hop_size, c.mel_bins = 16000, 512, 160, 64
    c.fmin, c.fmax, c.classes_num = 25.0, 7000.0, classes_num
    return c


def _create(model_type, feature_type=0):
    from sedx import _lib
    h = ctypes.c_void_p()
    st = _lib.lib().sedx_create(ctypes.byref(_cfg(model_type, feature_type)), 0, ctypes.byref(h))
    return st, h


def _load(h, key, shape):
    from sedx import _lib
    a = np.zeros(shape, np.float32)
    sh = (ctypes.c_int64 * a.ndim)(*a.shape)
    return _lib.lib().sedx_load_param(h, key.encode(), a.ctypes.data_as(ctypes.c_void_p), sh, a.ndim)


def test_create_accepts_7_and_8():
    from sedx import _lib
    L = _lib.lib()
    for mid in (7, 8):
        st, h = _create(mid)
        assert st == _lib.SEDX_OK and h.value
        L.sedx_destroy(h)
        st, h = _create(mid, feature_type=1)                 # gamma
        assert st == EINVAL and not h.value
    st, h = _create(9)
    assert st == EINVAL and not h.value
    assert L.sedx_abi_version() == 6


@pytest.mark.parametrize('mt', CR.MODELS, ids=MODEL_IDS)
def test_load_param_key_set(mt):
    from sedx import _lib, models
    L = _lib.lib()
    st, h = _create(models.MODEL_IDS[mt])
    assert st == _lib.SEDX_OK
    try:
        sd = getattr(models, mt)(*CR.P16, 25).state_dict()
        for k, v in sd.items():
            if k.endswith('num_batches_tracked'):
                continue
            assert _load(h, k, tuple(v.shape)) == _lib.SEDX_OK, k
        for k, shape in (('classifier.weight', (25, 144)), ('classifier.bias', (25,)), ('linear_emb.weight', (512, 1)),
                         ('linear_emb.bias', (512,))):
            assert _load(h, k, shape) == _lib.SEDX_OK, k
        if mt == CR.CATT:
            assert _load(h, 'att_block.bn_att.running_var', (25,)) == _lib.SEDX_OK
            assert _load(h, 'att_block.att.weight', (25, 512, 1)) == EKEY
            assert _load(h, 'fc.bias', (25,)) == EKEY
        else:
            assert _load(h, 'att_block.att.weight', (25, 144, 1)) == EKEY
        for k, shape in (('gru.weight_ih_l0', (768, 512)), ('multihead.w_qs.weight', (512, 512)),
                         ('fc.weight', (25, 512)), ('encoder.input_layer.4.pe', (1, 4999, 144)),
                         ('encoder.conformer_blocks.3.norm.weight', (144,))):
            assert _load(h, k, shape) == EKEY, k
            assert k.encode() in L.sedx_last_error(h)
    finally:
        L.sedx_destroy(h)
    # and the earlier models do not take the encoder's keys
    st, h = _create(models.MODEL_IDS['Cnn_9layers_FrameAvg'])
    try:
        assert _load(h, 'encoder.input_layer.0.weight', (144, 512)) == EKEY
        assert _load(h, 'classifier.weight', (25, 144)) == EKEY
    finally:
        L.sedx_destroy(h)


@pytest.mark.parametrize('mid', [7, 8])
def test_output_geometry(mid):
    from sedx import _lib
    L = _lib.lib()
    st, h = _create(mid)
    assert st == _lib.SEDX_OK
    try:
        fr, sl = ctypes.c_int64(), ctypes.c_int64()
        for length, want in ((5280, (100, 4)), (7777, (100, 6)), (160000, (1000, 125)), (16000 * 5, (500, 62)),
                             (160 * (8 * 5000 - 1), (40000, 5000))):
            assert L.sedx_output_geometry(h, length, ctypes.byref(fr), ctypes.byref(sl)) == _lib.SEDX_OK
            assert (fr.value, sl.value) == want, length
        too_long = 160 * (8 * 5001 - 1)                       # T = 40008 frames, T3 = 5001
        assert L.sedx_output_geometry(h, too_long, ctypes.byref(fr), ctypes.byref(sl)) == EINVAL
        assert b'5000' in L.sedx_last_error(h)
        n = ctypes.c_size_t()
        assert L.sedx_workspace_size(h, 1, too_long, ctypes.byref(n)) == EINVAL
        assert L.sedx_workspace_size(h, 2, 160000, ctypes.byref(n)) == _lib.SEDX_OK and n.value > 0
    finally:
        L.sedx_destroy(h)


def test_windowed_driver_and_events_match_goldens(golden_dir):
    """predict.py driver, 5 s windows, 1 s stride on
    Cnn_9layers_Conformer_FrameAtt: 496-frame windows padded to 500."""
    from oracle import sed_oracle as O
    g = np.load(os.path.join(golden_dir, 'conformer_windowed.npz'))['merged_5_1']
    ev = json.load(open(os.path.join(golden_dir, 'conformer_events.json')))
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    assert ev['model'] == CR.CATT and g.shape == (1, 1000, 25)
    audio = synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)[0]
    merged = CR.predict_windows(CR.full_state(CR.CATT), CR.CATT, audio, 16000, 5, 1, overlap=True)
    e = err(merged, g)
    print('windowed 5/1 max|d| =', e)
    assert e <= TOL
    for which in ('default', 'synthetic'):
        assert O.events_from_framewise(merged, tables['params_' + which]) == ev[which], which
        assert len(ev[which]) > 0
