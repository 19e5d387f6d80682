"""CPU-only checks of the five other 9-layer models (Cnn_9layers_FrameMax,
_FrameAvg, _FrameAtt, _Gru_FrameAvg, _Transformer_FrameAvg): the state_dict
contract of the classes, the synthetic weights, the torch restatement
(tests/family_refs.py) against the goldens the reference produced
(tools/make_golden_family.py), and what sedx_create / sedx_load_param accept.
No GPU work: creation and load_param are host-only until
sedx_finalize_weights."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import family_refs as FR
from oracle import sed_oracle as O
from sedx import synth

TOL = 1e-3          # the project's bar against the reference (tests/test_gpu_parity.py)
GRU, TRF = 'Cnn_9layers_Gru_FrameAtt', 'Cnn_9layers_Transformer_FrameAtt'
FAMILY_IDS = [FR.IDS[mt] for mt in FR.FAMILY]

# len(state_dict) and the total element count of the reference's own classes
# at the 16 kHz preset, 25 classes
CONTRACT = {FR.FMAX: (58, 4982690), FR.FAVG: (58, 4982690), FR.FATT: (65, 4995616),
            FR.GAVG: (66, 6165410), FR.TAVG: (68, 6034338)}


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


# ---------------------------------------------------------------------------
# state_dict contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', FR.FAMILY, ids=FAMILY_IDS)
def test_state_dict_contract(mt):
    from sedx import models
    m = getattr(models, mt)(*FR.ctor_args(mt))
    sd = m.state_dict()
    nk, ne = CONTRACT[mt]
    assert len(sd) == nk
    assert sum(v.numel() for v in sd.values()) == ne
    for k, v in O.frontend_state('16k').items():
        np.testing.assert_allclose(sd[k].numpy(), v, rtol=2e-6, atol=2e-7)
    if mt != FR.FATT:
        assert tuple(sd['fc.weight'].shape) == (25, 512) and tuple(sd['fc.bias'].shape) == (25,)
        assert not any(k.startswith('att_block.') for k in sd)
        assert torch.count_nonzero(sd['fc.bias']) == 0          # init_layer (models.py:20-26)
    seq = synth.MODEL_PARTS[mt][0]
    assert any(k.startswith('gru.') for k in sd) == (seq == 'gru')
    assert any(k.startswith('multihead.') for k in sd) == (seq == 'mha')


def test_constructor_and_forward_signatures():
    """Seven constructor arguments and forward(input, mixup_lambda=None) for
    the CNN-only classes (models.py:214-215, :255); eight and the four-argument
    forward for the other two (:467-468, :512)."""
    import inspect
    from sedx import models
    for mt in FR.FAMILY:
        cls = getattr(models, mt)
        ctor = list(inspect.signature(cls.__init__).parameters)[1:]
        fwd = list(inspect.signature(cls.forward).parameters)[1:]
        base = ['sample_rate', 'window_size', 'hop_size', 'mel_bins', 'fmin', 'fmax', 'classes_num']
        if synth.MODEL_PARTS[mt][0] is None:
            assert ctor == base and fwd == ['input', 'mixup_lambda'], mt
            with pytest.raises(TypeError):
                cls(*FR.P16, 25, 'logmel')
        else:
            assert ctor == base + ['feature_type'], mt
            assert fwd == ['input', 'mixup_lambda', 'timeshift', 'spec_augment'], mt
            with pytest.raises(TypeError):
                cls(*FR.P16, 25)
        assert models.MODEL_IDS[mt] == 2 + FR.FAMILY.index(mt)
        assert mt in models.__all__
    assert models.MODEL_IDS[GRU] == 0 and models.MODEL_IDS[TRF] == 1


def test_frameatt_has_25_classes_whatever_classes_num():
    """AttBlock(n_out=25) whatever classes_num is (models.py:416)."""
    from sedx import models
    m = models.Cnn_9layers_FrameAtt(*FR.P16, 10)
    sd = m.state_dict()
    assert tuple(sd['att_block.att.weight'].shape) == (25, 512, 1)
    assert tuple(sd['att_block.cla.weight'].shape) == (25, 512, 1)
    assert tuple(sd['att_block.bn_att.weight'].shape) == (25,)
    assert m._config().classes_num == 25


def test_feature_type_is_ignored_where_the_reference_ignores_it():
    """Gru_FrameAvg / Transformer_FrameAvg take feature_type and never read it
    (models.py:512-518, :929-935): the handle is a logmel one."""
    from sedx import models
    for mt in (FR.GAVG, FR.TAVG):
        m = getattr(models, mt)(*FR.P16, 25, 'gamma')
        assert m._config().feature_type == models.FEATURE_IDS['logmel']


@pytest.mark.parametrize('C', [25, 7])
@pytest.mark.parametrize('mt', FR.FAMILY, ids=FAMILY_IDS)
def test_synth_loads_strict(mt, C):
    from sedx import models
    m = getattr(models, mt)(*FR.ctor_args(mt, C))
    sd = m.state_dict()
    w = synth.make_state_dict(mt, classes_num=C, seed=synth.GOLDEN_SEEDS[mt])
    for k, v in w.items():
        assert k in sd and tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    assert set(sd) - set(w) == set(O.frontend_state('16k'))
    m.load_state_dict(sd, strict=True)


# ---------------------------------------------------------------------------
# synth
# ---------------------------------------------------------------------------
def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(str(v.dtype).encode())
        h.update(str(v.shape).encode())
        h.update(v.tobytes())
    return h.hexdigest()


# sha256 over (key, dtype, shape, bytes) in dict order, recorded before the
# five other models were added
OLD_DIGESTS = {
    (GRU, 0, 25): '0de11574f676e49ebc8ae944f8d524cb9e10af1f52c1384ff7f56a47ccbe5e55',
    (TRF, 1, 25): '1c8a3b6e71bbd4dd40de3b0db6cebe8d0ea288313cf50d4dad44422bc38d0836',
    (GRU, 3, 7): '9dcb4efb7d963be928b4076a65dde40110e0feb3bbda2e00a9dc71a1db54b8bb',
    (TRF, 5, 33): '957523fd23e51cd4544be1ff22470f35f4ca52862d72a90fa963820dd4839502',
}


def test_synth_output_of_the_two_first_models_is_unchanged():
    for (mt, seed, C), d in OLD_DIGESTS.items():
        assert _digest(synth.make_state_dict(mt, classes_num=C, seed=seed)) == d, (mt, seed, C)


def test_synth_draw_order_and_seeds():
    """Trunk first, then the sequence tensors, then the head: models of one
    seed share every tensor they both have up to the head."""
    assert synth.GOLDEN_SEEDS == {GRU: 0, TRF: 1, FR.FMAX: 2, FR.FAVG: 3, FR.FATT: 4, FR.GAVG: 5, FR.TAVG: 6}
    for a, b in ((GRU, FR.GAVG), (TRF, FR.TAVG), (GRU, FR.FAVG), (FR.FMAX, FR.FAVG)):
        sa, sb = synth.make_state_dict(a, seed=9), synth.make_state_dict(b, seed=9)
        shared = [k for k in sa if k in sb]
        assert any(k.startswith('conv_block4.') for k in shared)
        if synth.MODEL_PARTS[a][0] == synth.MODEL_PARTS[b][0] and synth.MODEL_PARTS[a][0]:
            assert any(k.split('.')[0] in ('gru', 'multihead') for k in shared)
        for k in shared:
            assert np.array_equal(sa[k], sb[k]), (a, b, k)
    sd = synth.make_state_dict(FR.FAVG, classes_num=7, seed=1)
    assert list(sd)[-2:] == ['fc.weight', 'fc.bias'] and sd['fc.weight'].shape == (7, 512)
    assert (sd['fc.bias'] <= 0).all() and (sd['fc.bias'] >= -0.5).all()
    with pytest.raises(ValueError):
        synth.make_state_dict('Cnn_14layers_FrameAtt')


# ---------------------------------------------------------------------------
# the restatement against the goldens
# ---------------------------------------------------------------------------
def _waves(kind):
    if kind == 'short':
        return synth.make_waveforms(2, seconds=5280 / 16000., sample_rate=16000, seed=11)
    if kind == 'ragged':
        return synth.make_waveforms(1, seconds=7777 / 16000., sample_rate=16000, seed=12)
    return synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)[:1]


@pytest.mark.parametrize('kind', ['short', 'ragged', 'clip10s'])
@pytest.mark.parametrize('mt', FR.FAMILY, ids=FAMILY_IDS)
def test_restatement_matches_goldens(mt, kind, golden_dir):
    g = np.load(os.path.join(golden_dir, 'family_%s.npz' % mt))
    out, acts = FR.forward(FR.full_state(mt), mt, wave=_waves(kind), return_acts=True)
    for k in FR.KEYS:
        e = err(out[k].numpy(), g['%s_%s' % (kind, k)])
        print(mt, kind, k, 'max|d| =', e)
        assert e <= TOL
    if kind == 'short':
        assert err(acts['cnn_out'].numpy(), g['short_cnn_out']) <= TOL
        assert err(acts['seq_out'].numpy(), g['short_seq_out']) <= TOL
    if kind == 'ragged':
        assert out['framewise_output'].shape[1] == 48      # 8 * 6 frames: no pad to 100


def test_restatement_float64_agrees_with_float32():
    """The same functions in float64 (the GPU tests' yardstick) give the fp32
    head up to fp32 rounding."""
    for mt in FR.FAMILY:
        x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 9, 512)).astype(np.float32))
        a = FR.head(FR.state(mt, dtype=torch.float32), mt, x)
        b = FR.head(FR.state(mt, dtype=torch.float64), mt, x.double())
        for k in FR.KEYS:
            assert b[k].dtype == torch.float64 and a[k].shape == b[k].shape
            assert err(a[k].numpy(), b[k].numpy()) <= 1e-5 * max(1.0, float(b[k].abs().max())), (mt, k)


def test_windowed_driver_and_events_match_goldens(golden_dir):
    """predict.py driver, 5 s windows, 1 s stride on Cnn_9layers_Gru_FrameAvg:
    496-frame windows (no pad to 500) merged at a 100-frame step."""
    g = np.load(os.path.join(golden_dir, 'family_windowed.npz'))['merged_5_1']
    ev = json.load(open(os.path.join(golden_dir, 'family_events.json')))
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    assert ev['model'] == FR.GAVG and g.shape == (1, 996, 25)
    audio = synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)[0]
    merged = FR.predict_windows(FR.full_state(FR.GAVG), FR.GAVG, audio, 16000, 5, 1, overlap=True)
    e = err(merged, g)
    print('windowed 5/1 max|d| =', e)
    assert e <= TOL
    for which in ('default', 'synthetic'):
        assert O.events_from_framewise(merged, tables['params_' + which]) == ev[which], which
        assert len(ev[which]) > 0


# ---------------------------------------------------------------------------
# sedx_create / sedx_load_param
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


def test_create_accepts_the_family_and_rejects_the_rest():
    from sedx import _lib, models
    L = _lib.lib()
    EINVAL = 1
    for mt in FR.FAMILY:
        st, h = _create(models.MODEL_IDS[mt])
        assert st == _lib.SEDX_OK and h.value, mt
        L.sedx_destroy(h)
        st, h = _create(models.MODEL_IDS[mt], feature_type=models.FEATURE_IDS['gamma'])
        assert st == EINVAL and not h.value, mt
    for bad in (max(models.MODEL_IDS.values()) + 1, -1):
        st, h = _create(bad)
        assert st == EINVAL and not h.value
    assert L.sedx_abi_version() == 6


def test_load_param_key_sets_follow_the_model():
    from sedx import _lib, models
    L = _lib.lib()
    EKEY = 5
    GRU_W, ATT_W, FC_W, MHA_W = (('gru.weight_ih_l0', (768, 512)), ('att_block.att.weight', (25, 512, 1)),
                                 ('fc.weight', (25, 512)), ('multihead.w_qs.weight', (512, 512)))
    accepts = {FR.FMAX: {FC_W}, FR.FAVG: {FC_W}, FR.FATT: {ATT_W}, FR.GAVG: {FC_W, GRU_W},
               FR.TAVG: {FC_W, MHA_W}, GRU: {ATT_W, GRU_W}, TRF: {ATT_W, MHA_W}}
    for mt, ok in accepts.items():
        st, h = _create(models.MODEL_IDS[mt])
        assert st == _lib.SEDX_OK
        try:
            for key, shape in (GRU_W, ATT_W, FC_W, MHA_W):
                st = _load(h, key, shape)
                assert st == (_lib.SEDX_OK if (key, shape) in ok else EKEY), (mt, key)
                if st == EKEY:
                    assert key.encode() in L.sedx_last_error(h)
            assert _load(h, 'conv_block4.conv2.weight', (512, 512, 3, 3)) == _lib.SEDX_OK
            if (FC_W in ok):
                assert _load(h, 'fc.weight', (512, 25)) == EKEY          # mis-shaped
                assert _load(h, 'fc.bias', (25,)) == _lib.SEDX_OK
        finally:
            L.sedx_destroy(h)


def test_finalize_names_a_missing_family_key():
    """An fc handle that never got fc.bias: finalize fails on the key check,
    before any device work."""
    from sedx import _lib, models
    L = _lib.lib()
    st, h = _create(models.MODEL_IDS[FR.FAVG])
    assert st == _lib.SEDX_OK
    try:
        assert _load(h, 'fc.weight', (25, 512)) == _lib.SEDX_OK
        assert L.sedx_finalize_weights(h) == 5
        assert b'missing key' in L.sedx_last_error(h)
    finally:
        L.sedx_destroy(h)
