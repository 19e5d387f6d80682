"""Cnn_9layers_Conformer (model id 21) and Cnn_9layers_Gru_Reg (id 22) without a
GPU: the classes and their state_dicts against the reference's
(tests/golden/token_meta.json), strict loading and the refusal of the
neighbouring models' key sets, the ABI (ids 21 and 22; 20 and 23 unknown; no gamma
for id 21; abi 6), the geometry against the reference's frame table, the refusals
from every size query and from the window geometry, the attention knob, the
restatement of tests/token_refs.py against the reference's recorded encoder
input and output, and the host side under ASan + UBSan
(tests/native/token_driver.cpp)."""
import ctypes
import inspect
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import token_refs as TR
from sedx import _lib, models, synth

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sound-event-detection_amd')
OK, EINVAL, EKEY = 0, 1, 5
TOKEN, REG = TR.TOKEN, TR.REG
IDS = {TOKEN: 21, REG: 22}
HOP = 160
FRONTEND = {'spectrogram_extractor.stft.conv_real.weight', 'spectrogram_extractor.stft.conv_imag.weight',
            'logmel_extractor.melW'}
CONSTANT = {TOKEN: FRONTEND | {'encoder.input_layer.4.pe'} | {
    'encoder.conformer_blocks.%d.mhsa.pos_emb.inv_freq' % b for b in range(3)}, REG: FRONTEND}


def build(mt, classes=25, **kw):
    if mt == TOKEN:
        return models.Cnn_9layers_Conformer(*TR.P16, classes, **kw)
    return models.Cnn_9layers_Gru_Reg(*TR.P16, classes, kw.pop('feature_type', 'logmel'))


def config(mid, feature=0, classes=25):
    cfg = _lib.SedxConfig()
    cfg.model_type, cfg.feature_type = mid, feature
    cfg.sample_rate, cfg.window_size, cfg.hop_size, cfg.mel_bins = TR.P16[:4]
    cfg.fmin, cfg.fmax, cfg.classes_num = float(TR.P16[4]), float(TR.P16[5]), classes
    return cfg


def create(mid, **kw):
    h = ctypes.c_void_p()
    st = _lib.lib().sedx_create(ctypes.byref(config(mid, **kw)), 0, ctypes.byref(h))
    return st, h


def load(h, key, arr):
    a = np.ascontiguousarray(arr, np.float32)
    shape = (ctypes.c_int64 * a.ndim)(*a.shape)
    return _lib.lib().sedx_load_param(h, key.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim)


@pytest.fixture(scope='module')
def meta(golden_dir):
    return json.load(open(os.path.join(golden_dir, 'token_meta.json')))


def test_classes_exist_with_the_references_signatures():
    for mt in (TOKEN, REG):
        assert mt in models.__all__ and models.MODEL_IDS[mt] == IDS[mt] and getattr(models, mt)._model_name == mt
    assert not hasattr(models, 'Cnn_7layers_Conformer') and 'Cnn_7layers_Conformer' not in models.MODEL_IDS
    p = inspect.signature(models.Cnn_9layers_Conformer.__init__).parameters
    assert list(p) == ['self', 'sample_rate', 'window_size', 'hop_size', 'mel_bins', 'fmin', 'fmax', 'classes_num',
                       'cnn_kwargs', 'encoder_kwargs', 'encoder_type', 'pooling', 'layer_init']
    assert [p[k].default for k in list(p)[8:]] == [None, None, 'Conformer', 'token', 'pytorch']
    f = inspect.signature(models.Cnn_9layers_Conformer.forward).parameters
    assert list(f) == ['self', 'x', 'mixup_lambda', 'timeshift', 'mask']
    assert [f[k].default for k in list(f)[2:]] == [None, False, None]
    p = inspect.signature(models.Cnn_9layers_Gru_Reg.__init__).parameters
    assert list(p) == ['self', 'sample_rate', 'window_size', 'hop_size', 'mel_bins', 'fmin', 'fmax', 'classes_num',
                       'feature_type']
    f = inspect.signature(models.Cnn_9layers_Gru_Reg.forward).parameters
    assert list(f) == ['self', 'input', 'mixup_lambda', 'timeshift']
    assert _lib.TUNE_CF_ATTN == 8


def test_constructor_refusals_name_the_supported_value():
    for kw, word in ((dict(encoder_type='Transformer'), 'Conformer'), (dict(encoder_type='Lstm'), 'Conformer'),
                     (dict(pooling='attention'), 'token'), (dict(pooling='auto'), 'token'),
                     (dict(layer_init='xavier_uniform'), 'pytorch')):
        with pytest.raises(ValueError, match=word):
            build(TOKEN, **kw)
    m = build(TOKEN, cnn_kwargs={'anything': 1}, encoder_kwargs={'adim': 7})      # accepted and ignored
    assert m.encoder_kwargs['adim'] == 144 and not m._has_embedding
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16000))                 # training mode
    m.eval()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16000))                 # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        m(torch.zeros(1, 16000), mask=torch.ones(1, 1, 3))
    with pytest.raises(TypeError):
        m(torch.zeros(1, 16000), spec_augment=True)      # the reference's forward has no such argument
    r = build(REG, classes=10).eval()
    assert r.classes_num == 25 and r._embedding_cla and tuple(r.att_block.att.weight.shape) == (25, 512, 1)
    assert build(REG, feature_type='gamma').feature_type == 'gamma'
    with pytest.raises(RuntimeError):
        r(torch.zeros(1, 16000))


@pytest.mark.parametrize('classes', [25, 10])
@pytest.mark.parametrize('mt', [TOKEN, REG])
def test_class_mirrors_the_reference_state_dict(mt, classes, meta):
    sd = build(mt, classes).state_dict()
    got = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()]
    ref = meta[mt]['classes_%d' % classes]
    assert got == ref['keys']
    assert len(sd) == ref['entries'] and sum(v.numel() for v in sd.values()) == ref['elements']
    if mt == TOKEN:
        assert ref['entries'] == 170
        assert tuple(sd['classifier.weight'].shape) == (classes, 144) and tuple(sd['linear_emb.weight'].shape) == (512, 1)
        assert tuple(sd['encoder.input_layer.0.weight'].shape) == (144, 512)
        assert not any(k.startswith(('att_block.', 'fc.')) for k in sd)
    else:
        g = models.Cnn_9layers_Gru_FrameAtt(*TR.P16, 25, 'logmel').state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(v.shape)) for k, v in g.items()]


@pytest.mark.parametrize('mt', [TOKEN, REG])
def test_strict_load_and_refusal_of_the_neighbouring_key_sets(mt, meta):
    m = build(mt)
    sd = m.state_dict()
    w = synth.make_state_dict(mt, seed=TR.SEEDS[mt])
    assert set(sd) - set(w) == CONSTANT[mt]
    assert [k for k in sd if k in w] == list(w)                      # the reference's order
    for k, v in w.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    others = ('Cnn_9layers_Conformer_FrameAtt', 'Cnn_9layers_Conformer_FrameAvg', REG) if mt == TOKEN else (
        'Cnn_9layers_Gru_FrameAvg', 'Cnn_9layers_Transformer_FrameAtt', TOKEN)
    for other in others:
        osd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(other, seed=0).items()}
        with pytest.raises(RuntimeError):
            m.load_state_dict(osd, strict=True)
    assert meta[REG]['windowed']['threshold_margin'] >= 1e-4
    # one seed: the trunk's draws are the other 9-layer models', the encoder's those of ids 7 and 8; and the
    # earlier models' draws do not move (tests/golden/ of those models is regenerated from them)
    c7 = synth.make_state_dict('Cnn_9layers_Conformer_FrameAvg', seed=TR.SEEDS[mt])
    shared = [k for k in w if k.startswith(('bn0.', 'conv_block') + (('encoder.',) if mt == TOKEN else ()))]
    assert shared and all(np.array_equal(w[k], c7[k]) for k in shared)
    if mt == REG:
        g = synth.make_state_dict('Cnn_9layers_Gru_FrameAtt', seed=TR.SEEDS[mt])
        assert list(g) == list(w) and all(np.array_equal(w[k], g[k]) for k in w)
        assert synth.make_state_dict(REG, classes_num=10)['att_block.cla.weight'].shape == (25, 512, 1)
    else:
        assert synth.make_state_dict(TOKEN, classes_num=10)['classifier.weight'].shape == (10, 144)


def test_abi_enum_values():
    hdr = open(os.path.join(os.path.dirname(PKG), 'include', 'sedx.h')).read()
    assert '#define SEDX_ABI_VERSION 6' in hdr
    for s in ('SEDX_MODEL_CONFORMER_TOKEN = 21', 'SEDX_MODEL_GRU_REG = 22', 'SEDX_TUNE_CF_ATTN = 8'):
        assert s in hdr
    L = _lib.lib()
    assert L.sedx_abi_version() == 6
    for a, kw, want in [((21,), {}, OK), ((22,), {}, OK), ((20,), {}, EINVAL), ((23,), {}, EINVAL),
                        ((21,), dict(feature=1), EINVAL), ((22,), dict(feature=1), OK), ((0,), dict(feature=1), OK),
                        ((21,), dict(classes=1), OK), ((21,), dict(classes=256), OK), ((21,), dict(classes=257), EINVAL)]:
        st, h = create(*a, **kw)
        assert st == want, (a, kw)
        if h:
            L.sedx_destroy(h)


def test_geometry_equals_the_references_table(meta):
    L = _lib.lib()
    fr, sl, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
    for mt in (TOKEN, REG):
        table = meta[mt]['frames']
        assert len(table) == 130 and table == [8 * t for t in range(1, 131)]      # what the reference's forward gave
        st, h = create(IDS[mt])
        assert st == OK
        try:
            for t3 in range(1, 131):
                for T in (8 * t3, 8 * t3 + 7):
                    assert L.sedx_output_geometry(h, (T - 1) * HOP, ctypes.byref(fr), ctypes.byref(sl)) == OK, T
                    assert (fr.value, sl.value) == (table[t3 - 1], 8 * t3 + 1 if mt == TOKEN else t3), (mt, T)
                    assert L.sedx_workspace_size(h, 2, (T - 1) * HOP, ctypes.byref(nb)) == OK and nb.value > 0
            for samples, frames in ((10400, 64), (7777, 48), (81760, 512), (160000, 1000)):
                assert L.sedx_output_geometry(h, samples, ctypes.byref(fr), ctypes.byref(sl)) == OK
                assert fr.value == frames
        finally:
            L.sedx_destroy(h)
    assert TR.geometry(1001) == (125, 1001, 1000) and TR.geometry(49) == (6, 49, 48)


def test_refusals_come_back_from_every_size_query():
    """T < 8 and more than 5000 tokens: sedx_output_geometry, sedx_workspace_size, both launch plans and the
    window queries answer SEDX_EINVAL with the forward's reason."""
    L = _lib.lib()
    st, h = create(21)
    assert st == OK
    fr, sl, nb, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t(), ctypes.c_int32()
    grows, crows = (_lib.SedxGemmLaunch * 40)(), (_lib.SedxConvLaunch * 40)()
    try:
        for T, why in ((7, b'3 pooling'), (1, b'3 pooling'), (5000, b'5000'), (8 * 625, b'5000'), (40007, b'5000')):
            length = (T - 1) * HOP
            assert L.sedx_output_geometry(h, length, ctypes.byref(fr), ctypes.byref(sl)) == EINVAL, T
            assert why in L.sedx_last_error(h), (T, L.sedx_last_error(h))
            assert L.sedx_workspace_size(h, 1, length, ctypes.byref(nb)) == EINVAL, T
            assert why in L.sedx_last_error(h)
            assert L.sedx_gemm_launch_plan(h, 1, length, 256, grows, 40, ctypes.byref(n)) == EINVAL, T
            assert L.sedx_conv_launch_plan(h, 1, length, 256, crows, 40, ctypes.byref(n)) == EINVAL, T
        for T in (8, 8 * 624 + 7):
            assert L.sedx_output_geometry(h, (T - 1) * HOP, ctypes.byref(fr), ctypes.byref(sl)) == OK, T
            assert sl.value == 8 * (T // 8) + 1 <= 5000
            assert L.sedx_workspace_size(h, 1, (T - 1) * HOP, ctypes.byref(nb)) == OK
        # the GEMM rows of a 10 s pair: 2002 token rows, the input layer's K = 512, the classifier last
        assert L.sedx_gemm_launch_plan(h, 2, 160000, 256, grows, 40, ctypes.byref(n)) == OK and n.value == 29
        assert (grows[0].M, grows[3].M, grows[3].K, grows[3].N) == (1001, 2002, 512, 144)
        assert (grows[28].stage, grows[28].M, grows[28].K, grows[28].N) == (10, 2002, 144, 64)
        # block 4's conv2 (stage 8) is planned with the store epilogue (0) in place of the frequency mean (2)
        assert L.sedx_conv_launch_plan(h, 2, 160000, 256, crows, 40, ctypes.byref(n)) == OK
        last = [r for r in crows[:n.value] if r.stage == 8]
        assert last and all((r.epi, r.F, r.cin, r.cout) == (0, 8, 512, 512) for r in last)
        # windows: 5 s at a 1 s stride on 10 s: six windows of 496 frames; 0.04 s windows have 5 frames, 51 s windows
        # 5097 tokens
        nw, ws, mf = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        spec = _lib.window_spec(5, 1.0)
        assert L.sedx_window_geometry(h, 160000, ctypes.byref(spec), ctypes.byref(nw), ctypes.byref(ws), ctypes.byref(mf)) == OK
        assert (nw.value, ws.value) == (6, 80000)
        assert L.sedx_window_workspace_size(h, 1, 160000, ctypes.byref(spec), ctypes.byref(nb)) == OK
        spec = _lib.window_spec(51, 1.0)
        assert L.sedx_window_geometry(h, 60 * 16000, ctypes.byref(spec), ctypes.byref(nw), ctypes.byref(ws), ctypes.byref(mf)) == EINVAL
        assert b'5000' in L.sedx_last_error(h)
        assert L.sedx_window_workspace_size(h, 1, 60 * 16000, ctypes.byref(spec), ctypes.byref(nb)) == EINVAL
    finally:
        L.sedx_destroy(h)
    # id 22 answers as id 0 does for an input too short for any forward: the size is reported, frames 0
    for mid in (0, 22):
        st, h = create(mid)
        try:
            assert L.sedx_output_geometry(h, 6 * HOP, ctypes.byref(fr), ctypes.byref(sl)) == OK and fr.value == 0
        finally:
            L.sedx_destroy(h)


def test_attention_knob_values():
    L = _lib.lib()
    for mid in (21, 7, 8, 19, 0):
        st, h = create(mid)
        assert st == OK
        try:
            for v, want in ((0, OK), (1, OK), (2, OK), (3, EINVAL), (-1, EINVAL)):
                assert L.sedx_set_tuning(h, 8, v) == want, (mid, v)
            assert L.sedx_set_tuning(h, 9, 0) == EINVAL
        finally:
            L.sedx_destroy(h)


def test_key_table_and_finalize_names_a_missing_key():
    L = _lib.lib()
    st, h = create(21, classes=10)
    assert st == OK
    try:
        for k, shape, want in (('classifier.weight', (10, 144), OK), ('classifier.weight', (25, 144), EKEY),
                               ('classifier.bias', (10,), OK), ('classifier.bias', (25,), EKEY),
                               ('linear_emb.weight', (512, 1), OK), ('linear_emb.weight', (2048, 1), EKEY),
                               ('linear_emb.bias', (512,), OK), ('att_block.att.weight', (25, 144, 1), EKEY),
                               ('fc.weight', (10, 144), EKEY), ('gru.weight_ih_l0', (768, 512), EKEY),
                               ('encoder.input_layer.0.weight', (144, 512), OK),
                               ('encoder.input_layer.0.weight', (144, 2048), EKEY)):
            assert load(h, k, np.zeros(shape)) == want, (k, shape)
            if want == EKEY:
                assert k.encode() in L.sedx_last_error(h)
        sd = {k: v.numpy() for k, v in build(TOKEN, 10).state_dict().items() if not k.endswith('num_batches_tracked')}
        for missing in ('linear_emb.bias', 'classifier.weight'):
            st2, h2 = create(21, classes=10)
            try:
                for k, v in sd.items():
                    if k != missing:
                        assert load(h2, k, v) == OK, k
                assert L.sedx_finalize_weights(h2) == EKEY            # host-side check: no device needed
                assert missing.encode() in L.sedx_last_error(h2)
            finally:
                L.sedx_destroy(h2)
    finally:
        L.sedx_destroy(h)
    # ids 7 and 8 still drop the four keys at any shape
    st, h = create(7)
    try:
        assert load(h, 'classifier.weight', np.zeros((3, 7))) == OK and load(h, 'linear_emb.bias', np.zeros(5)) == OK
    finally:
        L.sedx_destroy(h)


def test_restatement_reproduces_the_references_encoder_input_and_output(golden_dir):
    """tests/token_refs.py on the reference's own recorded tensors (the 'short' case): the tag row, the pe offset
    by one and the encoder at 65 tokens, then the classifier and the split."""
    g = np.load(os.path.join(golden_dir, 'token_%s.npz' % TOKEN))
    s32 = TR.state(torch.float32)
    seq_in, seq_out = torch.from_numpy(g['short_seq_in']), torch.from_numpy(g['short_seq_out'])
    assert tuple(seq_in.shape) == (2, 65, 512) and tuple(seq_out.shape) == (2, 65, 144)
    tag = TR.tag_token_fp32(s32)
    assert np.array_equal(seq_in[0, 0].numpy(), tag) and np.array_equal(seq_in[1, 0].numpy(), tag)
    assert np.array_equal(TR.tag_token(s32).numpy(), tag)
    with torch.no_grad():
        x = seq_in
        for src, _ in TR.STEPS[1:]:
            x = TR.step(s32, src, x)
        out = TR.head(s32, x)
    scale = max(1.0, float(seq_out.abs().max()))
    e = float((x - seq_out).abs().max())
    print('encoder at 65 tokens: max|d| = %.3g (scale %.3g)' % (e, scale))
    assert e <= 1e-4 * scale
    for k in TR.KEYS:
        e = float(np.abs(out[k].numpy() - g['short_' + k]).max())
        print(k, 'max|d| = %.3g' % e)
        assert out[k].shape == g['short_' + k].shape and e <= 1e-4 * max(1.0, float(np.abs(g['short_' + k]).max()))
    # 7 -> 8 on a small input: the (t, f) token order against a loop
    s64 = TR.state(torch.float64)
    rng = np.random.default_rng(0)
    x7 = torch.from_numpy(rng.uniform(0, 1, (1, 2, 8, 512)))
    with torch.no_grad():
        tok = TR.tokens(s64, x7)
        y = torch.nn.functional.relu(TR.O._bn(s64, 'conv_block4.bn2', torch.nn.functional.conv2d(
            x7.permute(0, 3, 1, 2), s64['conv_block4.conv2.weight'], padding=1)))
    assert tuple(tok.shape) == (1, 17, 512) and torch.equal(tok[0, 0], TR.tag_token(s64))
    for t in range(2):
        for f in range(8):
            assert torch.equal(tok[0, 1 + 8 * t + f], y[0, :, t, f])
    with pytest.raises(ValueError):
        TR.step(s64, 8, torch.zeros(1, 5001, 512, dtype=torch.float64))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_side_under_sanitizers():
    r = subprocess.run(['make', '-s', '-C', PKG, 'asan-token'], capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert 'token_driver: clean' in out and 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out, out[-4000:]
