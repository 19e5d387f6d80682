"""Cnn14_DecisionLevelAtt without a GPU: the class and its state_dict against
the reference's (tests/golden/cnn14_meta.json), strict loading, the ABI (model
id 13, up to 527 classes for this model alone), the key set a handle takes and
what finalize names when ``fc1.bias`` is missing, the geometry closed form with
its two refusals through both size queries, the inference-only guards, the
float64 restatement of the new steps (tests/cnn14_refs.py) against the
reference's own tensors, and the host side under ASan + UBSan
(tests/native/cnn14_driver.cpp)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cnn14_refs as C
from sedx import _lib, models, synth

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sound-event-detection_amd')
MT = C.CNN14
OK, EINVAL, EKEY = 0, 1, 5


def build(classes=25, preset=C.P16):
    return getattr(models, MT)(*preset, classes)


def config(mid=13, feature=0, classes=25, preset=C.P16):
    cfg = _lib.SedxConfig()
    cfg.model_type, cfg.feature_type = mid, feature
    cfg.sample_rate, cfg.window_size, cfg.hop_size, cfg.mel_bins = preset[:4]
    cfg.fmin, cfg.fmax, cfg.classes_num = float(preset[4]), float(preset[5]), classes
    return cfg


def create(**kw):
    h = ctypes.c_void_p()
    st = _lib.lib().sedx_create(ctypes.byref(config(**kw)), 0, ctypes.byref(h))
    return st, h


def load(h, key, arr):
    a = np.ascontiguousarray(arr, np.float32)
    shape = (ctypes.c_int64 * a.ndim)(*a.shape)
    return _lib.lib().sedx_load_param(h, key.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim)


def test_class_exists_by_name_and_mirrors_the_reference_state_dict(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, 'cnn14_meta.json')))
    m = build()
    sd = m.state_dict()
    got = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()]
    assert got == meta[MT]['keys']
    assert len(sd) == meta[MT]['entries'] == 91
    assert sum(v.numel() for v in sd.values()) == meta[MT]['elements'] == 80072228
    m527 = build(527, C.P32).state_dict()
    assert len(m527) == meta['classes_527']['entries'] == 91
    assert sum(v.numel() for v in m527.values()) == meta['classes_527']['elements'] == 82935272
    assert models.MODEL_IDS[MT] == 13 and MT in models.__all__
    # the constructor's class count reaches the AttBlock (the Cnn_14layers_* models ignore theirs)
    assert build(10).att_block.att.weight.shape == (10, 2048, 1) and build(10).classes_num == 10
    with pytest.raises(TypeError):
        getattr(models, MT)(*C.P16, 25, 'logmel')      # seven arguments, no feature_type


def test_strict_load_and_refusal_of_a_14_layer_gru_key_set():
    m = build()
    sd = m.state_dict()
    w = synth.make_state_dict(MT, seed=C.SEED)
    assert set(w) < set(sd)
    for k, v in w.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    gru = dict(sd)
    for k in ('fc1.weight', 'fc1.bias'):
        del gru[k]
    for k, v in synth.make_state_dict('Cnn_14layers_Gru_FrameAtt', seed=0).items():
        if k.startswith('gru.'):
            gru[k] = torch.from_numpy(np.asarray(v))
    with pytest.raises(RuntimeError):
        m.load_state_dict(gru, strict=True)


def test_synth_draws_trunk_then_fc1_then_the_head_at_the_callers_class_count():
    a = synth.make_state_dict(MT, classes_num=25, seed=3)
    b = synth.make_state_dict(MT, classes_num=527, seed=3)
    g = synth.make_state_dict('Cnn_14layers_Gru_FrameAtt', seed=3)
    assert a['att_block.att.weight'].shape == (25, 2048, 1) and b['att_block.cla.weight'].shape == (527, 2048, 1)
    for k in a:
        if k.startswith(('bn0', 'conv_block', 'fc1')):
            assert np.array_equal(a[k], b[k]), k                    # the class count changes the head only
        if k.startswith(('bn0', 'conv_block')):
            assert np.array_equal(a[k], g[k]), k                    # the 14-layer trunk's draws
    assert a['fc1.weight'].shape == (2048, 2048) and float(np.abs(a['fc1.bias']).max()) <= 0.1
    keys = list(a)
    assert keys.index('conv_block6.bn2.running_var') < keys.index('fc1.weight') < keys.index('att_block.att.weight')


def test_abi_enum_and_class_limits():
    hdr = open(os.path.join(os.path.dirname(PKG), 'include', 'sedx.h')).read()
    assert '#define SEDX_ABI_VERSION 6' in hdr and 'SEDX_MODEL_CNN14_DECISIONLEVELATT = 13' in hdr
    L = _lib.lib()
    assert L.sedx_abi_version() == 6
    cases = [(dict(classes=25), OK), (dict(classes=527, preset=C.P32), OK), (dict(classes=528, preset=C.P32), EINVAL),
             (dict(feature=1), EINVAL), (dict(mid=12), EINVAL), (dict(mid=14), EINVAL),
             # every other model keeps its 256 limit
             (dict(mid=10, classes=256), OK), (dict(mid=10, classes=257), EINVAL), (dict(mid=4, classes=527), EINVAL)]
    for kw, want in cases:
        st, h = create(**kw)
        assert st == want, kw
        if h:
            L.sedx_destroy(h)


def test_key_set_and_finalize_names_a_missing_fc1_bias():
    L = _lib.lib()
    st, h = create(classes=3)
    assert st == OK
    try:
        m = build(3)
        sd = {k: v.numpy() for k, v in m.state_dict().items() if not k.endswith('num_batches_tracked')}
        for k in ('fc1.weight', 'att_block.att.weight', 'att_block.bn_att.running_var', 'conv_block6.conv2.weight'):
            assert load(h, k, sd[k]) == OK, k
        # another family's keys, and fc1 with another shape
        assert load(h, 'gru.weight_ih_l0', np.zeros((3072, 2048))) == EKEY
        assert load(h, 'multihead.fc.weight', np.zeros((2048, 512))) == EKEY
        assert load(h, 'fc.weight', np.zeros((3, 2048))) == EKEY
        assert load(h, 'fc1.weight', np.zeros((2048, 512))) == EKEY
        assert load(h, 'att_block.att.weight', np.zeros((25, 2048, 1))) == EKEY      # the handle has 3 classes
        for k, v in sd.items():
            if k != 'fc1.bias':
                assert load(h, k, v) == OK, k
        assert L.sedx_finalize_weights(h) == EKEY                  # host-side check: no device needed
        assert b'fc1.bias' in L.sedx_last_error(h)
    finally:
        L.sedx_destroy(h)


def test_geometry_closed_form():
    """T -> (T // 32, T - 1) over T = 31 .. 2100 against the reference's rule:
    five floor halvings, x32, padded with (T % 32) - 1 copies of the last frame;
    no output below 32 frames and at every multiple of 32."""
    for T in range(31, 2101):
        t = T
        for _ in range(5):
            t //= 2
        pad = T % 32 - 1
        if t < 1 or pad < 0:
            assert C.geometry(T) is None, T
        else:
            assert C.geometry(T) == (t, 32 * t + pad) == (T // 32, T - 1), T
    assert C.geometry(1001) == (31, 1000) and C.geometry(501) == (15, 500)
    assert C.geometry(66) == (2, 65) and C.geometry(33) == (1, 32) and C.geometry(49) == (1, 48)


def test_size_queries_answer_the_closed_form_and_refuse_what_the_reference_raises_on():
    L = _lib.lib()
    for preset, classes in ((C.P16, 25), (C.P32, 527)):
        st, h = create(classes=classes, preset=preset)
        assert st == OK
        hop = preset[2]
        fr, sl, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
        try:
            for T in list(range(28, 200)) + [256, 500, 501, 992, 1000, 1001, 1024, 1025]:
                Ls = (T - 1) * hop + 7                              # T = L // hop + 1
                want = C.geometry(T)
                g = L.sedx_output_geometry(h, Ls, ctypes.byref(fr), ctypes.byref(sl))
                w = L.sedx_workspace_size(h, 2, Ls, ctypes.byref(nb))
                if want is None:
                    assert g == EINVAL and w == EINVAL, T
                    msg = L.sedx_last_error(h)
                    assert (b'too short' in msg) if T < 32 else (b'multiple of 32' in msg), (T, msg)
                else:
                    assert g == OK and w == OK and nb.value > 0, T
                    assert (sl.value, fr.value) == want, T
        finally:
            L.sedx_destroy(h)


def test_cpu_tensors_and_train_mode_raise():
    m = build()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16000))                 # train mode
    m.eval()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16000))                 # a CPU tensor: no fallback


@pytest.mark.parametrize('name,classes', [('cnn14_%s.npz' % MT, 25), ('cnn14_audioset.npz', 527)])
def test_float64_restatement_reproduces_the_references_tensors(name, classes, golden_dir):
    """cnn14_refs' float64 steps on the golden's own seq_in (block 6's frequency
    mean) give its fc1 input, its relu(fc1) and both outputs to <= 1e-5: the
    restatement the GPU tests measure against is the reference's arithmetic."""
    g = np.load(os.path.join(golden_dir, name))
    sd = C.state(torch.float64, classes)
    s = torch.from_numpy(g['short_seq_in']).double().transpose(1, 2)       # [B, 2048, T5]
    with torch.no_grad():
        p = C.step_pool(s).transpose(1, 2)
        h = C.step_decision(sd, s)
        out = C.step_head(sd, h, g['short_framewise_output'].shape[1])
    for what, a, b in (('fc1_in', p, g['short_fc1_in']), ('seq_out', h, g['short_seq_out']),
                       ('framewise', out['framewise_output'], g['short_framewise_output']),
                       ('clipwise', out['clipwise_output'], g['short_clipwise_output'])):
        e = float(np.abs(a.numpy() - b.astype(np.float64)).max())
        print(name, what, 'max|d| = %.3g' % e)
        assert a.shape == b.shape and e <= 1e-5, what
    # the synthetic weights exercise every branch (the issue's observations): spread outputs,
    # fc1 outputs of both signs, no attention logit at the clamp
    fw = g['short_framewise_output']
    assert 0.02 < fw.min() and fw.max() < 0.98 and fw.std() > 0.1
    pos = float((g['short_seq_out'] > 0).mean())
    assert 0.3 < pos < 0.7, pos
    att = torch.nn.functional.conv1d(h.transpose(1, 2), sd['att_block.att.weight'], sd['att_block.att.bias'])
    assert float(att.abs().max()) < 10.0
    # the pad frames are copies of the last repeated frame
    assert np.array_equal(fw[:, 64:], np.repeat(fw[:, 63:64], fw.shape[1] - 64, axis=1))


def test_pooled_operand_emulation_matches_torch_in_fp32_and_divides_by_three_at_the_edges():
    rng = np.random.default_rng(5)
    S = np.abs(rng.standard_normal((3, 5, 2048))).astype(np.float32)
    P = C.pooled_fp32(S)
    ref = C.step_pool(torch.from_numpy(S).double().transpose(1, 2)).transpose(1, 2).numpy()
    assert float(np.abs(P - ref).max()) <= 4 * 2.0 ** -23 * float(np.abs(ref).max())
    # a clip's first frame: max(S0, S1) + (S0 + S1) / 3, never a neighbour from the clip before
    want = np.maximum(S[:, 0], S[:, 1]).astype(np.float64) + (S[:, 0].astype(np.float64) + S[:, 1]) / 3.0
    assert float(np.abs(P[:, 0] - want).max()) <= 4 * 2.0 ** -23 * float(want.max())
    one = C.pooled_fp32(S[:, :1])                                   # T5 = 1: S + S / 3
    assert np.array_equal(one, (S[:, :1] + S[:, :1] / np.float32(3.0)).astype(np.float32))
    assert sorted(C.kernel_k_order().tolist()) == list(range(512))


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_side_under_sanitizers():
    r = subprocess.run(['make', '-s', '-C', PKG, 'asan-cnn14'], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert 'cnn14_driver: clean' in out and 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out, out[-4000:]
