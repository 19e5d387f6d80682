"""The two 14-layer models without a GPU: the classes, their state_dict
against the reference's (tests/golden/deep14_meta.json), strict loading, the
geometry closed form, the inference-only guards, the ABI, and the host side
(forward plan, expected_params, deep conv weight pack) under ASan + UBSan
(tests/native/deep14_driver.cpp)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import deep14_refs as D
from sedx import _lib, models, synth

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sound-event-detection_amd')
MODELS = (D.GRU14, D.TRF14)
P16 = (16000, 512, 160, 64, 25, 7000)


def build(mt):
    return getattr(models, mt)(*P16, 25, 'logmel')


@pytest.mark.parametrize('mt', MODELS)
def test_class_exists_by_name_and_mirrors_the_reference_state_dict(mt, golden_dir):
    meta = json.load(open(os.path.join(golden_dir, 'deep14_meta.json')))[mt]
    m = build(mt)
    sd = m.state_dict()
    got = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()]
    assert got == meta['keys']
    assert len(sd) == meta['entries'] and sum(v.numel() for v in sd.values()) == meta['elements']
    assert models.MODEL_IDS[mt] == {D.GRU14: 10, D.TRF14: 11}[mt]
    # feature_type is taken and ignored, classes_num does not reach AttBlock(2048, 25)
    other = getattr(models, mt)(*P16, 10, 'gamma')
    assert other.feature_type == 'logmel' and other.classes_num == 25
    assert other.att_block.att.weight.shape == (25, 2048, 1)


@pytest.mark.parametrize('mt', MODELS)
def test_strict_load_and_refusal_of_a_9_layer_key_set(mt):
    m = build(mt)
    sd = m.state_dict()
    w = synth.make_state_dict(mt, seed=synth.DEEP14_GOLDEN_SEEDS[mt])
    assert set(w) < set(sd)
    for k, v in w.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    nine = {D.GRU14: 'Cnn_9layers_Gru_FrameAtt', D.TRF14: 'Cnn_9layers_Transformer_FrameAtt'}[mt]
    sd9 = dict(sd)
    for k, v in synth.make_state_dict(nine, seed=0).items():
        sd9[k] = torch.from_numpy(np.asarray(v))
    for k in [k for k in sd9 if k.startswith(('conv_block5', 'conv_block6'))]:
        del sd9[k]
    with pytest.raises(RuntimeError):
        m.load_state_dict(sd9, strict=True)


def test_geometry_closed_form():
    """T -> (T5, out_frames) over T = 31 .. 2100 against the reference's rule:
    five floor halvings, x32, pad to a multiple of 100 unless exactly 1000."""
    for T in range(31, 2101):
        t = T
        for _ in range(5):
            t //= 2
        n = 32 * t
        frames = n if n == 1000 else -(-n // 100) * 100
        assert D.geometry(T) == (t, frames) == (T // 32, frames), T
    assert D.geometry(1001) == (31, 1000) and D.geometry(66) == (2, 100) and D.geometry(31)[0] == 0


@pytest.mark.parametrize('mt', MODELS)
def test_cpu_tensors_and_train_mode_raise(mt):
    m = build(mt)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16000))                 # train mode
    m.eval()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16000))                 # a CPU tensor: no fallback


def test_abi_and_enum_values():
    hdr = open(os.path.join(os.path.dirname(PKG), 'include', 'sedx.h')).read()
    assert '#define SEDX_ABI_VERSION 6' in hdr
    assert 'SEDX_MODEL_GRU14_FRAMEATT = 10' in hdr and 'SEDX_MODEL_TRANSFORMER14_FRAMEATT = 11' in hdr
    L = _lib.lib()
    assert L.sedx_abi_version() == 6
    # sedx_create needs no device: both ids make a handle, gamma features are refused; 9 stays unassigned
    # (tests/test_conformer_cpu.py probes it as the first unknown id) and 12 is the next unknown one
    for mid, feature, want in ((10, 0, 0), (11, 0, 0), (10, 1, 1), (11, 1, 1), (9, 0, 1), (12, 0, 1)):
        cfg = _lib.SedxConfig()
        cfg.model_type, cfg.feature_type = mid, feature
        cfg.sample_rate, cfg.window_size, cfg.hop_size, cfg.mel_bins = 16000, 512, 160, 64
        cfg.fmin, cfg.fmax, cfg.classes_num = 25.0, 7000.0, 25
        h = ctypes.c_void_p()
        assert L.sedx_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == want, (mid, feature)
        if h:
            fr, sl, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
            # the size queries reject what the forward rejects (31 frames), and answer from 32 on
            assert L.sedx_output_geometry(h, 30 * 160, ctypes.byref(fr), ctypes.byref(sl)) == 1
            assert L.sedx_workspace_size(h, 2, 30 * 160, ctypes.byref(nb)) == 1
            assert L.sedx_output_geometry(h, 160000, ctypes.byref(fr), ctypes.byref(sl)) == 0
            assert (fr.value, sl.value) == (1000, 31)
            assert L.sedx_workspace_size(h, 2, 160000, ctypes.byref(nb)) == 0 and nb.value > 0
            L.sedx_destroy(h)


@pytest.mark.parametrize('T5,n', [(1, 16), (5, 3)])
def test_emulated_gru_order_is_the_gru_step(T5, n):
    """deep14_refs.emulate_gru14 (the library's summation order in fp32, the
    e_alg of tests/test_gpu_deep14_seq.py) computes the float64 step: both
    directions' sampled frames within fp32 rounding of it (outputs <= 1; the
    2048-term chains round at most 2048 2^-24 relative, far above what is seen)."""
    s64 = D.state(D.GRU14, torch.float64)
    x = torch.rand(2, 2048, T5, generator=torch.Generator().manual_seed(T5))
    with torch.no_grad():
        r = D.step_seq(s64, D.GRU14, x.double())
    fwd, rev = D.emulate_gru14(s64, x, 1, n)
    k = min(n, T5)
    assert fwd.shape == rev.shape == (k, 1024) and fwd.dtype == torch.float32
    e = max(float((fwd.double() - r[1, :k, :1024]).abs().max()), float((rev.double() - r[1, T5 - k:, 1024:]).abs().max()))
    print('emulated order vs float64: max|d| = %.3g' % e)
    assert 0 < e <= 1e-5


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_side_under_sanitizers():
    r = subprocess.run(['make', '-s', '-C', PKG, 'asan-deep14'], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert 'deep14_driver: clean' in out and 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out, out[-4000:]
