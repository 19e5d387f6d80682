"""HIP path of the five other 9-layer models (Cnn_9layers_FrameMax, _FrameAvg,
_FrameAtt, _Gru_FrameAvg, _Transformer_FrameAvg): goldens the reference
produced (tools/make_golden_family.py), the exact structure of the outputs,
the fc head in isolation against its float64 restatement
(tests/family_refs.py) with the yardstick of tests/test_gpu_layers.py, reuse of
the trunk and sequence kernels bit for bit, the windowed driver and batch
invariance."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import family_refs as FR
import test_gpu_layers as TL
from oracle import layer_refs as R
from sedx import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the project's bar against the reference (tests/test_gpu_parity.py)
GRU, TRF = R.GRU, R.TRF
KEYS = FR.KEYS
FAMILY_IDS = [FR.IDS[mt] for mt in FR.FAMILY]
WINO = ('winograd', 2)      # the default form, in tests/test_gpu_layers.py's naming


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


# ---------------------------------------------------------------------------
# models and forwards
# ---------------------------------------------------------------------------
_MODELS = {}


def ctor_args(mt, C):
    if mt in (GRU, TRF):
        return FR.P16 + (C, 'logmel')
    return FR.ctor_args(mt, C)


def build(mt, prec='winograd', C=25, seed=None, keep=True):
    """The model with ``synth`` weights (the golden seed by default)."""
    from sedx import models
    seed = synth.GOLDEN_SEEDS[mt] if seed is None else seed
    key = (mt, prec, C, seed)
    if key in _MODELS:
        return _MODELS[key]
    m = getattr(models, mt)(*ctor_args(mt, C))
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, classes_num=C, seed=seed).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    m = m.to('cuda').eval().set_precision(prec)
    if keep:
        _MODELS[key] = m
    return m


def run(m, wave):
    with torch.no_grad():
        out = m(torch.as_tensor(np.asarray(wave), dtype=torch.float32).cuda())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    m.check_error()
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k
    return out


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def forward_features(m, x):
    """One forward of features x [B, 64, T] (cuda) through
    sedx_forward_features, which every handle accepts."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B, _, T = x.shape
    C, T3 = m.classes_num, T // 8
    frames = 8 * T3
    if m._model_name == GRU and frames != 1000 and frames % 100:
        frames += 100 - frames % 100
    fw = torch.full((B, frames, C), float('nan'), dtype=torch.float32, device=x.device)
    clip = torch.full((B, C), float('nan'), dtype=torch.float32, device=x.device)
    emb = torch.full((B, C, T3) if m._embedding_cla else (B, 512, T3), float('nan'), dtype=torch.float32,
                     device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(L.sedx_forward_features(nat.h, _p(x), B, T, _p(fw), _p(clip), _p(emb), None, 0, stream),
               nat.h, 'forward_features')
    return {'framewise_output': fw, 'clipwise_output': clip, 'embedding': emb}


def run_features(m, x):
    out = forward_features(m, x)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    m.check_error()
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k      # every element was written
    return out


def capture(m, stage, x):
    """Stage 8 / 9 of a features forward, in the oracle's layout."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B, _, T = x.shape
    buf = torch.full(R.capture_shape(stage, B, T), float('nan'), dtype=torch.float32, device=x.device)
    _lib.check(L.sedx_set_capture(nat.h, stage, _p(buf), buf.numel() * 4), nat.h, 'set_capture')
    try:
        forward_features(m, x)
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'set_capture')
    m.check_error()
    a = buf.cpu()
    assert torch.isfinite(a).all(), 'stage %d' % stage
    return R.from_capture(stage, a)


def feats(B, T):
    return torch.from_numpy(TL.feats(B, T)).cuda()


def _waves(kind):
    if kind == 'short':
        return synth.make_waveforms(2, seconds=5280 / 16000., sample_rate=16000, seed=11)
    if kind == 'ragged':
        return synth.make_waveforms(1, seconds=7777 / 16000., sample_rate=16000, seed=12)
    return synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)[:1]


# ---------------------------------------------------------------------------
# 1. goldens
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['short', 'ragged', 'clip10s'])
@pytest.mark.parametrize('prec', ['winograd', 'exact'])
@pytest.mark.parametrize('mt', FR.FAMILY, ids=FAMILY_IDS)
def test_goldens(mt, prec, kind, golden_dir):
    g = np.load(os.path.join(golden_dir, 'family_%s.npz' % mt))
    out = run(build(mt, prec), _waves(kind))
    for k in KEYS:
        ref = g['%s_%s' % (kind, k)]
        scale = max(1.0, float(np.abs(ref).max())) if (k == 'embedding' and ref.shape[1] == 512) else 1.0
        e = err(out[k], ref)
        print(mt, prec, kind, k, 'max|d| = %.3g (scale %.3g)' % (e, scale))
        assert e <= TOL * scale


# ---------------------------------------------------------------------------
# 2. exact structure
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', FR.FAMILY, ids=FAMILY_IDS)
def test_output_structure(mt):
    out = run(build(mt), _waves('short'))
    fw, clip, emb = out['framewise_output'], out['clipwise_output'], out['embedding']
    assert fw.shape == (2, 32, 25) and clip.shape == (2, 25)
    for j in range(1, 8):                                   # the x8 repeat
        assert np.array_equal(fw[:, j::8], fw[:, ::8]), j
    if mt == FR.FMAX:
        assert np.array_equal(clip, fw.max(axis=1))
    if mt == FR.FATT:
        assert emb.shape == (2, 25, 4)
        assert np.array_equal(emb, fw[:, ::8].transpose(0, 2, 1))
    else:
        assert emb.shape == (2, 512, 4)


def test_gru_frameavg_is_not_padded_to_100():
    """7777 samples: 48 frames (models.py:551), where Cnn_9layers_Gru_FrameAtt
    returns 100 (:678-681)."""
    out = run(build(FR.GAVG), _waves('ragged'))
    assert out['framewise_output'].shape == (1, 48, 25)
    assert out['embedding'].shape == (1, 512, 6)
    assert build(FR.GAVG).output_geometry(7777) == (48, 6)


# ---------------------------------------------------------------------------
# 3. the head in isolation
# ---------------------------------------------------------------------------
# T = 8: one sequence frame; 1032: 129 frames, one past fc_head_kernel's (and
# att_head_kernel's) 128-frame staging chunk
HEAD_SHAPES = [(B, T) for T in (8, 72, 1032) for B in (1, 3)]
HEAD_CASES = [(mt, C) for mt in FR.FC_MODELS for C in (1, 25, 33, 64, 65)] + [(FR.FATT, 25)]


def _head_refs(mt, C, s9):
    s64 = FR.state(mt, C, dtype=torch.float64)
    s32 = FR.state(mt, C, dtype=torch.float32)
    with torch.no_grad():
        return s64, FR.head(s64, mt, s9.double()), FR.head(s32, mt, s9)


@pytest.mark.parametrize('mt,C', HEAD_CASES, ids=['%s-C%d' % (FR.IDS[mt], C) for mt, C in HEAD_CASES])
def test_head_in_isolation(mt, C):
    """Stage 9 -> outputs: R the float64 head on the GPU's own stage 9, e_cpu
    the fp32 CPU head's distance from R; max|G - R| <= 4 max(e_cpu, 2^-23
    max|R|) (tests/test_gpu_layers.py, c = 4 of every non-conv step)."""
    ck = TL.Checks('family-head', WINO)
    m = build(mt, C=C, keep=C == 25)
    for B, T in HEAD_SHAPES:
        x = feats(B, T)
        s9 = capture(m, 9, x)
        outs = run_features(m, x)
        _, r, f = _head_refs(mt, C, s9)
        T3 = T // 8
        assert outs['framewise_output'].shape == (B, 8 * T3, C) == tuple(r['framewise_output'].shape)
        assert outs['clipwise_output'].shape == (B, C)
        for k in ('framewise_output', 'clipwise_output'):
            ck.check('%s-C%d-B%d-T%d-%s' % (FR.IDS[mt], C, B, T, k.split('_')[0]), outs[k], r[k], f[k], c=4)
        fw = outs['framewise_output']
        assert np.array_equal(fw, np.repeat(fw[:, ::8], 8, axis=1))
        if mt == FR.FMAX:
            assert np.array_equal(outs['clipwise_output'], fw.max(axis=1))
        if mt == FR.FATT:
            assert np.array_equal(outs['embedding'], fw[:, ::8].transpose(0, 2, 1))
        else:                                   # the head's input transposed: no arithmetic
            assert np.array_equal(outs['embedding'], s9.numpy().transpose(0, 2, 1))
    ck.done()


@pytest.mark.parametrize('mt', FR.FC_MODELS, ids=[FR.IDS[mt] for mt in FR.FC_MODELS])
def test_head_in_isolation_x3(mt):
    """Split-bf16 projection: max|G - R| <= 2^-15 S per element, S the float64
    step on |input|, |weight| and |bias| (tests/test_gpu_layers.py)."""
    form = ('x3', None)
    ck = TL.Checks('family-head', form)
    m = build(mt, 'x3')
    x = feats(3, 72)
    s9 = capture(m, 9, x)
    outs = run_features(m, x)
    s64, r, f = _head_refs(mt, 25, s9)
    with torch.no_grad():
        hb = FR.absbound_head(s64, mt, s9.double())
    for k in ('framewise_output', 'clipwise_output'):
        ck.check('%s-%s' % (FR.IDS[mt], k.split('_')[0]), outs[k], r[k], f[k], abs_bound=TL.X3_REL * hb[k])
    ck.done()


@pytest.mark.parametrize('mt', FR.FAMILY, ids=FAMILY_IDS)
def test_seven_frames_raise(mt):
    """Fewer than 8 frames leave nothing after the three pools: a loud error,
    as for the FrameAtt models."""
    m = build(mt)
    with pytest.raises(RuntimeError):
        forward_features(m, feats(2, 7))
    torch.cuda.synchronize()
    run_features(m, feats(2, 8))                # and the handle still works


# ---------------------------------------------------------------------------
# 4. reuse is real
# ---------------------------------------------------------------------------
def test_trunk_and_sequence_layers_are_the_same_kernels():
    """Same trunk (and sequence) weights, B = 3, T = 72: the new models'
    stage 8 / stage 9 are the FrameAtt models' bit for bit."""
    x = feats(3, 72)
    seed = 0
    gru8, gru9 = (capture(build(GRU, seed=seed), st, x) for st in (8, 9))
    favg = build(FR.FAVG, seed=seed)
    favg8 = capture(favg, 8, x)
    assert torch.equal(favg8, gru8)
    # no sequence layer: stage 9 is the head's input, the stage-8 buffer
    assert torch.equal(capture(favg, 9, x), favg8.transpose(1, 2))
    assert torch.equal(capture(build(FR.GAVG, seed=seed), 9, x), gru9)
    assert torch.equal(capture(build(FR.TAVG, seed=seed), 9, x), capture(build(TRF, seed=seed), 9, x))
    assert not torch.equal(gru9, gru8.transpose(1, 2))


# ---------------------------------------------------------------------------
# 5. drivers
# ---------------------------------------------------------------------------
def test_windowed_driver_and_events(golden_dir):
    """predict.py driver, 5 s windows, 1 s stride on Cnn_9layers_Gru_FrameAvg:
    496-frame windows of a GRU model (no pad to 500)."""
    from sedx import inference
    g = np.load(os.path.join(golden_dir, 'family_windowed.npz'))['merged_5_1']
    ev = json.load(open(os.path.join(golden_dir, 'family_events.json')))
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    m = build(FR.GAVG)
    audio = torch.from_numpy(synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)[:1]).cuda()
    merged = inference.predict_windows(m, audio, 5, 1, overlap=True).cpu().numpy()
    assert merged.shape == g.shape == (1, 996, 25)
    e = err(merged, g)
    print('windowed 5/1 max|d| =', e)
    assert e <= TOL
    for which in ('default', 'synthetic'):
        assert inference.events_from_framewise(merged, tables['params_' + which]) == ev[which], which


def test_graphed_forward_matches_eager():
    """The HIP-graph path goes through the handle: the same bits."""
    from sedx import inference
    m = build(FR.FAVG)
    w = torch.from_numpy(_waves('short')).cuda()
    with torch.no_grad():
        eager = {k: v.clone() for k, v in m(w).items()}
    out = inference.GraphedForward(m, w)(w)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], eager[k]), k


# ---------------------------------------------------------------------------
# 6. batch invariance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', [FR.FMAX, FR.GAVG], ids=['fmax', 'gavg'])
def test_batch_invariance(mt):
    """Clip 0 alone = clip 0 inside a batch of 3, bit for bit (3 clips keep
    the GRU on its small-batch kernel)."""
    m = build(mt)
    w = synth.make_waveforms(3, seconds=5280 / 16000., sample_rate=16000, seed=21)
    three, one = run(m, w), run(m, w[:1])
    for k in KEYS:
        assert np.array_equal(three[k][:1], one[k]), k
