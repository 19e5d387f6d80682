"""HIP path of the two Conformer models (Cnn_9layers_Conformer_FrameAtt,
_FrameAvg): goldens the reference produced (tools/make_golden_conformer.py),
the exact structure of the outputs, every encoder sublayer and each head in
isolation against its float64 restatement (tests/conformer_refs.py) with the
yardstick of tests/test_gpu_layers.py, batch invariance, the fp32 encoder under
the split-bf16 mode, the windowed driver, the graphed forward."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import conformer_refs as CR
import test_gpu_layers as TL
from sedx import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the project's bar against the reference (tests/test_gpu_parity.py)
KEYS = CR.KEYS
MODEL_IDS = [CR.IDS[mt] for mt in CR.MODELS]
WINO = ('winograd', 2)      # the default form, in tests/test_gpu_layers.py's naming


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


# ---------------------------------------------------------------------------
# models, forwards, captures
# ---------------------------------------------------------------------------
_MODELS, _SD = {}, {}


def build(mt, prec='winograd', C=25, keep=True):
    """The model with ``synth`` weights of the golden seed."""
    from sedx import models
    key = (mt, prec, C)
    if key in _MODELS:
        return _MODELS[key]
    m = getattr(models, mt)(*CR.P16, C)
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, classes_num=C, seed=CR.SEEDS[mt]).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    m = m.to('cuda').eval().set_precision(prec)
    if keep:
        _MODELS[key] = m
    return m


def states(mt, C=25):
    """(float64, float32) state dicts of the restatement."""
    if (mt, C) not in _SD:
        _SD[(mt, C)] = (CR.state(mt, C, dtype=torch.float64), CR.state(mt, C, dtype=torch.float32))
    return _SD[(mt, C)]


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


def out_frames(T3):
    n = 8 * T3
    return n if n == 1000 or n % 100 == 0 else n + 100 - n % 100


def forward_features(m, x):
    """One forward of features x [B, 64, T] (cuda) through sedx_forward_features."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B, _, T = x.shape
    C, T3 = m.classes_num, T // 8
    fw = torch.full((B, out_frames(T3), C), float('nan'), dtype=torch.float32, device=x.device)
    clip = torch.full((B, C), float('nan'), dtype=torch.float32, device=x.device)
    emb = torch.full((B, 144, T3), float('nan'), dtype=torch.float32, device=x.device)
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


def capture(m, stage, fwd, shape):
    """Capture id ``stage`` of the forward ``fwd()``: [B, T3, 512] for stage 8,
    [B, T3, 144] for 9 and 20..32."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    buf = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(L.sedx_set_capture(nat.h, stage, _p(buf), buf.numel() * 4), nat.h, 'set_capture')
    try:
        fwd()
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'set_capture')
    m.check_error()
    a = buf.cpu()
    assert torch.isfinite(a).all(), 'stage %d' % stage
    return a


def capture_features(m, stage, x):
    B, _, T = x.shape
    return capture(m, stage, lambda: forward_features(m, x), (B, T // 8, 512 if stage == 8 else 144))


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
@pytest.mark.parametrize('mt', CR.MODELS, ids=MODEL_IDS)
def test_goldens(mt, prec, kind, golden_dir):
    g = np.load(os.path.join(golden_dir, 'conformer_%s.npz' % mt))
    out = run(build(mt, prec), _waves(kind))
    for k in KEYS:
        ref = g['%s_%s' % (kind, k)]
        scale = max(1.0, float(np.abs(ref).max())) if k == 'embedding' else 1.0
        e = err(out[k], ref)
        print(mt, prec, kind, k, 'max|d| = %.3g (scale %.3g)' % (e, scale))
        assert e <= TOL * scale


# ---------------------------------------------------------------------------
# 2. exact structure
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', CR.MODELS, ids=MODEL_IDS)
def test_output_structure(mt):
    m = build(mt)
    out = run(m, _waves('short'))
    w = torch.from_numpy(_waves('short')).cuda()
    fw, clip, emb = out['framewise_output'], out['clipwise_output'], out['embedding']
    assert fw.shape == (2, 100, 25) and clip.shape == (2, 25) and emb.shape == (2, 144, 4)
    assert m.output_geometry(5280) == (100, 4)
    assert np.array_equal(fw[:, :32], np.repeat(fw[:, 0:32:8], 8, axis=1))        # the x8 repeat
    assert np.array_equal(fw[:, 32:], np.repeat(fw[:, 31:32], 68, axis=1))        # padded with the last frame
    assert not np.array_equal(fw[:, 0], fw[:, 8])
    if mt == CR.CAVG:
        # the mean over the 100 stored frames (8 x 4 values + 68 x the last),
        # not over the 32: one rounding of a float64 sum
        mean = fw.astype(np.float64).mean(axis=1)
        ulp = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
        d = np.abs(clip.astype(np.float64) - mean)
        print('cavg clipwise vs float64 mean of its 100 frames: max %.3g ulp' % float((d / ulp).max()))
        assert (d <= 2 * ulp).all()
        unpadded = fw[:, :32].astype(np.float64).mean(axis=1)
        assert (np.abs(clip - unpadded) > 8 * ulp).any()
    with torch.no_grad():
        s9 = capture(m, 9, lambda: m(w), (2, 4, 144))
    assert np.array_equal(emb, s9.numpy().transpose(0, 2, 1))


# ---------------------------------------------------------------------------
# 3. sublayers in isolation
# ---------------------------------------------------------------------------
# T3 = 1 (a single key), 2 (shorter than the 7-tap conv; the j = i + 1 zero),
# 9, 65 and 129 (one past a 64-key chunk / a 128-frame head chunk)
STEP_SHAPES = [(B, T) for T in (8, 16, 72, 520, 1032) for B in (1, 3)]


@pytest.mark.parametrize('B,T', STEP_SHAPES, ids=['B%d-T%d' % s for s in STEP_SHAPES])
def test_sublayers_in_isolation(B, T):
    """Every consecutive pair of capture ids (8 -> 20, 20 -> 21, ..., 31 -> 32)
    and the head (9 -> outputs): R the float64 restatement of the step on the
    GPU's own captured input, e_cpu the fp32 CPU restatement's distance from
    R; max|G - R| <= 4 max(e_cpu, 2^-23 max|R|) (tests/test_gpu_layers.py,
    c = 4 of every non-conv step)."""
    ck = TL.Checks('conformer', WINO)
    x = feats(B, T)
    for mt in CR.MODELS:
        m = build(mt)
        s64, s32 = states(mt)
        caps = {i: capture_features(m, i, x) for i in (8, 9) + CR.ACT_IDS}
        assert torch.equal(caps[32], caps[9])
        for src, dst in CR.STEPS:
            with torch.no_grad():
                r = CR.step(s64, src, caps[src].double())
                f = CR.step(s32, src, caps[src])
            ck.check('%s-B%d-T%d-%d->%d' % (CR.IDS[mt], B, T, src, dst), caps[dst], r, f, c=4)
        outs = run_features(m, x)
        with torch.no_grad():
            r, f = CR.head(s64, mt, caps[9].double()), CR.head(s32, mt, caps[9])
        assert outs['framewise_output'].shape == (B, out_frames(T // 8), 25) == tuple(r['framewise_output'].shape)
        for k in ('framewise_output', 'clipwise_output'):
            ck.check('%s-B%d-T%d-head-%s' % (CR.IDS[mt], B, T, k.split('_')[0]), outs[k], r[k], f[k], c=4)
        assert np.array_equal(outs['embedding'], caps[9].numpy().transpose(0, 2, 1))
    ck.done()


@pytest.mark.parametrize('C', [1, 33, 65])
def test_fc_head_class_counts(C):
    """FrameAvg's head at 1, 33 and 65 classes (one past the 32-class chunk,
    one past the 64-row projection tile)."""
    ck = TL.Checks('conformer-head', WINO)
    m = build(CR.CAVG, C=C, keep=False)
    s64, s32 = states(CR.CAVG, C)
    for B, T in ((1, 8), (3, 72), (3, 1032)):
        x = feats(B, T)
        s9 = capture_features(m, 9, x)
        outs = run_features(m, x)
        with torch.no_grad():
            r, f = CR.head(s64, CR.CAVG, s9.double()), CR.head(s32, CR.CAVG, s9)
        assert outs['framewise_output'].shape == (B, out_frames(T // 8), C)
        for k in ('framewise_output', 'clipwise_output'):
            ck.check('cavg-C%d-B%d-T%d-%s' % (C, B, T, k.split('_')[0]), outs[k], r[k], f[k], c=4)
        fw = outs['framewise_output']
        assert np.array_equal(fw[:, 8 * (T // 8):], np.repeat(fw[:, 8 * (T // 8) - 1:8 * (T // 8)],
                                                              fw.shape[1] - 8 * (T // 8), axis=1))
    ck.done()


# ---------------------------------------------------------------------------
# 4. batch invariance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('T', [72, 520], ids=['T3-9', 'T3-65'])
@pytest.mark.parametrize('mt', CR.MODELS, ids=MODEL_IDS)
def test_batch_invariance(mt, T):
    """Clip k of a batch of 5 equals the same clip run alone, bit for bit:
    also no depthwise tap and no attention key crosses a clip boundary."""
    m = build(mt)
    x = feats(5, T)
    five = run_features(m, x)
    for k in (0, 2, 4):
        one = run_features(m, x[k:k + 1].contiguous())
        for key in KEYS:
            assert np.array_equal(five[key][k:k + 1], one[key]), (k, key)


# ---------------------------------------------------------------------------
# 5. precision: the encoder is fp32 in every mode
# ---------------------------------------------------------------------------
def test_encoder_is_fp32_under_x3():
    """set_precision('x3'): stage 8 -> 9 (the whole encoder) on the GPU's own
    stage 8 still meets the fp32 yardstick of check 3."""
    ck = TL.Checks('conformer-x3', ('x3', None))
    m = build(CR.CATT, 'x3')
    s64, s32 = states(CR.CATT)
    x = feats(3, 72)
    s8, s9 = capture_features(m, 8, x), capture_features(m, 9, x)
    with torch.no_grad():
        r, f = CR.encoder(s64, s8.double()), CR.encoder(s32, s8)
    ck.check('catt-x3-8->9', s9, r, f, c=4)
    # the 144-wide head projection is fp32 too
    with torch.no_grad():
        hr, hf = CR.head(s64, CR.CATT, s9.double()), CR.head(s32, CR.CATT, s9)
    outs = run_features(m, x)
    for k in ('framewise_output', 'clipwise_output'):
        ck.check('catt-x3-head-%s' % k.split('_')[0], outs[k], hr[k], hf[k], c=4)
    ck.done()


# ---------------------------------------------------------------------------
# 6. drivers
# ---------------------------------------------------------------------------
def test_windowed_driver_and_events(golden_dir):
    """predict.py driver, 5 s windows, 1 s stride on
    Cnn_9layers_Conformer_FrameAtt: 496-frame windows padded to 500."""
    from sedx import inference
    g = np.load(os.path.join(golden_dir, 'conformer_windowed.npz'))['merged_5_1']
    ev = json.load(open(os.path.join(golden_dir, 'conformer_events.json')))
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    m = build(CR.CATT)
    audio = torch.from_numpy(synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)[:1]).cuda()
    merged = inference.predict_windows(m, audio, 5, 1, overlap=True).cpu().numpy()
    assert merged.shape == g.shape == (1, 1000, 25)
    e = err(merged, g)
    print('windowed 5/1 max|d| =', e)
    assert e <= TOL
    for which in ('default', 'synthetic'):
        assert inference.events_from_framewise(merged, tables['params_' + which]) == ev[which], which


@pytest.mark.parametrize('mt', CR.MODELS, ids=MODEL_IDS)
def test_graphed_forward_matches_eager(mt):
    """The HIP-graph path captures the whole forward (the r / r_k tables
    included: no host work inside it): the same bits."""
    from sedx import inference
    m = build(mt)
    w = torch.from_numpy(_waves('short')).cuda()
    with torch.no_grad():
        eager = {k: v.clone() for k, v in m(w).items()}
    out = inference.GraphedForward(m, w)(w)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], eager[k]), k


# ---------------------------------------------------------------------------
# 7. too-short input
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', CR.MODELS, ids=MODEL_IDS)
def test_seven_frames_raise(mt):
    m = build(mt)
    with pytest.raises(RuntimeError):
        forward_features(m, feats(2, 7))
    torch.cuda.synchronize()
    run_features(m, feats(2, 8))                # and the handle still works
