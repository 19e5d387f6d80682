"""HIP path of Cnn14_DecisionLevelAtt: goldens the reference produced
(tools/make_golden_cnn14.py) at 25 classes / 16 kHz and 527 classes / 32 kHz,
the windowed driver and its events, the fused pooling + fc1 launch
(csrc/decision.hip) in isolation against its float64 restatement
(tests/cnn14_refs.py) with the yardstick of tests/test_gpu_layers.py and its
documented summation order bit for bit, the head at 25 / 33 / 527 classes,
batch / run / graph / workspace bit-identity, fp32 under the split-bf16 mode,
and the rejections.

Layer yardstick (tests/test_gpu_layers.py unchanged): max|G - R| <=
4 max(e_cpu, e_alg, floor), R the float64 step on the GPU's own previous stage,
e_cpu the fp32 CPU step's distance from R, e_alg that of the CPU fp32 emulation
of the kernel's order (four in-order chains of 512 terms, summed in order) at
the sampled outputs, where the kernel's values equal the emulation bit for bit.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import cnn14_refs as C
import test_gpu_layers as TL
from sedx import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the project's bar against the reference (tests/test_gpu_parity.py)
KEYS = C.KEYS
MT = C.CNN14
WINO = ('winograd', 2)
EINVAL = 1


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


# ---------------------------------------------------------------------------
# models, forwards, captures
# ---------------------------------------------------------------------------
_MODELS, _SD = {}, {}
PRESET = {25: C.P16, 33: C.P16, 527: C.P32}     # one model per class count (the feature forwards skip the frontend)


def build(classes=25, prec='winograd'):
    from sedx import models
    if classes not in _MODELS:
        m = getattr(models, MT)(*PRESET[classes], classes)
        sd = m.state_dict()
        for k, v in synth.make_state_dict(MT, classes_num=classes, seed=C.SEED).items():
            sd[k] = torch.from_numpy(v)
        m.load_state_dict(sd, strict=True)
        _MODELS[classes] = m.to('cuda').eval()
    return _MODELS[classes].set_precision(prec)


def states(classes=25):
    """(float64, float32) tensors of the steps restated here: fc1 and the AttBlock."""
    if classes not in _SD:
        w = {k: torch.from_numpy(np.asarray(v)) for k, v in
             synth.make_state_dict(MT, classes_num=classes, seed=C.SEED).items() if k.startswith(('fc1.', 'att_block.'))}
        _SD[classes] = ({k: (v.double() if v.is_floating_point() else v) for k, v in w.items()}, w)
    return _SD[classes]


def run(m, wave):
    with torch.no_grad():
        out = m(torch.as_tensor(np.asarray(wave), dtype=torch.float32).cuda())
    torch.cuda.synchronize()
    assert sorted(out) == sorted(KEYS)           # the reference's two keys, no 'embedding'
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k
    return out


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def forward_features(m, x, ws=None, ws_bytes=0):
    """One forward of features x [B, 64, T] (cuda) through sedx_forward_features; d_embedding NULL."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B, _, T = x.shape
    geo = C.geometry(T)
    frames = geo[1] if geo else 32
    cn = m.classes_num
    fw = torch.full((B, frames, cn), float('nan'), dtype=torch.float32, device=x.device)
    clip = torch.full((B, cn), float('nan'), dtype=torch.float32, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(L.sedx_forward_features(nat.h, _p(x), B, T, _p(fw), _p(clip), None,
                                       _p(ws) if ws is not None else None, ws_bytes, stream),
               nat.h, 'forward_features')
    return {'framewise_output': fw, 'clipwise_output': clip}


def run_features(m, x, **kw):
    out = forward_features(m, x, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k      # every element was written, the pad frames included
    return out


def capture(m, stage, fwd, shape):
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
    a = buf.cpu()
    assert torch.isfinite(a).all(), 'stage %d' % stage
    return a


def capture_features(m, stage, x):
    """Stage 43 or 9 of a feature forward, [B, T5, 2048]."""
    B, _, T = x.shape
    return capture(m, stage, lambda: forward_features(m, x), (B, T // 32, 2048))


def feats(B, T):
    return torch.from_numpy(TL.feats(B, T)).cuda()


def _waves(kind, sr=16000):
    if kind == 'short':
        return synth.make_waveforms(2, seconds=10400 / 16000., sample_rate=sr, seed=11)
    if kind == 'ragged':
        return synth.make_waveforms(1, seconds=7777 / 16000., sample_rate=sr, seed=12)
    return synth.make_waveforms(2, seconds=10.0, sample_rate=sr, seed=1234)[:1]


def _stage_goldens(m, g, w, tag):
    """Stages 43 and 9 within 1e-4 x the stage's scale (test_stage_goldens' rule)."""
    w = torch.from_numpy(w).cuda()
    with torch.no_grad():
        for stage, key in ((43, 'short_seq_in'), (9, 'short_seq_out')):
            a = capture(m, stage, lambda: m(w), (2, 2, 2048)).numpy()
            scale = max(1.0, float(np.abs(g[key]).max()))
            e = err(a, g[key])
            print(tag, 'stage', stage, 'max|d| = %.3g (scale %.3g)' % (e, scale))
            assert e <= 1e-4 * scale


# ---------------------------------------------------------------------------
# 1. goldens
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['short', 'ragged', 'clip10s'])
@pytest.mark.parametrize('prec', ['winograd', 'exact', 'x3'])
def test_goldens(prec, kind, golden_dir):
    g = np.load(os.path.join(golden_dir, 'cnn14_%s.npz' % MT))
    m = build(25, prec)
    out = run(m, _waves(kind))
    for k in KEYS:
        ref = g['%s_%s' % (kind, k)]
        e = err(out[k], ref)
        print(prec, kind, k, 'max|d| = %.3g' % e)
        assert e <= TOL
    if kind == 'short':
        _stage_goldens(m, g, _waves(kind), prec)


def test_golden_audioset_preset_527_classes(golden_dir):
    """(32000, 1024, 320, 64, 50, 14000), 527 classes: 2 x 20800 samples, T = 66, 65 frames."""
    g = np.load(os.path.join(golden_dir, 'cnn14_audioset.npz'))
    m = build(527)
    w = synth.make_waveforms(2, seconds=20800 / 32000., sample_rate=32000, seed=11)
    out = run(m, w)
    assert out['framewise_output'].shape == (2, 65, 527) and out['clipwise_output'].shape == (2, 527)
    for k in KEYS:
        e = err(out[k], g['short_' + k])
        print('audioset', k, 'max|d| = %.3g' % e)
        assert e <= TOL
    _stage_goldens(m, g, w, 'audioset')


# ---------------------------------------------------------------------------
# 2. windowed driver and events
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['winograd', 'exact', 'x3'])
def test_windowed_driver_and_events(prec, golden_dir):
    """predict.py driver, 5 s windows at 1 s stride: 480 + 20 frames per window; the event lists of both tables."""
    from sedx import inference
    g = np.load(os.path.join(golden_dir, 'cnn14_windowed.npz'))['merged_5_1']
    ev = json.load(open(os.path.join(golden_dir, 'cnn14_events.json')))
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    m = build(25, prec)
    audio = torch.from_numpy(synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=ev['wave_seed'])[:1]).cuda()
    merged = inference.predict_windows(m, audio, 5, 1, overlap=True).cpu().numpy()
    assert merged.shape == g.shape == (1, 1000, 25)
    e = err(merged, g)
    print('windowed 5/1', prec, 'max|d| =', e)
    assert e <= TOL
    for which in ('default', 'synthetic'):
        assert inference.events_from_framewise(merged, tables['params_' + which]) == ev[which], which


# ---------------------------------------------------------------------------
# 3. the new launch in isolation, and the head on its output
# ---------------------------------------------------------------------------
# T5 = 1, 1, 2, 2, 3, 3, 5, 6 with 0, 30, 0, 30, 0, 30, 0, 7 pad frames; (33, 161): M = 165 rows cross a
# 128-row boundary and every 32-row tile edge falls inside a clip of 5 rows
LAYER_SHAPES = [(B, T) for T in (33, 63, 65, 95, 97, 127, 161, 200) for B in (1, 3)] + [(33, 161)]
EMU_COLS = np.array([0, 1, 15, 16, 17, 511, 512, 1023, 1024, 1300, 2031, 2032, 2046, 2047])


def check_decision(ck, m, x, tag):
    """GPU stage 9 against the float64 step on the GPU's own stage 43; the header's order bit for bit."""
    g64, g32 = states(m.classes_num)
    B, _, T = x.shape
    s43, s9 = capture_features(m, 43, x), capture_features(m, 9, x)
    assert float(s43.min()) >= 0.0                                   # a mean of ReLU outputs
    with torch.no_grad():
        r64 = C.step_decision(g64, s43.double().transpose(1, 2))
        r32 = C.step_decision(g32, s43.transpose(1, 2))
    rows = C.sample_rows(B, T // 32, 6, seed=B + T)
    E = C.emulate_decision(g32['fc1.weight'].numpy(), g32['fc1.bias'].numpy(), s43.numpy(), rows, EMU_COLS)
    got = s9.numpy()[rows[:, 0], rows[:, 1]][:, EMU_COLS]
    nd = int((got != E).sum())
    print('  %sstage 9: kernel vs emulated fp32 order on %d rows x %d outputs: %d of %d values differ'
          % (tag, len(rows), len(EMU_COLS), nd, E.size))
    assert nd == 0, 'the kernel no longer sums in the order its header documents'
    e_alg = float(np.abs(E.astype(np.float64) - r64.numpy()[rows[:, 0], rows[:, 1]][:, EMU_COLS]).max())
    ck.check(tag + 'decision', s9, r64, r32, c=4, e_alg=e_alg)
    return s9


def check_head(ck, m, x, s9, tag):
    """The head on the GPU's own stage 9: shape (B, T - 1, C), pad frames = the last frame."""
    g64, g32 = states(m.classes_num)
    B, _, T = x.shape
    T5, frames = C.geometry(T)
    outs = run_features(m, x)
    fw = outs['framewise_output']
    assert fw.shape == (B, T - 1, m.classes_num) and frames == T - 1
    assert np.array_equal(fw[:, 32 * T5:], np.repeat(fw[:, 32 * T5 - 1:32 * T5], frames - 32 * T5, axis=1))
    assert np.array_equal(fw[:, :32 * T5], np.repeat(fw[:, 0:32 * T5:32], 32, axis=1))
    with torch.no_grad():
        rh, fh = C.step_head(g64, s9.double(), frames), C.step_head(g32, s9, frames)
    for key in KEYS:
        ck.check(tag + 'head-' + key.split('_')[0], outs[key], rh[key], fh[key], c=4)


@pytest.mark.parametrize('B,T', LAYER_SHAPES, ids=['B%d-T%d' % s for s in LAYER_SHAPES])
def test_decision_stage_and_head_in_isolation(B, T):
    ck = TL.Checks('cnn14', WINO)
    m = build(25)
    x = feats(B, T)
    s9 = check_decision(ck, m, x, 'B%d-T%d-' % (B, T))
    check_head(ck, m, x, s9, 'B%d-T%d-' % (B, T))
    ck.done()


@pytest.mark.parametrize('classes', [33, 527])
def test_head_at_other_class_counts(classes):
    """33: a partial second chunk of 32 classes; 527: 17 chunks, nac = 1088."""
    ck = TL.Checks('cnn14-C%d' % classes, WINO)
    m = build(classes)
    for B, T in ((1, 33), (3, 200)):
        x = feats(B, T)
        s9 = check_decision(ck, m, x, 'C%d-B%d-T%d-' % (classes, B, T))
        check_head(ck, m, x, s9, 'C%d-B%d-T%d-' % (classes, B, T))
    ck.done()


# ---------------------------------------------------------------------------
# 4. bit-identity
# ---------------------------------------------------------------------------
def test_batch_run_graph_workspace_identity():
    from sedx import _lib, inference
    m = build(25)
    x = feats(33, 97)                            # T5 = 3: clips straddle the 32-row tiles
    big = run_features(m, x)
    again = run_features(m, x)
    for key in KEYS:
        assert np.array_equal(big[key], again[key]), key                     # a second run
    for i in (0, 10, 32):
        one = run_features(m, x[i:i + 1].contiguous())
        three = run_features(m, torch.stack([x[5], x[i], x[9]]).contiguous())
        for key in KEYS:
            assert np.array_equal(big[key][i:i + 1], one[key]), (i, key)     # alone
            assert np.array_equal(big[key][i], three[key][1]), (i, key)      # at B = 3 in another position
    # both sides of the launch's tile-shape threshold: 32 clips are 96 rows (one column tile per
    # workgroup), 33 clips 99 rows (four)
    low = run_features(m, x[:32].contiguous())
    for key in KEYS:
        assert np.array_equal(big[key][:32], low[key]), key
    # a caller workspace of exactly sedx_workspace_size bytes, 0xFF-filled inside a larger tensor
    L = _lib.lib()
    nat = m.native(x.device)
    xs = x[:3].contiguous()
    need = ctypes.c_size_t()
    # (a logmel handle's size query takes samples: 96 hops are the 97 frames)
    _lib.check(L.sedx_workspace_size(nat.h, 3, 96 * 160, ctypes.byref(need)), nat.h, 'workspace_size')
    buf = torch.full((need.value + 4096,), 0xFF, dtype=torch.uint8, device='cuda')
    own = run_features(m, xs, ws=buf, ws_bytes=need.value)
    cached = run_features(m, xs)
    for key in KEYS:
        assert np.array_equal(own[key], cached[key]), key
    assert bool((buf[need.value:] == 0xFF).all())
    # the HIP-graph path
    w = torch.from_numpy(_waves('short')).cuda()
    with torch.no_grad():
        eager = {k: v.clone() for k, v in m(w).items()}
    out = inference.GraphedForward(m, w)(w)
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(out[key], eager[key]), key


# ---------------------------------------------------------------------------
# 5. precision: the new stage and the head are fp32 in every mode
# ---------------------------------------------------------------------------
def test_new_stages_are_fp32_under_x3():
    ck = TL.Checks('cnn14-x3', ('x3', None))
    m = build(25, 'x3')
    x = feats(3, 97)
    s9 = check_decision(ck, m, x, 'x3-')
    check_head(ck, m, x, s9, 'x3-')
    ck.done()


# ---------------------------------------------------------------------------
# 6. rejections
# ---------------------------------------------------------------------------
def test_short_and_multiple_of_32_inputs_are_rejected_alike():
    from sedx import _lib
    L = _lib.lib()
    m = build(25)
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    fr, sl, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
    for T in (31, 32, 64):
        with pytest.raises(RuntimeError):
            forward_features(m, feats(2, T))
        with pytest.raises(RuntimeError):
            run(m, np.zeros((1, (T - 1) * 160), np.float32))
        # logmel handles: the queries take samples; T frames = T - 1 hops
        assert L.sedx_output_geometry(nat.h, (T - 1) * 160, ctypes.byref(fr), ctypes.byref(sl)) == EINVAL
        assert L.sedx_workspace_size(nat.h, 2, (T - 1) * 160, ctypes.byref(nb)) == EINVAL
        msg = L.sedx_last_error(nat.h)
        assert (b'too short' in msg) if T < 32 else (b'multiple of 32' in msg), msg
    torch.cuda.synchronize()
    for T in (33, 65):                            # and the handle still works
        assert L.sedx_output_geometry(nat.h, (T - 1) * 160, ctypes.byref(fr), ctypes.byref(sl)) == 0
        assert (fr.value, sl.value) == (T - 1, T // 32)
        out = run_features(m, feats(2, T))
        assert out['framewise_output'].shape == (2, T - 1, 25)


def test_a_handle_refuses_the_14_layer_transformer_keys():
    from sedx import models
    m = getattr(models, MT)(*C.P16, 25).to('cuda').eval()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
          synth.make_state_dict('Cnn_14layers_Transformer_FrameAtt', seed=0).items()}
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    with pytest.raises(RuntimeError):
        nat.load(sd)
