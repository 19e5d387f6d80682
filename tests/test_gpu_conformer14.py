"""HIP path of Cnn_14layers_Conformer_FrameAtt: goldens the reference produced
(tools/make_golden_conformer14.py), every encoder step and the head in isolation
against the float64 restatement (tests/conformer14_refs.py) with the yardstick
of tests/test_gpu_layers.py, the head's structure and its documented summation
order bit for bit, batch / run / graph / workspace bit-identity, the fp32 encoder
in every precision mode, the windowed driver with its events, and the refusals.

Layer yardstick (tests/test_gpu_layers.py unchanged): max|G - R| <= 4 max(e_cpu,
floor) per step on the GPU's own previous capture, for every step.  The input
layer sums 2048 terms as four 512-term chains (csrc/conformer.hip); it meets the
unchanged yardstick (largest measured e / max(e_cpu, floor) 2.30 over the 14
shapes), so no exception is recorded for it.  e_alg, the error of the
CPU fp32 emulation of that order (conformer14_refs.emulate_input_layer) on the
same input, is printed beside it: the kernel's worst element is the emulation's.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import conformer14_refs as C14
import test_gpu_layers as TL
from sedx import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the project's bar against the reference (tests/test_gpu_parity.py, test_gpu_deep14.py)
KEYS = C14.KEYS
MT = C14.CF14
WINO = ('winograd', 2)
OK, EINVAL = 0, 1
HOP = 160
PRECISIONS = ['winograd', 'exact', 'x3']


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


# ---------------------------------------------------------------------------
# models, forwards, captures
# ---------------------------------------------------------------------------
_MODELS, _SD, _WAVES = {}, {}, {}


def build(prec='winograd'):
    from sedx import models
    if prec not in _MODELS:
        m = getattr(models, MT)(*C14.P16, 25, 'logmel')
        sd = m.state_dict()
        for k, v in synth.make_state_dict(MT, seed=C14.SEED).items():
            sd[k] = torch.from_numpy(v)
        m.load_state_dict(sd, strict=True)
        _MODELS[prec] = m.to('cuda').eval().set_precision(prec)
    return _MODELS[prec]


def states():
    if not _SD:
        _SD[0] = (C14.state(torch.float64), C14.state(torch.float32))
    return _SD[0]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def _forward(m, x, T, wave, ws=None, ws_bytes=0):
    """One forward through the C ABI into NaN-filled outputs; returns (status, outputs on the device)."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B = x.shape[0]
    T5, _, frames = C14.geometry(T) if 32 <= T < 32032 else (max(T // 32, 1), 0, 1000)
    out = {'framewise_output': _nan(B, frames, 25), 'clipwise_output': _nan(B, 25), 'embedding': _nan(B, 144, T5)}
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    fn = L.sedx_forward if wave else L.sedx_forward_features
    st = fn(nat.h, _p(x), B, x.shape[1] if wave else T, _p(out['framewise_output']), _p(out['clipwise_output']),
            _p(out['embedding']), _p(ws), ws_bytes, stream)
    return st, out, nat


def _finish(st, out, nat):
    from sedx import _lib
    _lib.check(st, nat.h, 'forward')
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k      # every element was written over its NaN
    return out


def run_features(m, x, **kw):
    """features x [B, 64, T] (cuda) through sedx_forward_features."""
    return _finish(*_forward(m, x, x.shape[2], False, **kw))


def run_wave(m, wave):
    w = torch.as_tensor(np.asarray(wave), dtype=torch.float32).cuda()
    return _finish(*_forward(m, w, w.shape[1] // HOP + 1, True))


def capture(m, stage, fwd, shape):
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    buf = _nan(*shape)
    _lib.check(L.sedx_set_capture(nat.h, stage, _p(buf), buf.numel() * 4), nat.h, 'set_capture')
    try:
        fwd()
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'set_capture')
    a = buf.cpu()
    assert torch.isfinite(a).all(), 'stage %d' % stage
    return a


def capture_shape(stage, B, T5):
    return (B, T5, 2048) if stage == 43 else (B, T5, 64) if stage == C14.LOGITS else (B, T5, 144)


def capture_features(m, stage, x):
    B, _, T = x.shape
    return capture(m, stage, lambda: run_features(m, x), capture_shape(stage, B, T // 32))


def feats(B, T):
    return torch.from_numpy(TL.feats(B, T)).cuda()


def waves(kind):
    if kind not in _WAVES:
        cases = {'short': (2, 10400, 11), 'ragged': (1, 7777, 12), 't3': (1, 15900, 13), 't128': (1, 655200, 14),
                 'long': (1, 5119840, 15), 'clip10s': (2, 160000, 1234)}
        n, samples, seed = cases[kind]
        w = synth.make_waveforms(n, seconds=samples / 16000., sample_rate=16000, seed=seed)
        assert w.shape == (n, samples)
        _WAVES[kind] = w[:1] if kind == 'clip10s' else w
    return _WAVES[kind]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'conformer14_%s.npz' % MT)))


@pytest.fixture(scope='module')
def meta(golden_dir):
    return json.load(open(os.path.join(golden_dir, 'conformer14_meta.json')))


# ---------------------------------------------------------------------------
# 1. goldens
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['short', 'ragged', 't3', 'clip10s', 't128', 'long'])
@pytest.mark.parametrize('prec', PRECISIONS)
def test_goldens(prec, kind, golden):
    m = build(prec)
    out = run_wave(m, waves(kind))
    for k in KEYS:
        if kind == 'long' and k == 'embedding':
            continue                                   # framewise and clipwise only
        ref = golden['%s_%s' % (kind, k)]
        scale = max(1.0, float(np.abs(ref).max())) if k == 'embedding' else 1.0
        e = err(out[k], ref)
        print(prec, kind, k, 'max|d| = %.3g (scale %.3g)' % (e, scale))
        assert e <= TOL * scale
    if kind == 'short':
        for stage, key, width in ((43, 'short_seq_in', 2048), (9, 'short_seq_out', 144)):
            a = capture(m, stage, lambda: run_wave(m, waves(kind)), (2, 2, width)).numpy()
            scale = max(1.0, float(np.abs(golden[key]).max()))
            e = err(a, golden[key])
            print(prec, 'stage', stage, 'max|d| = %.3g (scale %.3g)' % (e, scale))
            assert e <= 1e-4 * scale


# ---------------------------------------------------------------------------
# 2. layer yardstick
# ---------------------------------------------------------------------------
# T5 = 1 (a single key), 2 (shorter than the 7-tap conv), 3, 9, 33 (one row past the attention core's 32-query
# block), 65 (one past a 64-key chunk), 129 (one past the head's 128-frame chunk)
LAYER_SHAPES = [(B, T5) for T5 in (1, 2, 3, 9, 33, 65, 129) for B in (1, 3)]


def check_steps(ck, prec, B, T5):
    """Every step 43 -> 20 -> ... -> 32 and the head on the GPU's own previous capture."""
    x = feats(B, 32 * T5)
    m = build(prec)
    s64, s32 = states()
    caps = {i: capture_features(m, i, x) for i in (43, 9) + C14.ACT_IDS}
    assert torch.equal(caps[32], caps[9])
    tag = '%s-B%d-T5_%d-' % (prec, B, T5)
    with torch.no_grad():
        for src, dst in C14.STEPS:
            r = C14.step(s64, src, caps[src].double())
            f = C14.step(s32, src, caps[src])
            if src == 43:
                e_alg = float((C14.emulate_input_layer(s64, s32, caps[43]).double() - r).abs().max())
                print('  %s43->20: e_alg (four 512-term chains, emulated) = %.3g' % (tag, e_alg))
            ck.check(tag + '%d->%d' % (src, dst), caps[dst], r, f, c=4)
        outs = run_features(m, x)
        r, f = C14.head(s64, caps[9].double()), C14.head(s32, caps[9])
    assert outs['framewise_output'].shape == (B, C14.geometry(32 * T5)[2], 25) == tuple(r['framewise_output'].shape)
    for k in ('framewise_output', 'clipwise_output'):
        ck.check(tag + 'head-' + k.split('_')[0], outs[k], r[k], f[k], c=4)
    assert np.array_equal(outs['embedding'], caps[9].numpy().transpose(0, 2, 1))


@pytest.mark.parametrize('B,T5', LAYER_SHAPES, ids=['B%d-T5_%d' % s for s in LAYER_SHAPES])
def test_steps_in_isolation(B, T5):
    ck = TL.Checks('conformer14', WINO)
    check_steps(ck, 'winograd', B, T5)
    ck.done()


# ---------------------------------------------------------------------------
# 3. head structure
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('T5', [1, 3, 7, 31, 128, 129])
def test_head_structure_and_stated_order(T5, meta):
    B = 2
    m = build()
    x = feats(B, 32 * T5 + 5)
    out = run_features(m, x)
    fw, clip, emb = out['framewise_output'], out['clipwise_output'], out['embedding']
    ratio = 1000 // T5
    assert fw.shape == (B, meta['frames'][T5 - 1], 25) and clip.shape == (B, 25) and emb.shape == (B, 144, T5)
    assert m.output_geometry((32 * T5 + 4) * HOP) == (meta['frames'][T5 - 1], T5)
    f = np.arange(fw.shape[1])
    src = ratio * np.minimum(f // ratio, T5 - 1)
    assert np.array_equal(fw, fw[:, src])                              # frame f = frame ratio min(f // ratio, T5 - 1)
    if T5 > 1:
        assert not np.array_equal(fw[:, 0], fw[:, ratio])
    s9 = capture_features(m, 9, x)
    assert np.array_equal(emb, s9.numpy().transpose(0, 2, 1))
    lg = capture_features(m, C14.LOGITS, x).numpy()                    # [B, T5, 64]: att | cla | zeros
    assert not lg[:, :, 50:].any()
    tot, want = C14.emulate_clipwise(lg[:, :, :25], fw[:, ::ratio][:, :T5])
    nd = int((clip != want).sum())
    print('T5 %d: clipwise vs the emulated stated order: %d of %d values differ' % (T5, nd, clip.size))
    assert nd == 0, 'the head no longer sums in the order its header documents'
    # the framewise values are sigmoid(cla) of the captured logits within fp32 rounding of the two exponentials
    # (per side: the exponential's ulp moves s by at most 2^-25, the add and the divide round once each)
    assert err(fw[:, ::ratio][:, :T5], C14.sigmoid32(lg[:, :, 25:50])) <= 6 * 2.0 ** -24


# ---------------------------------------------------------------------------
# 4. bit-identity
# ---------------------------------------------------------------------------
def test_batch_run_graph_workspace_identity():
    from sedx import _lib, inference
    m = build()
    x = feats(3, 32 * 9 + 17)
    three = run_features(m, x)
    again = run_features(m, x)
    one = run_features(m, x[1:2].contiguous())
    for key in KEYS:
        assert np.array_equal(three[key], again[key]), key                 # a second run
        assert np.array_equal(three[key][1:2], one[key]), key              # clip 1 of 3, alone
    # a caller workspace of exactly sedx_workspace_size bytes between guard words
    L = _lib.lib()
    nat = m.native(x.device)
    need = ctypes.c_size_t()
    _lib.check(L.sedx_workspace_size(nat.h, 3, (x.shape[2] - 1) * HOP, ctypes.byref(need)), nat.h, 'workspace_size')
    guard = 4096
    buf = torch.full((need.value + 2 * guard,), 0xA5, dtype=torch.uint8, device='cuda')
    own = run_features(m, x, ws=buf[guard:], ws_bytes=need.value)
    for key in KEYS:
        assert np.array_equal(own[key], three[key]), key
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need.value:] == 0xA5).all())
    st, _, nat = _forward(m, x, x.shape[2], False, ws=buf[guard:], ws_bytes=need.value - 1)
    assert st == EINVAL and b'workspace too small' in L.sedx_last_error(nat.h)
    # the HIP-graph path
    w = torch.from_numpy(waves('short')).cuda()
    with torch.no_grad():
        eager = {k: v.clone() for k, v in m(w).items()}
    out = inference.GraphedForward(m, w)(w)
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(out[key], eager[key]), key


# ---------------------------------------------------------------------------
# 5. precision: the encoder and the head are fp32 in every mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['exact', 'x3'])
def test_encoder_and_head_are_fp32_in_every_mode(prec):
    """On the pattern of test_gpu_conformer.test_encoder_is_fp32_under_x3: each
    mode's steps 43 -> 20 -> ... -> 32 and its head on that mode's own captures
    against the fp32 yardstick of check 2, which a split-bf16 GEMM does not meet."""
    ck = TL.Checks('conformer14-' + prec, (prec, None))
    check_steps(ck, prec, 3, 9)
    ck.done()


def test_one_sequence_input_gives_the_same_bits_in_every_mode():
    """Given one and the same id-43 tensor, captures 20 .. 32, 9, the logits (44)
    and the three outputs are bit-identical under winograd, exact and x3.  The
    modes differ in blocks 1-3 and block 4's conv1 only, so a model whose
    conv_block4.conv1.weight is zero has the same block 4 conv1 output in every
    mode (relu of the folded BatchNorm bias, whatever arithmetic multiplied the
    zeros); block 4's conv2 and blocks 5-6 are fp32 in every mode, hence capture
    43 is bit-equal across the modes -- asserted first -- and still varies along
    the sequence (the zero padding of the deep convs reaches every frame of a
    short clip differently)."""
    from sedx import models
    m = getattr(models, MT)(*C14.P16, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(MT, seed=C14.SEED).items():
        sd[k] = torch.from_numpy(v)
    sd['conv_block4.conv1.weight'] = torch.zeros_like(sd['conv_block4.conv1.weight'])
    m.load_state_dict(sd, strict=True)
    m = m.to('cuda').eval()
    B, T5 = 3, 9
    x = feats(B, 32 * T5 + 7)
    ids = (43,) + C14.ACT_IDS + (9, C14.LOGITS)
    got = {}
    for prec in PRECISIONS:
        m.set_precision(prec)
        caps = {i: capture_features(m, i, x).numpy() for i in ids}
        caps.update(run_features(m, x))
        got[prec] = caps
    ref = got['winograd']
    for prec in ('exact', 'x3'):
        assert np.array_equal(ref[43], got[prec][43]), 'capture 43 differs under ' + prec
    s43 = ref[43]
    assert float(np.abs(s43).max()) > 0 and not np.array_equal(s43[:, 0], s43[:, T5 // 2])
    for prec in ('exact', 'x3'):
        for i in ids[1:] + KEYS:
            assert np.array_equal(ref[i], got[prec][i]), (prec, i)
    # and the modes do differ on this input ahead of the zeroed layer (the comparison above is not of one kernel)
    m.set_precision('winograd')
    a = capture(m, 6, lambda: run_features(m, x), (B, x.shape[2] // 8, 8, 256)).numpy()
    m.set_precision('x3')
    b = capture(m, 6, lambda: run_features(m, x), (B, x.shape[2] // 8, 8, 256)).numpy()
    assert not np.array_equal(a, b)


# ---------------------------------------------------------------------------
# 6. windowed driver and events
# ---------------------------------------------------------------------------
def test_windowed_driver_and_events(golden_dir):
    """predict.py driver, 5 s windows at a 1 s stride: 15 x 66 = 990 frames padded
    to 1000 per window, six windows merged into 1500 frames."""
    from sedx import inference
    g = np.load(os.path.join(golden_dir, 'conformer14_windowed.npz'))['merged_5_1']
    ev = json.load(open(os.path.join(golden_dir, 'conformer14_events.json')))
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    m = build()
    audio = torch.from_numpy(synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=ev['wave_seed'])[:1]).cuda()
    merged = inference.predict_windows(m, audio, 5, 1, overlap=True).cpu().numpy()
    assert merged.shape == g.shape == (1, 1500, 25)
    e = err(merged, g)
    print('windowed 5/1 max|d| =', e)
    assert e <= TOL
    for which in ('default', 'synthetic'):
        assert inference.events_from_framewise(merged, tables['params_' + which]) == ev[which], which


# ---------------------------------------------------------------------------
# 7. refusals on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('T', [31, 32032])
def test_refused_shapes_leave_the_outputs_untouched(T):
    from sedx import _lib
    m = build()
    x = torch.zeros((1, 64, T), dtype=torch.float32, device='cuda')
    st, out, nat = _forward(m, x, T, False)
    torch.cuda.synchronize()
    assert st == EINVAL
    assert (b'5 pooling' if T == 31 else b'1000') in _lib.lib().sedx_last_error(nat.h)
    for k in KEYS:
        assert bool(torch.isnan(out[k]).all()), k
    run_features(m, feats(1, 32))                # and the handle still works


def test_mask_training_mode_and_cpu_tensors_raise():
    m = build()
    w = torch.from_numpy(waves('ragged')).cuda()
    with pytest.raises(ValueError):
        m(w, mask=torch.ones(1, 1, 1, device='cuda'))
    with pytest.raises(RuntimeError):
        m(w.cpu())
    m.train()
    try:
        with pytest.raises(RuntimeError):
            m(w)
    finally:
        m.eval()
    with torch.no_grad():
        assert tuple(m(w)['framewise_output'].shape) == (1, 1000, 25)
