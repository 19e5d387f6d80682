"""HIP path of the two 14-layer models (Cnn_14layers_Gru_FrameAtt,
Cnn_14layers_Transformer_FrameAtt): goldens the reference produced
(tools/make_golden_deep14.py), every new launch in isolation against its
float64 restatement (tests/deep14_refs.py) with the yardstick of
tests/test_gpu_layers.py, the deep conv kernel's documented summation order bit
for bit, batch / run / graph / workspace bit-identity, fp32 under the
split-bf16 mode, and the rejections.

Layer yardstick (tests/test_gpu_layers.py unchanged): max|G - R| <=
4 max(e_cpu, floor).  The deep convs sum up to 18,432 terms as ONE in-order
fp32 chain (csrc/conv_deep.hip header), the recorded exception of that file's
stages 5 and 7: their yardstick is max(e_cpu, e_alg, floor), e_alg the error of
the CPU fp32 emulation of that order (deep14_refs.emulate_step) on the same
input, and the kernel's values equal the emulation bit for bit at the sampled
pixels.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import deep14_refs as D
import test_gpu_layers as TL
from sedx import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the project's bar against the reference (tests/test_gpu_parity.py)
KEYS = D.KEYS
MODELS = (D.GRU14, D.TRF14)
IDS = {D.GRU14: 'gru14', D.TRF14: 'trf14'}
MODEL_IDS = [IDS[m] for m in MODELS]
P16 = (16000, 512, 160, 64, 25, 7000)
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


def build(mt, prec='winograd'):
    from sedx import models
    if (mt, prec) not in _MODELS:
        m = getattr(models, mt)(*P16, 25, 'logmel')
        sd = m.state_dict()
        for k, v in synth.make_state_dict(mt, seed=D.SEEDS[mt]).items():
            sd[k] = torch.from_numpy(v)
        m.load_state_dict(sd, strict=True)
        _MODELS[(mt, prec)] = m.to('cuda').eval().set_precision(prec)
    return _MODELS[(mt, prec)]


def states(mt):
    if mt not in _SD:
        _SD[mt] = (D.state(mt, torch.float64), D.state(mt, torch.float32))
    return _SD[mt]


def run(m, wave):
    with torch.no_grad():
        out = m(torch.as_tensor(np.asarray(wave), dtype=torch.float32).cuda())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k
    return out


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def forward_features(m, x, ws=None, ws_bytes=0):
    """One forward of features x [B, 64, T] (cuda) through sedx_forward_features."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B, _, T = x.shape
    T5, frames = D.geometry(T)
    fw = torch.full((B, frames, 25), float('nan'), dtype=torch.float32, device=x.device)
    clip = torch.full((B, 25), float('nan'), dtype=torch.float32, device=x.device)
    emb = torch.full((B, 25 if m._embedding_cla else 2048, T5), float('nan'), dtype=torch.float32, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(L.sedx_forward_features(nat.h, _p(x), B, T, _p(fw), _p(clip), _p(emb),
                                       _p(ws) if ws is not None else None, ws_bytes, stream),
               nat.h, 'forward_features')
    return {'framewise_output': fw, 'clipwise_output': clip, 'embedding': emb}


def run_features(m, x, **kw):
    out = forward_features(m, x, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k      # every element was written
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
    B, _, T = x.shape
    return D.from_capture(stage, capture(m, stage, lambda: forward_features(m, x), D.capture_shape(stage, B, T)))


def feats(B, T):
    return torch.from_numpy(TL.feats(B, T)).cuda()


def _waves(kind):
    if kind == 'short':
        return synth.make_waveforms(2, seconds=10400 / 16000., sample_rate=16000, seed=11)
    if kind == 'ragged':
        return synth.make_waveforms(1, seconds=7777 / 16000., sample_rate=16000, seed=12)
    return synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)[:1]


# ---------------------------------------------------------------------------
# 1. goldens
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['short', 'ragged', 'clip10s'])
@pytest.mark.parametrize('prec', ['winograd', 'exact', 'x3'])
@pytest.mark.parametrize('mt', MODELS, ids=MODEL_IDS)
def test_goldens(mt, prec, kind, golden_dir):
    g = np.load(os.path.join(golden_dir, 'deep14_%s.npz' % mt))
    m = build(mt, prec)
    out = run(m, _waves(kind))
    for k in KEYS:
        ref = g['%s_%s' % (kind, k)]
        scale = max(1.0, float(np.abs(ref).max())) if k == 'embedding' else 1.0
        e = err(out[k], ref)
        print(mt, prec, kind, k, 'max|d| = %.3g (scale %.3g)' % (e, scale))
        assert e <= TOL * scale
    if kind == 'short':
        # both captured stages within 1e-4 x the stage's scale (test_stage_goldens' rule)
        w = torch.from_numpy(_waves(kind)).cuda()
        with torch.no_grad():
            for stage, key in ((43, 'short_seq_in'), (9, 'short_seq_out')):
                a = capture(m, stage, lambda: m(w), (2, 2, 2048)).numpy()
                scale = max(1.0, float(np.abs(g[key]).max()))
                e = err(a, g[key])
                print(mt, prec, 'stage', stage, 'max|d| = %.3g (scale %.3g)' % (e, scale))
                assert e <= 1e-4 * scale


@pytest.mark.parametrize('prec', ['winograd', 'exact', 'x3'])
def test_windowed_driver_and_events(prec, golden_dir):
    """predict.py driver, 5 s windows at 1 s stride on Cnn_14layers_Gru_FrameAtt:
    480-frame windows padded to 500; the event lists of both tables."""
    from sedx import inference
    g = np.load(os.path.join(golden_dir, 'deep14_windowed.npz'))['merged_5_1']
    ev = json.load(open(os.path.join(golden_dir, 'deep14_events.json')))
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    m = build(D.GRU14, prec)
    audio = torch.from_numpy(synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=ev['wave_seed'])[:1]).cuda()
    merged = inference.predict_windows(m, audio, 5, 1, overlap=True).cpu().numpy()
    assert merged.shape == g.shape == (1, 1000, 25)
    e = err(merged, g)
    print('windowed 5/1', prec, 'max|d| =', e)
    assert e <= TOL
    for which in ('default', 'synthetic'):
        assert inference.events_from_framewise(merged, tables['params_' + which]) == ev[which], which


# ---------------------------------------------------------------------------
# 2. layer isolation
# ---------------------------------------------------------------------------
# T5 = 1, 1, 1, 2, 3, 6; odd rows at every pooled level (T3 = 5, 25; T4 = 3, 7;
# T2 = 11, 15); at (3, 112) the deep layers have 84 and 18 pixels
LAYER_SHAPES = [(B, T) for T in (32, 47, 63, 64, 112, 200) for B in (1, 3)]
DEEP_NEXT = (8, 40, 41, 42, 43)     # the outputs of csrc/conv_deep.hip's launches


def check_layers(ck, prec, B, T, n_pix=2):
    """Every new launch against the float64 step on the GPU's own previous stage."""
    x = feats(B, T)
    g64, g32 = states(D.GRU14)
    m = build(D.GRU14, prec)
    caps = {st: capture_features(m, st, x) for st in (7,) + DEEP_NEXT + (9,)}
    tag = 'B%d-T%d-' % (B, T)
    with torch.no_grad():
        for prev, nxt, k, fn in D.conv_steps():
            if nxt not in DEEP_NEXT:
                continue
            xin, G = caps[prev], caps[nxt]
            r64 = fn(g64, xin.double())
            pix, E = D.emulate_step(g64, nxt, k, xin, n_pix)
            sel = (lambda a: a[pix[:, 0], :, pix[:, 1]]) if nxt == 43 else (lambda a: a[pix[:, 0], :, pix[:, 1], pix[:, 2]])
            nd = int((sel(G) != E).sum())
            print('  stage %d: kernel vs emulated fp32 chain on %d pixels: %d of %d values differ'
                  % (nxt, len(pix), nd, E.numel()))
            assert nd == 0, 'stage %d: the kernel no longer sums in the order its header documents' % nxt
            e_alg = float((E.double() - sel(r64)).abs().max())
            ck.check(tag + 'conv-%d' % nxt, G, r64, fn(g32, xin), c=4, e_alg=e_alg)
        # the sequence layer and the head of both models on the GPU's own stage 43 / 9
        for mt in MODELS:
            mm = build(mt, prec)
            s64, s32 = states(mt)
            s43 = caps[43] if mt == D.GRU14 else capture_features(mm, 43, x)
            s9 = caps[9] if mt == D.GRU14 else capture_features(mm, 9, x)
            ck.check(tag + IDS[mt] + '-seq', s9, D.step_seq(s64, mt, s43.double()), D.step_seq(s32, mt, s43), c=4)
            outs = run_features(mm, x)
            rh, fh = D.step_head(s64, mt, s9.double()), D.step_head(s32, mt, s9)
            assert outs['framewise_output'].shape == (B, D.geometry(T)[1], 25) == tuple(rh['framewise_output'].shape)
            for key in KEYS:
                ck.check(tag + IDS[mt] + '-head-' + key.split('_')[0], outs[key], rh[key], fh[key], c=4)


@pytest.mark.parametrize('B,T', LAYER_SHAPES, ids=['B%d-T%d' % s for s in LAYER_SHAPES])
def test_layers_in_isolation(B, T):
    ck = TL.Checks('deep14', WINO)
    check_layers(ck, 'winograd', B, T)
    ck.done()


def test_block4_conv2_reads_every_family_layout():
    """Block 4's pooled conv2 reads block 4 conv1's NHWC output under the exact
    family and the chunk-of-4 one under F(4x4,3x3): same yardstick on both."""
    ck = TL.Checks('deep14-b4c2', ('exact', None))
    g64, g32 = states(D.GRU14)
    x = feats(3, 112)
    for prec in ('exact', 'winograd'):
        m = build(D.GRU14, prec)
        s7, s8 = capture_features(m, 7, x), capture_features(m, 8, x)
        with torch.no_grad():
            r64 = D.step_conv2(g64, 4, s7.double())
            pix, E = D.emulate_step(g64, 8, 4, s7, 2)
            sel = lambda a: a[pix[:, 0], :, pix[:, 1], pix[:, 2]]
            assert torch.equal(sel(s8), E), prec
            ck.check(prec + '-conv-8', s8, r64, D.step_conv2(g32, 4, s7), c=4,
                     e_alg=float((E.double() - sel(r64)).abs().max()))
    ck.done()


# ---------------------------------------------------------------------------
# 3. bit-identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', MODELS, ids=MODEL_IDS)
def test_batch_run_graph_workspace_identity(mt):
    from sedx import _lib, inference
    m = build(mt)
    x = feats(33, 64)
    big = run_features(m, x)
    again = run_features(m, x)
    for key in KEYS:
        assert np.array_equal(big[key], again[key]), key                     # a second run
    for i in (0, 17, 32):
        one = run_features(m, x[i:i + 1].contiguous())
        three = run_features(m, torch.stack([x[5], x[i], x[9]]).contiguous())
        for key in KEYS:
            assert np.array_equal(big[key][i:i + 1], one[key]), (i, key)     # alone
            assert np.array_equal(big[key][i], three[key][1]), (i, key)      # at B = 3 in another position
    # a caller workspace of exactly sedx_workspace_size bytes, 0xFF-filled inside a larger tensor
    L = _lib.lib()
    nat = m.native(x.device)
    xs = x[:3].contiguous()
    need = ctypes.c_size_t()
    # (a logmel handle's size query takes samples: 63 hops are the 64 frames)
    _lib.check(L.sedx_workspace_size(nat.h, 3, 63 * 160, ctypes.byref(need)), nat.h, 'workspace_size')
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
# 4. precision: everything new is fp32 in every mode
# ---------------------------------------------------------------------------
def test_new_stages_are_fp32_under_x3():
    ck = TL.Checks('deep14-x3', ('x3', None))
    check_layers(ck, 'x3', 3, 112)
    ck.done()


# ---------------------------------------------------------------------------
# 5. rejections
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', MODELS, ids=MODEL_IDS)
def test_31_frames_are_rejected_alike(mt):
    from sedx import _lib
    L = _lib.lib()
    m = build(mt)
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    with pytest.raises(RuntimeError):
        forward_features(m, feats(2, 31))
    fr, sl, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
    # logmel handles: the queries take samples; 31 frames = 30 hops
    assert L.sedx_output_geometry(nat.h, 30 * 160, ctypes.byref(fr), ctypes.byref(sl)) == EINVAL
    assert L.sedx_workspace_size(nat.h, 2, 30 * 160, ctypes.byref(nb)) == EINVAL
    assert L.sedx_output_geometry(nat.h, 31 * 160, ctypes.byref(fr), ctypes.byref(sl)) == 0
    assert (fr.value, sl.value) == (100, 1)
    with pytest.raises(RuntimeError):
        run(m, np.zeros((1, 30 * 160), np.float32))
    torch.cuda.synchronize()
    run_features(m, feats(2, 32))                # and the handle still works


def test_a_handle_refuses_the_other_models_keys():
    from sedx import models
    other = {D.GRU14: D.TRF14, D.TRF14: D.GRU14}
    for mt in MODELS:
        m = getattr(models, mt)(*P16, 25, 'logmel').to('cuda').eval()
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(other[mt], seed=0).items()}
        nat = m.native(torch.device('cuda', torch.cuda.current_device()))
        with pytest.raises(RuntimeError):
            nat.load(sd)
