"""The fp16 conv stack (SEDX_PRECISION_F16, csrc/conv_f16.hip) on the GPU.

The reference of a conv step is E of tests/f16_refs.py: the oracle's float64
step on q(input) and q(fp32(folded weight)), taken on the GPU's own previous
stage, so what is left between the kernel's G and E is the kernel's fp32
accumulation (and the rare operand whose rounding flips because block 1's
conv1 is fp32 on the GPU and float64-then-fp32 in E).  Bound: max|G - E| <=
2^-15 S16 element-wise, S16 the same step on the absolute values; 2^-15 is
X3_REL of tests/test_gpu_layers.py, the allowance the project gives a
reduced-precision MFMA step.  The sequence layer and the head run as in
'exact' and keep that file's yardstick, c = 4.

End to end the GPU may be no further from the chained emulation E_out than the
emulation is from the un-rounded float64 chain: max|G - E_out| <= d_q per
output key, both sides from the reference alone."""
import json
import os

import numpy as np
import pytest
import torch

import f16_refs as H
import test_gpu_layers as TL
from oracle import layer_refs as R
from sedx import synth

pytestmark = pytest.mark.gpu

GRU, TRF = R.GRU, R.TRF
F16 = ('f16', None)
EXACT = ('exact', None)
F16_REL = TL.X3_REL
KEYS = H.KEYS
# (1, 8): the smallest T; (3, 37): odd T, floor pooling, a ragged last t-tile; (2, 135): several t-tiles per clip
# with a ragged end; (8, 64), (16, 136): more tiles than resident workgroups on some layers (tile claims, stealing)
CHAIN_SHAPES = [(1, 8), (3, 37), (2, 135), (8, 64), (16, 136)]


def _model(mt):
    return TL.model(mt, F16)


def _sd64(mt):
    return TL.sd(mt, 25, torch.float64)


def check_conv_chain(m, mt, x, tag):
    """Every conv step of the f16 stack on the GPU's own previous stage; returns the captures."""
    caps = {st: TL.capture(m, mt, st, x) for st in R.STAGES}
    s64, bad = _sd64(mt), []
    with torch.no_grad():
        for prev, nxt, E, S16, _, _ in H.steps():
            xin, G = caps[prev], caps[nxt].double()
            e, s = E(s64, xin), S16(s64, xin)
            assert G.shape == e.shape == s.shape, (nxt, G.shape, e.shape)
            d = (G - e).abs()
            ratio = float((d / (F16_REL * s)).max())
            print('RATIO|f16|%sconv-%d|%.4f| max|G-E|=%.3g max|E|=%.3g shape=%s'
                  % (tag, nxt, ratio, float(d.max()), float(e.abs().max()), tuple(G.shape)))
            if not (d <= F16_REL * s).all():
                bad.append('stage %d: %.3f of 2^-15 S16' % (nxt, ratio))
    assert not bad, bad
    return caps


# ---------------------------------------------------------------------------
# 1. the stage chain, every layer isolated
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', CHAIN_SHAPES, ids=['B%d-T%d' % s for s in CHAIN_SHAPES])
def test_stage_chain(B, T):
    m = _model(GRU)
    x = torch.from_numpy(TL.feats(B, T)).cuda()
    caps = check_conv_chain(m, GRU, x, 'B%d-T%d-' % (B, T))
    outs = TL.run(m, GRU, x)
    ck = TL.Checks('f16-seq-head', EXACT)      # the exact mode's yardstick, c = 4
    TL.check_seq_and_head(ck, GRU, 25, EXACT, caps[8], caps[9], outs, tag='B%d-T%d-' % (B, T))
    ck.done()


# ---------------------------------------------------------------------------
# 2. end to end
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', [(3, 37), (2, 135)])
@pytest.mark.parametrize('mt', [GRU, TRF], ids=['gru', 'trf'])
def test_end_to_end(mt, B, T):
    e, _, dq = H.outputs(mt, TL.SEEDS[mt], B, T)
    G = TL.run(_model(mt), mt, torch.from_numpy(R.features(B, T, 0)).cuda())
    bad = []
    for k in KEYS:
        d = float(np.abs(G[k].astype(np.float64) - e[k]).max())
        print('E2E|f16|%s|B%d-T%d|%s| max|G-E_out|=%.3g d_q=%.3g ratio=%.4f'
              % (TL.MT_IDS[mt], B, T, k, d, dq[k], d / dq[k]))
        if not d <= dq[k]:
            bad.append((k, d, dq[k]))
    assert not bad, bad


# ---------------------------------------------------------------------------
# 3. bit identity
# ---------------------------------------------------------------------------
def test_a_clip_alone_equals_the_clip_in_a_batch():
    m = _model(GRU)
    x = torch.from_numpy(TL.feats(3, 37)).cuda()
    big = TL.run(m, GRU, x)
    for i in range(3):
        one = TL.run(m, GRU, x[i:i + 1].contiguous())
        for k in KEYS:
            assert np.array_equal(one[k][0], big[k][i]), (i, k)


def test_two_runs_and_a_second_stream_are_bit_identical():
    m = _model(GRU)
    x = torch.from_numpy(TL.feats(16, 136)).cuda()
    first = TL.run(m, GRU, x)
    again = TL.run(m, GRU, x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = TL.run(m, GRU, x)
    for k in KEYS:
        assert np.array_equal(first[k], again[k]), k
        assert np.array_equal(first[k], other[k]), k


# ---------------------------------------------------------------------------
# 4. the other trunks
# ---------------------------------------------------------------------------
def test_the_14_layer_trunk():
    """Cnn_14layers_Gru_FrameAtt at (2, 64): 'f16' moves the outputs, and by no
    more than 4 d_q.  A sanity bound, not a derived one: d_q is the 9-layer GRU
    model's distance between the emulation and the float64 chain at (2, 135),
    used as the scale of what operand rounding does to an output; the factor 4
    allows for the other model.  The launches after the last f16 layer
    (conv_deep.hip, the sequence layer, the head) are checked as in 'exact':
    every one against its float64 step on the GPU's own previous stage, with
    the documented summation order bit for bit (test_gpu_deep14.check_layers)."""
    import deep14_refs as D
    import test_gpu_deep14 as T14
    x = T14.feats(2, 64)
    of = T14.run_features(T14.build(D.GRU14, 'f16'), x)
    oe = T14.run_features(T14.build(D.GRU14, 'exact'), x)
    # block 4's conv1 (stage 7) is the last f16 layer: its capture moves with the mode
    s7f = T14.capture_features(T14.build(D.GRU14, 'f16'), 7, x)
    s7e = T14.capture_features(T14.build(D.GRU14, 'exact'), 7, x)
    print('DEEP14|f16 vs exact|stage 7| max|d|=%.3g at max|x|=%.3g' % (float((s7f - s7e).abs().max()), float(s7e.abs().max())))
    assert not torch.equal(s7f, s7e)
    dq = H.outputs(GRU, 0, 2, 135)[2]
    for k in KEYS:
        d = float(np.abs(of[k].astype(np.float64) - oe[k]).max())
        print('DEEP14|f16 vs exact|%s| max|d|=%.3g 4 d_q=%.3g' % (k, d, 4 * dq[k]))
        assert 0 < d <= 4 * dq[k], (k, d, dq[k])
    ck = TL.Checks('f16-deep14', EXACT)
    T14.check_layers(ck, 'f16', 2, 64)
    ck.done()


def test_a_vggish_model_is_bit_identical_to_exact():
    import test_gpu_vggish as TV
    import vggish_refs as V
    mt = V.MODELS[0]
    x = torch.from_numpy(TL.feats(2, 64)).cuda()
    oe = TV.run_features(TV.build(mt, 'exact'), mt, x)
    of = TV.run_features(TV.build(mt, 'f16'), mt, x)
    TV.build(mt, 'winograd')
    for k in KEYS:
        assert np.array_equal(oe[k], of[k]), k


# ---------------------------------------------------------------------------
# 5. a driver
# ---------------------------------------------------------------------------
def test_windowed_driver_equals_the_host_merge_of_its_windows(golden_dir):
    from sedx import inference
    m = _model(TRF)                              # takes waveforms (log-mel front end)
    audio = synth.make_waveforms(1, seconds=7.0, sample_rate=16000, seed=77)
    assert audio.shape == (1, 112000)
    merged = inference.predict_windows(m, torch.from_numpy(audio).cuda(), 5, 1.0, overlap=True).cpu().numpy()
    starts, lens = inference.window_starts(16000, audio.shape[1], 5, 1.0, 'predict', True)
    assert len(starts) > 1
    wins = []
    with torch.no_grad():
        for st, ln in zip(starts, lens):
            w = np.zeros((1, 5 * 16000), np.float32)           # pad_truncate to the window
            w[0, :ln] = audio[0, st:st + ln]
            wins.append(m(torch.from_numpy(w).cuda())['framewise_output'][0].cpu().numpy())
    m.check_error()
    want = inference.merge_host(wins, 5, 1.0)
    assert merged.shape == want.shape and np.isfinite(merged).all()
    assert np.array_equal(merged, want)
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    ev = inference.events_from_framewise(merged, tables['params_default'])
    assert isinstance(ev, list)


# ---------------------------------------------------------------------------
# 6. out-of-range input
# ---------------------------------------------------------------------------
def test_out_of_range_input_is_clamped():
    """Features scaled by 1e5: stage 0 passes 65504, so block 1's conv1 output
    and the activations after it meet the clamp of q.  Every conv step stays
    within the chain bound of its emulation, the outputs are finite and within
    d_q of the emulation's (an unclamped fp16 conversion gives inf, and inf - inf
    in the next layer NaN)."""
    B, T = 2, 37
    feat = (R.features(B, T, 5) * np.float32(1e5)).astype(np.float32)
    m = _model(GRU)
    x = torch.from_numpy(feat).cuda()
    caps = check_conv_chain(m, GRU, x, 'big-')
    assert float(caps[0].abs().max()) > 65504 and float(caps[2].max()) > 65504
    e, _, dq = H.outputs(GRU, 0, B, T, feat=feat, tag='big')
    G = TL.run(m, GRU, x)                         # asserts finite outputs
    for k in KEYS:
        d = float(np.abs(G[k].astype(np.float64) - e[k]).max())
        print('BIG|f16|%s| max|G-E_out|=%.3g d_q=%.3g' % (k, d, dq[k]))
        assert np.isfinite(e[k]).all() and d <= dq[k], (k, d, dq[k])
