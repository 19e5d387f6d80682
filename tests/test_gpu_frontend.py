"""The log-mel front end (csrc/frontend.hip) alone against a float64 reference.

Every test feeds a waveform to ``Cnn_9layers_FrameAvg`` (the cheapest model
behind the front end, synthetic weights; window mode needs a model with 100
framewise frames per second) and reads stage 0 (X0 = bn0 of the
log-mel spectrogram, [items, T, 64]) through ``sedx_set_capture``.  The
reference R is ``oracle.sed_oracle.logmel`` + ``bn0`` in float64 on the model's
own fp32 front-end tensors (tests/frontend_refs.py).

Yardstick (``test_gpu_layers.Checks``, c = 4, never derived from the kernel's
output): max|G - R| <= 4 max(e_cpu, e_fft, floor), e_cpu the fp32 oracle's own
distance from R (a DFT as two convolutions), e_fft that of an fp32 rfft
restatement of the kernel's algorithm class (passed as ``e_alg``), floor =
2^-23 max|R|.  Every check prints ``RATIO`` before it asserts.

What runs where: logmel_kernel<256 / 1024, float / int16> (8 k / 32 k),
logmel512_kernel<float / int16, band sums / MFMA> (16 k, SEDX_TUNE_MEL_MFMA
0 / 1), and through caller-supplied filter banks the three mel loops of each
(band table, per-band LDS loop, per-band global loop), the MFMA path's bin
clamp and its fall-back when the table is too large, DC and Nyquist weights.
"""
import ctypes

import numpy as np
import pytest
import torch

import frontend_refs as FR
import test_gpu_layers as TL
from oracle import sed_oracle as O

pytestmark = pytest.mark.gpu

GRU = 'Cnn_9layers_Gru_FrameAtt'
FORM = ('exact', None)          # the conv arithmetic behind the front end (not under test)
C = 4                           # the project's constant for non-conv steps
SHAPES = [(8, 0), (8, 1), (9, -1), (10, 1), (11, 0), (19, 3), (33, -1)]      # (T, r); r = -1: hop - 1
_MODELS = {}


# ---------------------------------------------------------------------------
# models, captures, references
# ---------------------------------------------------------------------------
def build(preset, fmin=None, fmax=None, mt=FR.FAVG):
    from sedx import models, synth
    args = FR.preset_args(preset, fmin, fmax) + ((25,) if mt == FR.FAVG else (25, 'logmel'))
    m = getattr(models, mt)(*args)
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, seed=FR.SEED).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval().set_precision(FORM[0])


def model(preset):
    if preset not in _MODELS:
        _MODELS[preset] = build(preset)
    return _MODELS[preset]


def ref_state(m, preset):
    """The reference's state dict from the tensors the model itself holds."""
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if k in (FR.WR, FR.WI, FR.MELW) + FR.BN0}
    sd['_hop'] = O.PRESETS[preset]['hop_size']
    return sd


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def capture_x0(m, items, T, call):
    """X0 [items, T, 64] of the forward that ``call()`` runs."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(torch.device('cuda', 0))
    buf = torch.full((items, T, 64), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(L.sedx_set_capture(nat.h, 0, _p(buf), buf.numel() * 4), nat.h, 'set_capture')
    try:
        with torch.no_grad():
            call()
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'set_capture')
    m.check_error()
    a = buf.cpu()
    assert torch.isfinite(a).all(), 'X0 was not written everywhere'
    return a


def x0(m, preset, wave, mfma=None):
    from sedx import _lib
    if mfma is not None:
        m.set_tuning(_lib.TUNE_MEL_MFMA, mfma)
    wave = np.ascontiguousarray(wave)
    T = wave.shape[1] // O.PRESETS[preset]['hop_size'] + 1
    w = torch.from_numpy(wave).cuda()
    return capture_x0(m, wave.shape[0], T, lambda: m(w))


def mfma_modes(preset):
    return (0, 1) if preset == '16k' else (None,)


def check(ck, step, G, sd, wave):
    wave = FR.as_float(wave)
    R = FR.ref_x0(sd, wave, torch.float64)
    e_fft = float((FR.fft_x0(sd, wave).double() - R).abs().max())
    ck.check(step, G, R, FR.ref_x0(sd, wave, torch.float32), c=C, e_alg=e_fft)
    return R


def quantise(x):
    return (np.clip(x, -1.0, 1.0) * 32767).astype(np.int16)


def wave_of(cls, preset, B, L, i16, seed):
    if i16:
        return FR.inputs('int16', preset, B, L, seed) if cls == 'noise' else quantise(FR.inputs(cls, preset, B, L, seed))
    return FR.inputs(cls, preset, B, L, seed)


def hop_of(preset):
    return O.PRESETS[preset]['hop_size']


# ---------------------------------------------------------------------------
# a. float64 parity over the instantiations and edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('i16', [False, True], ids=['f32', 'i16'])
@pytest.mark.parametrize('preset', FR.PRESETS)
def test_parity(preset, i16, B):
    """Every (T, r) of SHAPES (L = hop (T - 1) + r: both reflections in most
    frames, odd L, L % hop = hop - 1, flat frame counts 8 .. 99 with clip
    boundaries inside the 4- and 16-frame groups) x noise / synth, plus tone /
    silence at (3, 19); 16 kHz with the band-sum and the MFMA mel path."""
    m = model(preset)
    sd = ref_state(m, preset)
    ck = TL.Checks('fe-parity-%s-%s' % (preset, 'i16' if i16 else 'f32'), FORM)
    for T, r in SHAPES:
        L = FR.clip_len(preset, T, hop_of(preset) - 1 if r < 0 else r)
        classes = ['noise', 'synth'] + (['tone', 'silence'] if (B, T) == (3, 19) else [])
        for cls in classes:
            wave = wave_of(cls, preset, B, L, i16, seed=T)
            for mf in mfma_modes(preset):
                G = x0(m, preset, wave, mf)
                assert G.shape == (B, T, 64)
                check(ck, '%s-B%d-T%d-L%d-mfma%s' % (cls, B, T, L, mf), G, sd, wave)
    ck.done()


# ---------------------------------------------------------------------------
# b. filter-bank regimes
# ---------------------------------------------------------------------------
BANKS = [('16k', 'full'), ('16k', 'sparse'), ('16k', 'wide'), ('16k', 'dense'), ('16k', 'dense_mt'),
         ('8k', 'full'), ('8k', 'dense'), ('32k', 'full'), ('32k', 'dense')]


@pytest.mark.parametrize('preset,kind', BANKS, ids=['%s-%s' % b for b in BANKS])
def test_filter_banks(preset, kind):
    """Caller-supplied banks reach the mel loops no preset reaches (asserted
    on the bank's geometry), and each meets the yardstick; at 16 kHz the MFMA
    mel path gives the band sums' bits on every bank (its bin clamp on
    ``full`` / ``dense``; ``dense_mt``'s table is too large and falls back)."""
    p = O.PRESETS[preset]
    n_fft = p['window_size']
    base = model(preset)
    if kind == 'full':
        m = build(preset, 0, p['sample_rate'] // 2)
    elif kind == 'sparse':
        m = build(preset, 0, p['sample_rate'] // 16)
    else:
        # through load_state_dict on a model that already ran: the handle must repack
        m = build(preset)
        wave = FR.inputs('noise', preset, 1, FR.clip_len(preset, 8, 0), seed=1)
        before = x0(m, preset, wave)
        assert torch.equal(before, x0(base, preset, wave))
        sig = m.native(torch.device('cuda', 0)).signature
        sdm = m.state_dict()
        sdm[FR.MELW] = torch.from_numpy(FR.bank(kind, preset))
        m.load_state_dict(sdm, strict=True)
        after = x0(m, preset, wave)
        assert m.native(torch.device('cuda', 0)).signature != sig, 'the native handle did not reload'
        assert not torch.equal(before, after), 'X0 did not change with the filter bank'
    sd = ref_state(m, preset)
    melW = sd[FR.MELW].numpy()
    g = FR.regime(melW)
    cap = FR.mel_lds_cap(n_fft)
    print('BANK|%s|%s| nnz=%d cap=%d wmax=%d mt_floats=%s clamp=%s' % (preset, kind, g['nnz'], cap, g['wmax'],
                                                                     g.get('mt_floats'), g.get('mt_clamp')))
    if kind == 'full':
        assert g['nnz'] <= cap and (n_fft != 512 or (g['wmax'] <= FR.FE16_MEL_MW and g['mt_clamp']))
    elif kind == 'sparse':
        assert (g['width'] == 0).sum() >= 2 and (g['width'] == 1).sum() >= 2
    elif kind == 'wide':
        assert g['wmax'] > FR.FE16_MEL_MW and g['nnz'] <= cap
    else:
        assert g['nnz'] > cap and melW[0, 0] > 0 and melW[-1, 63] > 0
        if kind == 'dense_mt':
            assert g['mt_floats'] > FR.FE_MT_MAX_FLOATS
        elif n_fft == 512:
            assert g['mt_floats'] <= FR.FE_MT_MAX_FLOATS and g['mt_clamp']
    ck = TL.Checks('fe-bank-%s-%s' % (preset, kind), FORM)
    for B, T in [(3, 19), (1, 8)]:
        L = FR.clip_len(preset, T, 1)
        for cls in ('noise', 'synth'):
            wave = FR.inputs(cls, preset, B, L, seed=5 + T)
            got = {}
            for mf in mfma_modes(preset):
                got[mf] = x0(m, preset, wave, mf)
                R = check(ck, '%s-B%d-T%d-mfma%s' % (cls, B, T, mf), got[mf], sd, wave)
            if preset == '16k':
                assert torch.equal(got[1], got[0]), 'MEL_MFMA 1 differs from the band sums'
            if kind == 'sparse':
                # bands without a bin: bn0(10 log10(1e-10)), as the float64 reference gives it
                empty = np.flatnonzero(g['width'] == 0)
                for mf, G in got.items():
                    d = (G[..., empty].double() - R[..., empty]).abs().max()
                    assert (G[..., empty] == G[0, 0, empty]).all()
                    assert float(d) <= C * 2.0 ** -23 * float(R[..., empty].abs().max()), float(d)
    ck.done()


# ---------------------------------------------------------------------------
# c. position and alignment invariance, d. int16 = dequantised float (exact)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('i16', [False, True], ids=['f32', 'i16'])
@pytest.mark.parametrize('preset', FR.PRESETS)
def test_clip_position_and_alignment_invariance(preset, i16):
    """Odd L: clip 1 of a batch starts at an odd sample offset, so its interior
    frames take the element-wise loads, clip 0's the 8-byte ones.  The same
    clip at indices 0 and 1 (and alone) gives the same bits."""
    m = model(preset)
    L = FR.clip_len(preset, 19, 1)
    assert L % 2 == 1
    wave = wave_of('synth', preset, 4, L, i16, seed=11)
    wave[1] = wave[0]
    for mf in mfma_modes(preset):
        G = x0(m, preset, wave, mf)
        alone = x0(m, preset, wave[:1], mf)
        assert torch.equal(G[0], G[1]), 'mfma %s: clip at index 1 differs from index 0' % mf
        assert torch.equal(G[0], alone[0]), 'mfma %s: clip in a batch differs from the clip alone' % mf
        assert not torch.equal(G[2], G[0])


@pytest.mark.parametrize('preset', FR.PRESETS)
def test_int16_equals_dequantised_float(preset):
    m = model(preset)
    q = FR.inputs('int16', preset, 3, FR.clip_len(preset, 19, 3), seed=2)
    deq = O.int16_to_float32(q)
    assert deq.dtype == np.float32
    for mf in mfma_modes(preset):
        assert torch.equal(x0(m, preset, q, mf), x0(m, preset, deq, mf)), 'mfma %s' % mf


# ---------------------------------------------------------------------------
# e. several passes of the frame loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('preset', FR.PRESETS)
def test_frame_loop_passes(preset):
    """More frames than twice what the launch's resident workgroups hold, so
    every wave walks its loop (and prefetches the next group's samples) at
    least twice: bit-identical to the same clips in batches of one pass, and
    every 97th frame meets the yardstick."""
    from sedx import synth
    p = O.PRESETS[preset]
    sr, hop = p['sample_rate'], p['hop_size']
    # launch_logmel_t / launch_logmel512: min(frames / 16, CUs * per_cu) workgroups of 16 frames
    per_cu = 1 if p['window_size'] == 1024 else 2
    cap = torch.cuda.get_device_properties(0).multi_processor_count * per_cu * 16
    L = 10 * sr
    T = L // hop + 1
    B = 2 * cap // T + 1
    if (B * T) % 16 == 0:
        B += 1
    small = cap // T
    assert B * T > 2 * cap and (B * T) % 16 != 0 and 1 <= small and small * T <= cap
    m = model(preset)
    sd = ref_state(m, preset)
    wave = synth.make_waveforms(B, seconds=10.0, sample_rate=sr, seed=41)
    flat = np.arange(0, B * T, 97)
    R = FR.ref_x0_frames(sd, wave, flat, torch.float64)
    f32 = FR.ref_x0_frames(sd, wave, flat, torch.float32)
    e_fft = float((FR.fft_x0_frames(sd, wave, flat).double() - R).abs().max())
    ck = TL.Checks('fe-passes-%s' % preset, FORM)
    for mf in mfma_modes(preset):
        G = x0(m, preset, wave, mf)
        parts = [x0(m, preset, wave[i:i + small], mf) for i in range(0, B, small)]
        assert torch.equal(G, torch.cat(parts)), 'mfma %s: B = %d differs from batches of %d' % (mf, B, small)
        ck.check('B%d-T%d-cap%d-mfma%s' % (B, T, cap, mf), G.reshape(-1, 64)[flat], R, f32, c=C, e_alg=e_fft)
    ck.done()


# ---------------------------------------------------------------------------
# f. window mode
# ---------------------------------------------------------------------------
def test_window_mode():
    """8 kHz, 3.5 s clips in 1 s windows up to audio_duration 4.0: the last
    window holds 0.5 s of audio and 0.5 s of pad_truncate zeros.  The model is
    Cnn_9layers_Gru_FrameAtt: its 100 framewise frames per 1 s window merge at
    the driver's 100-frame step, while FrameAvg's 96 make the reference's
    merge raise (sedx_window_geometry refuses it, whatever audio_duration)."""
    from sedx import inference
    preset, sr = '8k', 8000
    m = build(preset, mt=GRU)
    sd = ref_state(m, preset)
    L = 28001                                           # 3.5 s (+ 1: odd clip stride)
    kw = dict(sample_duration=1, overlap_value=1.0, overlap=True, driver='predict', audio_duration=4.0)
    starts, lens = inference.window_starts(sr, L, **kw)
    assert starts == [0, 8000, 16000, 24000] and lens == [sr] * 4 and starts[-1] + sr > L
    nw, wlen, _ = inference.window_geometry(m, L, **kw)
    assert (nw, wlen) == (4, sr)
    T = sr // 80 + 1
    wave = FR.inputs('synth', preset, 2, L, seed=23)
    ck = TL.Checks('fe-windows', FORM)
    got = {}
    for name, w in (('clip1', wave[1:2]), ('both', wave)):
        wd = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        G = capture_x0(m, w.shape[0] * nw, T, lambda: inference.predict_windows(m, wd, **kw))
        check(ck, name, G, sd, FR.window_slices(w, starts, sr))
        got[name] = G
    # the zero tail reaches the output: the last window's late frames sit on the clamp
    tail = FR.ref_logmel(sd, FR.window_slices(wave[1:2], starts, sr), torch.float64)[-1, -10:]
    assert (tail == -100.0).all()
    assert torch.equal(got['both'][nw:], got['clip1']), 'clip 1 of two differs from the clip alone'
    ck.done()
