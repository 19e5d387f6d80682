"""The front-end references and fixtures of tests/frontend_refs.py, on the CPU:
the references are the oracle's own arithmetic, the yardstick built from them
is sharp (far below a tenth of a dB), and every filter bank reaches the
kernel path it is named for."""
import os

import numpy as np
import pytest
import torch

import frontend_refs as FR
from oracle import sed_oracle as O

HALF_SECOND = {'8k': (3, 51, 1), '16k': (3, 51, 1), '32k': (3, 51, 1)}      # (B, T, r): L ~ 0.5 s, odd
SHARP_DB = 1e-3                 # 4 max(e_cpu, e_fft, floor) before bn0 stays under this
BANKS = [(p, 'preset') for p in FR.PRESETS] + [(p, 'full') for p in FR.PRESETS] + \
        [(p, 'dense') for p in FR.PRESETS] + [('16k', 'wide'), ('16k', 'dense_mt')]


def _wave(kind, preset):
    B, T, r = HALF_SECOND[preset]
    return FR.inputs(kind, preset, B, FR.clip_len(preset, T, r), seed=3)


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize('preset', FR.PRESETS)
def test_ref_fp32_is_the_oracle(preset):
    """ref_x0(fp32) before bn0 is O.logmel bit for bit, and ref_x0 is its bn0."""
    sd = FR.state(preset)
    wave = _wave('synth', preset)
    full = O.full_state({k: sd[k].numpy() for k in FR.BN0}, preset)
    with torch.no_grad():
        want = O.logmel(full, torch.from_numpy(wave))
        want0 = O.bn0(full, want)
    assert torch.equal(FR.ref_logmel(sd, wave, torch.float32), want[:, 0])
    assert torch.equal(FR.ref_x0(sd, wave, torch.float32), want0[:, 0])
    assert FR.ref_x0(sd, wave, torch.float64).dtype == torch.float64
    # the per-frame form is the same operation on the selected frames
    flat = np.arange(0, want.shape[0] * want.shape[2], 7)
    r = FR.ref_x0(sd, wave, torch.float64).reshape(-1, 64)[flat]
    assert _err(FR.ref_x0_frames(sd, wave, flat, torch.float64), r) <= 1e-9
    assert _err(FR.fft_x0_frames(sd, wave, flat), FR.fft_x0(sd, wave).reshape(-1, 64)[flat]) <= 1e-4


@pytest.mark.parametrize('mt,seed', [('Cnn_9layers_Gru_FrameAtt', 0), ('Cnn_9layers_Transformer_FrameAtt', 1)])
def test_ref_reproduces_stage_golden(golden_dir, mt, seed):
    g = np.load(os.path.join(golden_dir, 'stages_%s.npz' % mt))
    got = FR.ref_x0(FR.state('16k', seed=seed), g['wave'], torch.float32).numpy()
    ref = g['bn0'][:, 0]
    assert got.shape == ref.shape
    assert np.max(np.abs(got.astype(np.float64) - ref)) / max(1.0, np.max(np.abs(ref))) <= 1e-5


@pytest.mark.parametrize('preset,kind', BANKS, ids=['%s-%s' % b for b in BANKS])
@pytest.mark.parametrize('cls', ['noise', 'synth'])
def test_yardstick_is_sharp(preset, kind, cls):
    """4 max(e_cpu, e_fft, floor) <= 1e-3 dB before bn0: the yardstick of
    tests/test_gpu_frontend.py would catch a spectrum error of a thousandth of
    a dB on these classes (bn0 scales by ~1/20)."""
    sd = FR.state(preset, None if kind == 'preset' else FR.bank(kind, preset))
    wave = _wave(cls, preset)
    R = FR.ref_logmel(sd, wave, torch.float64)
    e_cpu = _err(FR.ref_logmel(sd, wave, torch.float32), R)
    e_fft = _err(FR.fft_logmel(sd, wave), R)
    floor = 2.0 ** -23 * float(R.abs().max())
    print('SHARP|%s|%s|%s| e_cpu=%.3g e_fft=%.3g floor=%.3g 4max=%.3g dB' % (preset, kind, cls, e_cpu, e_fft, floor,
                                                                            4 * max(e_cpu, e_fft, floor)))
    assert 4 * max(e_cpu, e_fft, floor) <= SHARP_DB


@pytest.mark.parametrize('preset', FR.PRESETS)
@pytest.mark.parametrize('cls', ['noise', 'synth', 'tone', 'silence', 'int16'])
def test_fft_restatement_vs_float64(preset, cls):
    """fft_x0 against R per class (printed): on ``tone`` the FFT class errs
    more than the oracle's DFT convolution, which is why e_fft is in the
    yardstick.  Asserted: both fp32 forms stay within 1e-3 of R after bn0
    wherever the band power is not cancellation noise (noise / synth / int16)."""
    sd = FR.state(preset)
    wave = FR.as_float(_wave(cls, preset))
    R = FR.ref_x0(sd, wave, torch.float64)
    e_cpu = _err(FR.ref_x0(sd, wave, torch.float32), R)
    e_fft = _err(FR.fft_x0(sd, wave), R)
    floor = 2.0 ** -23 * float(R.abs().max())
    print('FFT|%s|%s| e_cpu=%.3g e_fft=%.3g floor=%.3g e_fft/max(e_cpu,floor)=%.2f'
          % (preset, cls, e_cpu, e_fft, floor, e_fft / max(e_cpu, floor)))
    assert torch.isfinite(R).all()
    if cls in ('noise', 'synth', 'int16'):
        assert max(e_cpu, e_fft) <= 1e-3


def test_silence_sits_on_the_clamp():
    sd = FR.state('16k')
    wave = _wave('silence', '16k')
    db = FR.ref_logmel(sd, wave, torch.float64)
    assert (db[0] == -100.0).all() and (db[1] > -100.0).all()


def test_int16_class_has_the_edge_codes():
    q = _wave('int16', '8k')
    assert q.dtype == np.int16 and q[0, :5].tolist() == [32767, -32768, 0, 1, -1]
    assert FR.as_float(q).dtype == np.float32 and FR.as_float(q)[0, 1] < -1.0


def test_window_slices():
    w = np.arange(1, 21, dtype=np.float32).reshape(2, 10)
    s = FR.window_slices(w, [0, 4, 8], 4)
    assert s.shape == (6, 4)
    assert s[1].tolist() == [5, 6, 7, 8] and s[2].tolist() == [9, 10, 0, 0] and s[5].tolist() == [19, 20, 0, 0]


# ---------------------------------------------------------------------------
# the banks reach the regimes they are named for
# ---------------------------------------------------------------------------
def test_lds_caps():
    # fe_mel_lds<N>() / 4 of csrc/frontend.hip: ((2 (N/2 + 1) 4 + 255) / 256) 256 bytes
    assert [FR.mel_lds_cap(n) for n in (256, 512, 1024)] == [320, 576, 1088]


@pytest.mark.parametrize('preset', FR.PRESETS)
def test_preset_and_full_banks_stay_on_the_fast_paths(preset):
    n_fft = O.PRESETS[preset]['window_size']
    for kind in ('preset', 'full'):
        w = FR.bank(kind, preset)
        g = FR.regime(w)
        assert w.dtype == np.float32 and w.shape == (n_fft // 2 + 1, 64)
        assert g['nnz'] <= FR.mel_lds_cap(n_fft)
        assert not w[0].any() and not w[-1].any()          # no Slaney bank weighs DC or Nyquist
        if n_fft == 512:
            assert g['wmax'] <= FR.FE16_MEL_MW and 0 < g['mt_floats'] <= FR.FE_MT_MAX_FLOATS
    if n_fft == 512:
        # fmax = sr / 2: the last band tile's 4-bin steps run past bin 256 (the MFMA path's clamp)
        assert FR.regime(FR.bank('full', preset))['mt_clamp']
        assert not FR.regime(FR.bank('preset', preset))['mt_clamp']


def test_sparse_bank_has_empty_and_one_bin_bands():
    g = FR.regime(FR.bank('sparse', '16k'))
    assert set(g['width'].tolist()) == {0, 1} and (g['width'] == 0).sum() >= 2
    assert g['wmax'] <= FR.FE16_MEL_MW and g['mt_floats'] <= FR.FE_MT_MAX_FLOATS


def test_wide_bank_takes_the_per_band_lds_loop():
    w = FR.bank('wide', '16k')
    g = FR.regime(w)
    assert g['width'].max() == FR.WIDE_BINS and g['wmax'] == 40 > FR.FE16_MEL_MW
    assert g['nnz'] <= FR.mel_lds_cap(512)
    assert (w >= 0).all() and g['mt_floats'] <= FR.FE_MT_MAX_FLOATS


@pytest.mark.parametrize('preset', FR.PRESETS)
def test_dense_bank_takes_the_global_loop(preset):
    n_fft = O.PRESETS[preset]['window_size']
    w = FR.bank('dense', preset)
    g = FR.regime(w)
    assert 4100 <= g['nnz'] <= 4700 and g['nnz'] > max(FR.mel_lds_cap(n) for n in (256, 512, 1024))
    assert w[0, 0] > 0 and w[-1, 63] > 0                   # DC in band 0, Nyquist in band 63
    assert (w >= 0).all()
    s, wd = FR.DENSE[n_fft]
    assert g['lo'].tolist() == [s * m for m in range(64)] and g['width'][:63].tolist() == [wd + 1] * 63
    if n_fft == 512:
        assert g['wmax'] > FR.FE16_MEL_MW
        # (3, 64) keeps the MFMA table under its limit (the table path with the
        # bin clamp); dense_mt is the bank past it (the fall-back to band sums)
        assert g['mt_floats'] <= FR.FE_MT_MAX_FLOATS and g['mt_clamp']


def test_dense_mt_bank_exceeds_the_mfma_table():
    w = FR.bank('dense_mt', '16k')
    g = FR.regime(w)
    assert g['mt_floats'] > FR.FE_MT_MAX_FLOATS
    assert g['nnz'] > FR.mel_lds_cap(512) and w[0, 0] > 0 and w[-1, 63] > 0


@pytest.mark.parametrize('fit', [False, True], ids=['1s', 'fit'])
@pytest.mark.parametrize('preset', ['16k', '8k'])
def test_gamma_cases_keep_clear_of_rounding_boundaries(preset, fit):
    """The int16 codes of the GPU test (test_gamma_codes_vs_oracle_low_rates)
    truncate x 32767; every float64 value stays 1e-6 or more from an integer,
    so a differing code is an error of the kernel, not a tie."""
    audio, codes, margin = FR.gamma_case(preset, fit)
    nfft, hop = FR.GAMMA_NFFT[preset], O.PRESETS[preset]['hop_size']
    assert audio.shape[0] == 3 and ((audio.shape[1] - nfft) % hop == 0) == fit
    assert codes.shape == (3, 64, 1 + (audio.shape[1] - nfft) // hop)
    print('gamma %s fit=%s: margin %.3g' % (preset, fit, margin))
    assert margin >= 1e-6
