"""References of the log-mel front end alone (test infrastructure only):
``oracle.sed_oracle.logmel`` followed by ``bn0`` in float64 / float32, an fp32
FFT restatement of the kernel's algorithm class, the filter banks and input
classes of tests/test_gpu_frontend.py, and the host's mel-table geometry
(csrc/weights.cpp: mel_tables) restated so the banks can be shown to reach the
kernel paths they are named for.

CPU only; nothing here imports the library.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import sed_oracle as O
from sedx import synth

FAVG = 'Cnn_9layers_FrameAvg'
SEED = synth.GOLDEN_SEEDS[FAVG]
PRESETS = ('8k', '16k', '32k')
WR, WI, MELW = ('spectrogram_extractor.stft.conv_real.weight', 'spectrogram_extractor.stft.conv_imag.weight',
                'logmel_extractor.melW')
BN0 = ('bn0.weight', 'bn0.bias', 'bn0.running_mean', 'bn0.running_var')
# csrc/weights.h
FE16_MEL_MW = 36                # widest band of logmel512_kernel's table path
FE_MT_MAX_FLOATS = 8192         # MFMA mel table limit
# (band step s, band width w) of the ``dense`` bank per n_fft
DENSE = {256: (1, 65), 512: (3, 64), 1024: (7, 71)}
WIDE_BINS = 40


def preset_args(preset, fmin=None, fmax=None):
    """Constructor arguments (sample_rate .. fmax) of a preset."""
    p = O.PRESETS[preset]
    return (p['sample_rate'], p['window_size'], p['hop_size'], p['mel_bins'],
            p['fmin'] if fmin is None else fmin, p['fmax'] if fmax is None else fmax)


def mel_lds_cap(n_fft):
    """Floats of LDS the launch gives the packed band weights: fe_mel_lds<N>() / 4
    of csrc/frontend.hip (2 (N/2 + 1) floats rounded up to 256 bytes)."""
    return (2 * (n_fft // 2 + 1) * 4 + 255) // 256 * 256 // 4


# ---------------------------------------------------------------------------
# filter banks [n_fft/2 + 1, 64] float32
# ---------------------------------------------------------------------------
def bank(kind, preset, seed=0):
    p = O.PRESETS[preset]
    sr, n_fft = p['sample_rate'], p['window_size']
    K = n_fft // 2 + 1
    mk = lambda lo, hi: O.mel_filterbank(sr, n_fft, 64, lo, hi)
    if kind == 'preset':
        return mk(p['fmin'], p['fmax'])
    if kind == 'full':
        return mk(0, sr // 2)
    if kind == 'sparse':
        return mk(0, sr // 16)                      # (16 kHz, 0-1000 Hz): bands of width 0 and 1
    rng = np.random.default_rng(1000 + seed)
    if kind == 'wide':
        # band 40 becomes a positive ramp of 40 bins that keeps the band's area
        w = mk(p['fmin'], p['fmax'])
        m = 40
        lo = int(np.flatnonzero(w[:, m])[0])
        assert lo + WIDE_BINS <= K
        ramp = np.arange(1, WIDE_BINS + 1, dtype=np.float64)
        area = float(w[:, m].sum())
        w[:, m] = 0
        w[lo:lo + WIDE_BINS, m] = (ramp * area / ramp.sum()).astype(np.float32)
        return w
    if kind in ('dense', 'dense_mt'):
        # band m covers bins [s m, s m + w], positive weights of about 1 / w;
        # band 0 holds the DC bin, band 63 reaches the Nyquist bin.  dense_mt
        # (n_fft 512) is the bank whose MFMA table exceeds FE_MT_MAX_FLOATS
        s, wd = DENSE[n_fft] if kind == 'dense' else (2, 100)
        w = np.zeros((K, 64), np.float32)
        for m in range(64):
            hi = K - 1 if m == 63 else s * m + wd
            assert hi < K
            w[s * m:hi + 1, m] = (rng.uniform(0.5, 1.5, hi + 1 - s * m) / wd).astype(np.float32)
        return w
    raise ValueError(kind)


def regime(melW):
    """Geometry of csrc/weights.cpp mel_tables for a bank: band first bins and
    widths (first to last non-zero weight), nnz (floats of the packed runs),
    mel_wmax (widest band rounded up to 4) and, for n_fft 512, the MFMA table's
    floats (per 16-band tile the covered bin range in 4-bin steps x 64) and
    whether a tile's last step reaches past bin 256 (the kernel's bin clamp)."""
    melW = np.asarray(melW)
    K = melW.shape[0]
    lo, width = np.zeros(64, np.int64), np.zeros(64, np.int64)
    for m in range(64):
        nz = np.flatnonzero(melW[:, m])
        if nz.size:
            lo[m], width[m] = nz[0], nz[-1] - nz[0] + 1
    r = dict(lo=lo, width=width, nnz=int(width.sum()), wmax=int((width.max() + 3) & ~3))
    if K == 257:
        mt, clamp = 0, False
        for j in range(4):
            sel = [m for m in range(16 * j, 16 * j + 16) if width[m] > 0]
            if not sel:
                continue
            klo = min(lo[m] for m in sel)
            khi = max(lo[m] + width[m] - 1 for m in sel)
            ns = (khi - klo + 1 + 3) // 4
            mt += 64 * ns
            clamp = clamp or klo + 4 * (ns - 1) + 3 > K - 1
        r.update(mt_floats=int(mt), mt_clamp=bool(clamp))
    return r


# ---------------------------------------------------------------------------
# state dicts and the references
# ---------------------------------------------------------------------------
def state(preset, melW=None, seed=SEED):
    """The tensors of the reference model's front end (fp32, as it holds them)
    plus bn0 of ``synth.make_state_dict`` and the oracle's '_hop'."""
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in O.frontend_state(preset).items()}
    if melW is not None:
        sd[MELW] = torch.from_numpy(np.ascontiguousarray(melW, dtype=np.float32))
    w = synth.make_state_dict(FAVG, seed=seed)
    for k in BN0:
        sd[k] = torch.from_numpy(w[k])
    sd['_hop'] = O.PRESETS[preset]['hop_size']
    return sd


def _cast(sd, dtype):
    return {k: (torch.as_tensor(v).to(dtype) if k != '_hop' else v) for k, v in sd.items()
            if k == '_hop' or k in (WR, WI, MELW) + BN0}


def _wave(wave, dtype):
    return torch.as_tensor(np.asarray(wave)).to(dtype)


def ref_logmel(sd, wave, dtype):
    """``O.logmel`` in ``dtype`` (the fp32 tensors cast up): [B, T, 64] dB."""
    with torch.no_grad():
        return O.logmel(_cast(sd, dtype), _wave(wave, dtype))[:, 0]


def ref_x0(sd, wave, dtype):
    """``O.logmel`` then ``O.bn0`` in ``dtype``: [B, T, 64], the layout of capture 0."""
    s = _cast(sd, dtype)
    with torch.no_grad():
        return O.bn0(s, O.logmel(s, _wave(wave, dtype)))[:, 0]


def _frames(sd, wave, dtype):
    """Reflect-padded frames [B, T, n_fft] of wave [B, L]."""
    n_fft = sd[WR].shape[-1]
    x = F.pad(_wave(wave, dtype)[:, None, :], (n_fft // 2, n_fft // 2), mode='reflect')[:, 0]
    return x.unfold(1, n_fft, sd['_hop'])


def _pick(fr, flat):
    """Frames b T + t of the (unfolded, not copied) frame view [B, T, n_fft]."""
    flat = torch.as_tensor(np.asarray(flat), dtype=torch.long)
    return fr[flat // fr.shape[1], flat % fr.shape[1]]


def _db_bn0(s, mel):
    db = 10.0 * torch.log10(torch.clamp(mel, min=1e-10))
    return O.bn0(s, db[:, None])[:, 0]


def fft_logmel(sd, wave):
    """fp32 restatement of the kernel's algorithm class before bn0: reflect
    pad, frame, times the window (row 0 of conv_real), rfft, re^2 + im^2,
    @ melW, 10 log10(clamp(., 1e-10)).  [B, T, 64]."""
    s = _cast(sd, torch.float32)
    with torch.no_grad():
        z = torch.fft.rfft(_frames(s, wave, torch.float32) * s[WR][0, 0], dim=-1)
        mel = torch.matmul(z.real ** 2 + z.imag ** 2, s[MELW])
        return 10.0 * torch.log10(torch.clamp(mel, min=1e-10))


def fft_x0(sd, wave):
    """``fft_logmel`` then bn0 (fp32): supplies e_fft of the yardstick."""
    s = _cast(sd, torch.float32)
    with torch.no_grad():
        return O.bn0(s, fft_logmel(sd, wave)[:, None])[:, 0]


def ref_x0_frames(sd, wave, flat, dtype):
    """``ref_x0`` of the frames with flat index b T + t in ``flat`` only
    ([n, 64]): the oracle's two convolutions applied to those frames alone."""
    s = _cast(sd, dtype)
    with torch.no_grad():
        fr = _frames(s, wave, dtype)
        fr = _pick(fr, flat)
        re = F.conv1d(fr[:, None, :], s[WR])[:, :, 0]
        im = F.conv1d(fr[:, None, :], s[WI])[:, :, 0]
        return _db_bn0(s, torch.matmul(re ** 2 + im ** 2, s[MELW])[None])[0]


def fft_x0_frames(sd, wave, flat):
    s = _cast(sd, torch.float32)
    with torch.no_grad():
        fr = _frames(s, wave, torch.float32)
        fr = _pick(fr, flat)
        z = torch.fft.rfft(fr * s[WR][0, 0], dim=-1)
        return _db_bn0(s, torch.matmul(z.real ** 2 + z.imag ** 2, s[MELW])[None])[0]


def window_slices(wave, starts, length):
    """The pad_truncate'd window batch of window mode: wave [B, L] ->
    [B * len(starts), length], clip-major, zeros past the clip's end."""
    wave = np.asarray(wave)
    out = np.zeros((wave.shape[0], len(starts), length), wave.dtype)
    for i, s in enumerate(starts):
        seg = wave[:, s:s + length]
        out[:, i, :seg.shape[1]] = seg
    return out.reshape(-1, length)


# ---------------------------------------------------------------------------
# input classes (all seeded)
# ---------------------------------------------------------------------------
def clip_len(preset, T, r):
    """L = hop (T - 1) + r: T frames, r samples past the last hop."""
    return O.PRESETS[preset]['hop_size'] * (T - 1) + r


def inputs(kind, preset, B, L, seed=0):
    """[B, L] float32 (int16 for ``int16``)."""
    sr = O.PRESETS[preset]['sample_rate']
    rng = np.random.default_rng(77 + seed)
    n = np.arange(L, dtype=np.float64)
    if kind == 'noise':
        return (0.3 * rng.standard_normal((B, L))).astype(np.float32)
    if kind == 'synth':
        return np.ascontiguousarray(synth.make_waveforms(B, seconds=(L + 1.0) / sr, sample_rate=sr,
                                                         seed=77 + seed)[:, :L])
    if kind == 'tone':
        out = np.empty((B, L), np.float32)
        for b in range(B):
            if b % 2 == 0:
                x = 0.8 * np.sin(2 * np.pi * 0.31 * n + 0.7 * b) + 1e-4 * rng.standard_normal(L)
            else:
                x = np.sin(2 * np.pi * 440.0 / sr * n + 0.3 * b)
            out[b] = x.astype(np.float32)
        return out
    if kind == 'silence':
        out = np.zeros((B, L), np.float32)
        out[1::2] = (1e-4 * rng.standard_normal((len(out[1::2]), L))).astype(np.float32)
        return out
    if kind == 'int16':
        x = np.clip(0.3 * rng.standard_normal((B, L)), -1.0, 1.0)
        q = (x * 32767).astype(np.int16)
        q[0, :5] = [32767, -32768, 0, 1, -1]
        return q
    raise ValueError(kind)


def as_float(wave):
    """What the front end computes on: int16 batches dequantised as the
    reference does (``O.int16_to_float32``)."""
    wave = np.asarray(wave)
    return O.int16_to_float32(wave) if wave.dtype == np.int16 else wave


# ---------------------------------------------------------------------------
# gammatone codes at the 16 kHz / 8 kHz presets
# ---------------------------------------------------------------------------
GAMMA_NFFT = {'8k': 512, '16k': 1024, '32k': 2048}
GAMMA_SEEDS = {('16k', False): 51, ('16k', True): 52, ('8k', False): 53, ('8k', True): 54}


def gamma_case(preset, fit):
    """3 clips of about 1 s (``fit``: (L - nfft) % hop == 0, specgram's loop
    leaves the last column unfilled) -> (audio [3, L] float32, the oracle's
    int16 codes [3, 64, T] as int32, the smallest distance of a float64
    pre-truncation value x 32767 from an integer)."""
    p = O.PRESETS[preset]
    sr, hop, nfft = p['sample_rate'], p['hop_size'], GAMMA_NFFT[preset]
    L = nfft + hop * 90 if fit else sr
    audio = np.ascontiguousarray(synth.make_waveforms(3, seconds=1.2, sample_rate=sr,
                                                      seed=GAMMA_SEEDS[(preset, fit)])[:, :L])
    codes, margin = [], np.inf
    for a in audio:
        db = O.power_to_db(O.fft_gtgram(a, sr, p['window_size'] / sr, hop / sr, 64, p['fmin']))
        top = np.max(np.abs(db))
        x = db / top * 32767.0 if top > 1.0 else db * 32767.0
        # (the cells that hold the clip's max |dB| are +-32767 exactly, by construction)
        margin = min(margin, float(np.min(np.abs(x - np.round(x))[np.abs(db) != top])))
        codes.append(O.float32_to_int16(db).astype(np.int32))
    return audio, np.stack(codes), margin
