"""Windowed inference of a gammatone model: the cases of
tests/test_gamma_windows_cpu.py and tests/test_gpu_gamma_windows.py and their
oracle (test infrastructure only; CPU, nothing here imports the library).

The reference has no such path (predict.py raises on a gamma model): its features
are made per clip when the HDF5 files are packed (utils/features.py:356-370).
The oracle treats a window as that packing treats a clip, by composing functions
oracle/sed_oracle.py already has:

    pad_truncate_sequence -> fft_gtgram -> power_to_db(top_db 80)
    -> float32_to_int16 (the WINDOW's own max |dB|) -> int16_to_float32
    -> forward(features=...) -> merge -> avg_merge (or binarize_pred -> merge)

with window_starts / driver_stride as the loop.  tools/make_golden_gamma_windows.py
records its results in tests/golden/gamma_windows.{json,npz}.
"""
import collections
import functools

import numpy as np

import gamma_refs as G
from oracle import sed_oracle as O
from sedx import synth

GRU = 'Cnn_9layers_Gru_FrameAtt'
# every oracle framewise value keeps this distance from every threshold a test applies to it: 5 x the 2e-5 the
# Winograd forms are held to per layer, so a GPU value within tolerance falls on the oracle's side
THRESHOLD_MARGIN = 1e-4

# lengths in samples; dur: per-clip loop bounds in seconds (None: the clip's own length)
# seed: the waveform's (synth.make_waveforms); wseed: the weights' (synth.make_state_dict)
# high, low: the event thresholds of the case (low is also the vote mode's binarisation threshold).  The
# synthetic weights give every class a nearly constant output whatever the waveform, and avg_merge's divisor
# schedule turns those constants into hundreds of levels, so the distance from a threshold is a property of the
# weights and the thresholds: the 32 kHz case takes weight seed 5 (seeds 0-4 come within 9e-5 of 0.5 / 0.3), and
# the main_strong case, whose 476 levels come within 4e-5 of 0.5 / 0.3 under every weight seed 0-12, takes
# 0.55 / 0.35
Case = collections.namedtuple('Case', 'preset seed lengths sd ov driver dur wseed high low')
CASES = {
    # 4.0 / 5.3 / 2.0 s in 2 s windows: 3 / 4 / 1 windows of T = 194 frames (three ERB tiles and a partial one)
    '8k': Case('8k', 3, (32000, 42400, 16000), 2, 1.0, 'predict', None, 0, 0.5, 0.3),
    # odd lengths: clip 1 starts at an odd sample of the concatenated buffer
    '8k-odd': Case('8k', 4, (17001, 40003, 16000), 2, 1.0, 'predict', None, 0, 0.5, 0.3),
    # a loop bound past the samples: the second window's last 4000 samples are pad_truncate's zeros
    '8k-pad': Case('8k', 3, (20000,), 2, 1.0, 'predict', (3.2,), 0, 0.5, 0.3),
    # 7.2 s in 5 s windows: 3 windows of T = 494 (nfft 2048: both spectrum kernels)
    '32k': Case('32k', 3, (230400,), 5, 1.0, 'predict', None, 5, 0.5, 0.3),
    # main_strong (overlap_value 0.5, sample_duration 6) on a 10.5 s file: the clip is cut to 10 s, nine full
    # windows (T = 594) and a shorter tail window (44000 samples, T = 544) as its own group; the vote merge runs
    # on the same windows.  (An 11 s file's second tail window has 500 frames and numpy's merge raises.)
    '8k-ms': Case('8k', 4, (84000,), 6, 0.5, 'main_strong', None, 0, 0.55, 0.35),
}


def params(name):
    c = CASES[name]
    return {'audio_tagging_threshold': 0.099, 'sed_high_threshold': c.high, 'sed_low_threshold': c.low,
            'n_smooth': 10, 'n_salt': 10}


def sample_rate(case):
    return O.PRESETS[case.preset]['sample_rate']


@functools.lru_cache(maxsize=None)
def clips(name):
    """The case's clips: one seeded waveform cut at the lengths (float32)."""
    c = CASES[name]
    sr = sample_rate(c)
    cat = synth.make_waveforms(1, seconds=sum(c.lengths) / float(sr), sample_rate=sr, seed=c.seed)[0]
    assert cat.shape[0] == sum(c.lengths)
    off = np.concatenate([[0], np.cumsum(c.lengths)])
    return [np.ascontiguousarray(cat[off[i]:off[i + 1]]) for i in range(len(c.lengths))]


def durations(name):
    c = CASES[name]
    return [None] * len(c.lengths) if c.dur is None else list(c.dur)


def windows_of(name, clip):
    """[n_win] float32 windows of clip `clip` as the model's frontend receives them: predict.py pad_truncate's every
    window (:302-305); main_strong pad_truncate's the clip to 10 s and slices (:790-797)."""
    c = CASES[name]
    sr = sample_rate(c)
    audio = clips(name)[clip]
    dur = durations(name)[clip]
    dur = len(audio) / float(sr) if dur is None else dur
    if c.driver == 'main_strong':
        audio = O.pad_truncate_sequence(audio, sr * 10)
    out = []
    for start in O.window_starts(dur, c.sd, O.driver_stride(c.driver, c.sd, c.ov)):
        s = int(start * sr)
        seg = audio[s:int(c.sd * sr) + s]
        if c.driver == 'predict':
            seg = O.pad_truncate_sequence(seg, int(sr * c.sd))
        out.append(np.asarray(seg, np.float32))
    return out


@functools.lru_cache(maxsize=None)
def state(preset, wseed):
    return O.full_state(synth.make_state_dict(GRU, seed=wseed), preset)


Window = collections.namedtuple('Window', 'codes guarded framewise')
Clip = collections.namedtuple('Clip', 'windows merged votes')


def window_oracle(seg, preset, wseed):
    """One window: its int16 codes [64, T], the tie-guarded cells, the model's framewise output [frames, C]."""
    o = G.oracle(seg[None], preset)
    feats = O.int16_to_float32(o.codes[0].astype(np.int16))          # [64, T]
    fw = O.forward(state(preset, wseed), GRU, features=feats.T[None, None])['framewise_output'].numpy()[0]
    return Window(o.codes[0].astype(np.int16), o.guarded[0], fw)


def _merge_all(frames, c):
    merged, prev = None, None
    for k, curr in enumerate(frames, start=1):
        curr = curr[None]
        merged = curr if k == 1 else O.merge(prev if k == 2 else merged, curr, c.sd, k, c.ov)
        prev = curr
    return merged


@functools.lru_cache(maxsize=None)
def clip_oracle(name, clip):
    """The windows of one clip, their averaged merge [N, C] and (main_strong) the vote merge [N, C]."""
    c = CASES[name]
    wins = [window_oracle(w, c.preset, c.wseed) for w in windows_of(name, clip)]
    merged = O.avg_merge(np.array(_merge_all([w.framewise for w in wins], c), copy=True), c.sd, c.ov)[0]
    votes = None
    if c.driver == 'main_strong':
        votes = _merge_all([O.binarize_pred(w.framewise[None], c.low)[0] for w in wins], c)[0]
    return Clip(wins, merged.astype(np.float32), votes)


def threshold_distance(name):
    """The smallest distance of an oracle framewise value of the case from a threshold a test applies to it: the
    event thresholds on the merged output and, in vote mode, the binarisation threshold on every window."""
    c = CASES[name]
    d = np.inf
    for i in range(len(c.lengths)):
        o = clip_oracle(name, i)
        for thr in (c.high, c.low):
            d = min(d, float(np.min(np.abs(o.merged.astype(np.float64) - thr))))
        if o.votes is not None:
            for w in o.windows:
                d = min(d, float(np.min(np.abs(w.framewise.astype(np.float64) - c.low))))
    return d


def guarded_cells(name):
    c = CASES[name]
    return sum(int(w.guarded.sum()) for i in range(len(c.lengths)) for w in clip_oracle(name, i).windows)


def events(name):
    """Per clip, the oracle's events of the averaged merge (the tests compare them as sorted tuples)."""
    c = CASES[name]
    return [O.events_from_framewise(clip_oracle(name, i).merged[None], params(name), audio_name='clip%d' % i, sort=True)
            for i in range(len(c.lengths))]


def vote_events(name):
    c = CASES[name]
    return [O.events_from_votes(clip_oracle(name, i).votes[None], c.ov, c.sd, params(name), audio_name='clip%d' % i)
            for i in range(len(c.lengths))]
