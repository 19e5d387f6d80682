"""SED threshold calibration (utils/optimize_thresholds.py
``optimize_sed_thresholds``): produces the per-class threshold dictionary that
``inference.events_from_framewise`` consumes.

The reference takes numerical gradients of the segment-based F1 (1 s grid)
over 75 parameters with up to ``max_search`` probes each and re-runs
``activity_detection`` over the whole validation set for every probe.
Perturbing parameter k only changes class k mod C and the segment counts are
additive over classes, so here one gradient epoch is ONE call of the fused
segment-count kernel (csrc/calib.hip) with V = 1 + 2 max_search threshold
variants per class; the optimiser loop around it restates
``HyperParamsOptimizer`` + ``Adam`` (optimize_thresholds.py:31-141) in float64.

The segment metric follows the definition utilities.py:294-340 asks of
``sed_eval`` (segment-based, time_resolution 1.0: an event's onset is floored
and its offset ceiled to the grid).  Deviation: F = 0.0 where Ntp = 0 (the
toolbox leaves it undefined there).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .inference import LABELS, _ptr, event_pairs

MAX_SEGMENTS = 64       # the fused path's segment mask is one 64-bit word
MAX_VARIANTS = 64
_BAD = ('a run begins at the last frame after the find_bgn_fin_pairs quirk '
        '(the reference raises IndexError there)')


# ---- targets ---------------------------------------------------------------

def _load_reference_csv(path):
    """The reference's ground-truth files: filename, onset, offset, event_label
    per line, tab or comma separated, no header."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            cols = line.split('\t') if '\t' in line else line.split(',')
            if len(cols) < 4:
                continue                      # a file without events
            out.append({'filename': cols[0], 'onset': float(cols[1]), 'offset': float(cols[2]),
                        'event_label': cols[3]})
    return out


def segment_targets(reference_events, audio_names, labels=LABELS, n_segments=10, time_resolution=1.0):
    """uint8 [N, S, C]: class active in segment s of clip n.  reference_events
    is a list of {'filename','onset','offset','event_label'} or the path of a
    ground-truth CSV; onsets are floored and offsets ceiled to the grid
    (segments past n_segments are dropped, unknown files / labels ignored)."""
    if isinstance(reference_events, str):
        reference_events = _load_reference_csv(reference_events)
    clip = {name: i for i, name in enumerate(audio_names)}
    cls = {name: i for i, name in enumerate(labels)}
    out = np.zeros((len(audio_names), n_segments, len(labels)), np.uint8)
    for e in reference_events:
        n, k = clip.get(e['filename']), cls.get(e['event_label'])
        if n is None or k is None:
            continue
        s0 = max(int(math.floor(e['onset'] * 1 / time_resolution)), 0)
        s1 = min(int(math.ceil(e['offset'] * 1 / time_resolution)), n_segments)
        out[n, s0:s1, k] = 1
    return out


def pack_targets(targets):
    """uint8 [N, S, C] (S <= 64) -> uint64 [N, C] masks, bit s = segment s."""
    t = np.asarray(targets)
    N, S, C = t.shape
    if S > MAX_SEGMENTS:
        raise ValueError('%d segments do not fit a 64-bit mask' % S)
    w = (np.uint64(1) << np.arange(S, dtype=np.uint64))[None, :, None]
    return np.ascontiguousarray(((t != 0).astype(np.uint64) * w).sum(axis=1, dtype=np.uint64))


# ---- counts ----------------------------------------------------------------

def _per_class(v, C, dtype):
    a = np.asarray(v, dtype=dtype)
    return np.ascontiguousarray(np.broadcast_to(a, (C,)) if a.ndim == 0 else a.reshape(C))


def _variants(v, C):
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full((1, C), float(a))
    elif a.ndim == 1:
        a = a.reshape(1, C)
    return np.ascontiguousarray(a)


def _c(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _fail(st, what):
    msg = _lib.lib().sedx_last_error(None).decode()
    raise RuntimeError('libsedx %s failed (%s): %s' % (what, _lib.STATUS.get(st, st), msg))


def segment_counts_fallback(framewise, targets, high, low, n_smooth=10, n_salt=10, segment_frames=100):
    """The per-candidate path: inference.event_pairs per variant, events
    rasterised onto the segment grid in numpy.  Any S and V; targets uint8
    [N, S, C].  Same int64 [V, C, 4] = (tp, fp, fn, bad) as segment_counts."""
    N, T, C = framewise.shape
    S = (T + segment_frames - 1) // segment_frames
    ref = np.asarray(targets)[:, :S] != 0
    if ref.shape != (N, S, C):
        raise ValueError('targets %s, expected %s' % (ref.shape, (N, S, C)))
    high, low = _variants(high, C), _variants(low, C)
    ns, nsalt = _per_class(n_smooth, C, np.int64), _per_class(n_salt, C, np.int64)
    out = np.zeros((high.shape[0], C, 4), np.int64)
    for v in range(high.shape[0]):
        params = {'sed_high_threshold': high[v].tolist(), 'sed_low_threshold': low[v].tolist(),
                  'n_smooth': ns.tolist(), 'n_salt': nsalt.tolist()}
        bad = np.zeros((N, C), bool)
        try:
            pairs = event_pairs(framewise, params)
        except RuntimeError:                 # some series is the reference's IndexError: find which
            rows = []
            for n in range(N):
                for k in range(C):
                    one = {key: [val[k]] for key, val in params.items()}
                    try:
                        p = event_pairs(framewise[n:n + 1, :, k:k + 1], one)
                    except RuntimeError:
                        bad[n, k] = True
                        continue
                    p = np.asarray(p).copy()
                    p[:, 0], p[:, 1] = n, k
                    rows.append(p)
            pairs = np.concatenate(rows) if rows else np.zeros((0, 4), np.int32)
        # events -> segments [bgn / seg, ceil(fin / seg)) as +1 / -1 marks and a running sum
        pairs = np.asarray(pairs, np.int64).reshape(-1, 4)
        s0 = pairs[:, 2] // segment_frames
        s1 = np.maximum(-(-pairs[:, 3] // segment_frames), s0)
        mark = np.zeros((N, S + 1, C), np.int64)
        np.add.at(mark, (pairs[:, 0], s0, pairs[:, 1]), 1)
        np.add.at(mark, (pairs[:, 0], s1, pairs[:, 1]), -1)
        est = np.cumsum(mark, axis=1)[:, :S] > 0
        ok = ~bad[:, None, :]
        out[v, :, 0] = (est & ref & ok).sum(axis=(0, 1))
        out[v, :, 1] = (est & ~ref & ok).sum(axis=(0, 1))
        out[v, :, 2] = (ref & ~est & ok).sum(axis=(0, 1))
        out[v, :, 3] = bad.sum(axis=0)
    return out


class _Counter:
    """segment_counts for one fixed (framewise, targets): the inputs are laid
    out (and, for a HIP tensor, uploaded) once, then called per epoch."""

    def __init__(self, framewise, targets, n_smooth, n_salt, segment_frames):
        self.device = isinstance(framewise, torch.Tensor) and framewise.device.type == 'cuda'
        if self.device:
            self.x = framewise.detach().to(torch.float32).contiguous()
        else:
            fw = framewise.detach().cpu().numpy() if isinstance(framewise, torch.Tensor) else np.asarray(framewise)
            self.x = np.ascontiguousarray(fw, dtype=np.float32)
        self.N, self.T, self.C = (int(d) for d in self.x.shape)
        self.seg = int(segment_frames)
        self.S = (self.T + self.seg - 1) // self.seg if self.seg >= 1 else 0
        self.ns, self.nsalt = _per_class(n_smooth, self.C, np.int64), _per_class(n_salt, self.C, np.int64)
        t = targets.cpu().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
        self.targets = t
        self.fused = self.seg >= 1 and self.S <= MAX_SEGMENTS
        if not self.fused:
            return
        if t.ndim == 3:
            t = pack_targets(t[:, :self.S])
        self.masks = np.ascontiguousarray(t, dtype=np.uint64)
        if self.masks.shape != (self.N, self.C):
            raise ValueError('targets %s, expected masks %s' % (self.masks.shape, (self.N, self.C)))
        if self.device:
            dev = self.x.device
            self.d_masks = torch.from_numpy(self.masks.view(np.int64)).to(dev)
            self.ws = None

    def __call__(self, high, low):
        high, low = _variants(high, self.C), _variants(low, self.C)
        V = high.shape[0]
        if low.shape != high.shape:
            raise ValueError('high %s and low %s differ' % (high.shape, low.shape))
        if not self.fused or V > MAX_VARIANTS:
            if self.targets.ndim != 3:
                raise ValueError('the per-candidate path needs uint8 [N, S, C] targets')
            return segment_counts_fallback(self.x, self.targets, high, low, self.ns, self.nsalt, self.seg)
        L = _lib.lib()
        if not self.device:
            counts = np.zeros((V, self.C, 4), np.int64)
            st = L.sedx_segment_counts(_c(self.x), self.N, self.T, self.C, _c(self.masks), self.seg, V,
                                       _c(high), _c(low), _c(self.ns), _c(self.nsalt), _c(counts))
            if st != _lib.SEDX_OK:
                _fail(st, 'segment_counts')
            return counts
        dev = self.x.device
        wsz = ctypes.c_size_t()
        st = L.sedx_segment_counts_workspace_size(self.N, self.T, self.C, V, ctypes.byref(wsz))
        if st != _lib.SEDX_OK:
            _fail(st, 'segment_counts_workspace_size')
        if self.ws is None or self.ws.numel() < wsz.value:
            self.ws = torch.empty(max(wsz.value, 1), dtype=torch.uint8, device=dev)
        counts = torch.empty((V, self.C, 4), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            st = L.sedx_segment_counts_device(_ptr(self.x), self.N, self.T, self.C, _ptr(self.d_masks), self.seg, V,
                                              _c(high), _c(low), _c(self.ns), _c(self.nsalt), _ptr(counts),
                                              _ptr(self.ws), self.ws.numel(), stream)
            if st != _lib.SEDX_OK:
                _fail(st, 'segment_counts_device')
            return counts.cpu().numpy()


def segment_counts(framewise, targets, high, low, n_smooth=10, n_salt=10, segment_frames=100):
    """Segment-based (tp, fp, fn, bad) of activity_detection for V threshold
    variants: int64 [V, C, 4].  framewise [N, T, C]; targets uint8 [N, S, C]
    (segment_targets) or packed uint64 [N, C]; high / low [V, C], [C] or scalar.
    A HIP tensor runs the fused kernel (sedx_segment_counts_device), anything
    else the host entry; more than 64 segments or variants take the
    per-candidate path (segment_counts_fallback).  `bad` counts the series the
    reference raises IndexError on; they add nothing to tp / fp / fn."""
    return _Counter(framewise, targets, n_smooth, n_salt, segment_frames)(high, low)


# ---- metrics ---------------------------------------------------------------

def _prf(tp, fp, fn):
    """P = Ntp / Nsys, R = Ntp / Nref, F = 2PR / (P + R); 0.0 where Ntp = 0."""
    tp, fp, fn = int(tp), int(fp), int(fn)
    if tp == 0:
        return 0.0, 0.0, 0.0
    p = tp / float(tp + fp)
    r = tp / float(tp + fn)
    return p, r, 2 * p * r / (p + r)


def _metrics_from_counts(counts):
    counts = np.asarray(counts, np.int64)
    if counts.ndim != 2 or counts.shape[1] < 3:
        raise ValueError('counts [C, 4] expected (one variant of segment_counts)')
    tot = counts.sum(axis=0)
    p, r, f = _prf(tot[0], tot[1], tot[2])
    cw = [_prf(*row[:3]) for row in counts]
    return {'overall': {'precision': p, 'recall': r, 'f_measure': f,
                        'Ntp': int(tot[0]), 'Nfp': int(tot[1]), 'Nfn': int(tot[2])},
            'class_wise': {'precision': [c[0] for c in cw], 'recall': [c[1] for c in cw],
                           'f_measure': [c[2] for c in cw]}}


def segment_metrics(counts_or_events, reference_events=None, audio_names=None, labels=LABELS, n_segments=10,
                    time_resolution=1.0):
    """Overall and class-wise precision / recall / F1 of the segment-based
    metric.  From counts [C, 4] (one variant of segment_counts), or from an
    estimated event list plus reference_events and audio_names; the event form
    also returns the segment error rate (substitutions S = min(Nfn, Nfp),
    deletions D = max(0, Nfn - Nfp), insertions I = max(0, Nfp - Nfn) per
    segment, ER = (S + D + I) / Nref), which is not separable per class.
    Deviation from the toolbox: F (and P, R) = 0.0 where Ntp = 0."""
    if reference_events is None:
        return _metrics_from_counts(counts_or_events)
    if audio_names is None:
        raise ValueError('audio_names is needed with event lists')
    est = segment_targets(counts_or_events, audio_names, labels, n_segments, time_resolution) != 0
    ref = segment_targets(reference_events, audio_names, labels, n_segments, time_resolution) != 0
    counts = np.stack([(est & ref).sum(axis=(0, 1)), (est & ~ref).sum(axis=(0, 1)),
                       (ref & ~est).sum(axis=(0, 1))], axis=1)
    out = _metrics_from_counts(counts)
    nfp, nfn = (est & ~ref).sum(axis=2), (ref & ~est).sum(axis=2)     # per segment
    nref = int(ref.sum())
    s = int(np.minimum(nfp, nfn).sum())
    d = int(np.maximum(0, nfn - nfp).sum())
    i = int(np.maximum(0, nfp - nfn).sum())
    div = float(nref) if nref else float('nan')
    out['error_rate'] = {'error_rate': (s + d + i) / div, 'substitution_rate': s / div, 'deletion_rate': d / div,
                         'insertion_rate': i / div, 'Nref': nref, 'Nsubs': s, 'Ndel': d, 'Nins': i}
    return out


# ---- optimiser -------------------------------------------------------------

def _as_list(v, C):
    return [float(x) for x in v] if isinstance(v, (list, tuple, np.ndarray)) else [float(v)] * C


def optimize_sed_thresholds(framewise, targets, init=None, learning_rate=1e-2, epochs=70, step=0.02, max_search=5,
                            n_smooth=10, n_salt=10, segment_frames=100):
    """optimize_thresholds.py optimize_sed_thresholds on in-memory outputs.

    framewise [N, T, C] (a HIP tensor runs every epoch as one fused launch),
    targets from segment_targets.  Returns (score, params_dict, record):
    params_dict is the pickle-format dictionary events_from_framewise accepts,
    record[i] = {'thresholds': [3C floats], 'score': F1 before the epoch's
    update}, score the last epoch's.

    The 3C parameters are audio_tagging, high, low thresholds (init 0.5 / 0.3 /
    0.1, :483-486).  Probes accumulate p + step, (p + step) + step, ... in
    float64; cnt is the first probe whose score != the base score (else
    max_search); grad = (new_score - score) / (step cnt); Adam as :120-135
    (eps inside the root, bias-corrected alpha_t).  The audio_tagging entries
    get gradient 0 without any evaluation: the reference's tagging gate is
    commented out (utilities.py:121-122), so no probe can change the score;
    they stay exactly at their initial value.

    Raises RuntimeError where the reference raises IndexError: a bad series
    at the base thresholds or at a probe the reference loop reaches
    (1 .. cnt); probes beyond cnt are speculative and their `bad` is ignored."""
    counter = _Counter(framewise, targets, n_smooth, n_salt, segment_frames)
    C = counter.C
    init = init or {}
    params = (_as_list(init.get('audio_tagging_threshold', 0.5), C) +
              _as_list(init.get('sed_high_threshold', 0.3), C) +
              _as_list(init.get('sed_low_threshold', 0.1), C))
    ms = [np.zeros_like(p) for p in params]
    vs = [np.zeros_like(p) for p in params]
    beta1, beta2, eps = 0.9, 0.999, 1e-8
    record = {}
    score = None
    V = 1 + 2 * max_search
    for it in range(epochs):
        high = np.empty((V, C), np.float64)
        low = np.empty((V, C), np.float64)
        high[:] = params[C:2 * C]
        low[:] = params[2 * C:]
        for c in range(C):
            ph, pl = params[C + c], params[2 * C + c]
            for j in range(1, max_search + 1):
                ph = ph + step
                pl = pl + step
                high[j, c] = ph
                low[max_search + j, c] = pl
        counts = counter(high, low)
        if counts[0, :, 3].any():
            raise RuntimeError('optimize_sed_thresholds: ' + _BAD)
        base = counts[0, :, :3]
        tot = base.sum(axis=0)
        score = _prf(*tot)[2]
        grads = [0.0] * C                            # audio_tagging: inert (gate commented out)
        for first in (1, max_search + 1):            # high probes, then low probes
            for c in range(C):
                cnt, new_score = 0, score
                while cnt < max_search:
                    cnt += 1
                    row = counts[first + cnt - 1, c]
                    if row[3]:
                        raise RuntimeError('optimize_sed_thresholds: ' + _BAD)
                    new_score = _prf(*(tot - base[c] + row[:3]))[2]
                    if new_score != score:
                        break
                grads.append((new_score - score) / (step * cnt) if cnt else 0.0)
        grads = [-g for g in grads]
        alpha_t = learning_rate * np.sqrt(1 - np.power(beta2, it + 1)) / (1 - np.power(beta1, it + 1))
        new_params = []
        for i in range(len(params)):
            ms[i] = beta1 * ms[i] + (1 - beta1) * grads[i]
            vs[i] = beta2 * vs[i] + (1 - beta2) * np.square(grads[i])
            new_params.append(params[i] - alpha_t * ms[i] / (np.sqrt(vs[i] + eps)))
        params = new_params
        record[it] = {'thresholds': [float(p) for p in params], 'score': score}
    flat = [float(p) for p in params]
    params_dict = {'audio_tagging_threshold': flat[:C], 'sed_high_threshold': flat[C:2 * C],
                   'sed_low_threshold': flat[2 * C:],
                   'n_smooth': n_smooth if np.ndim(n_smooth) == 0 else [int(v) for v in n_smooth],
                   'n_salt': n_salt if np.ndim(n_salt) == 0 else [int(v) for v in n_salt]}
    return score, params_dict, record
