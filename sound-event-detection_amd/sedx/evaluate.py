"""The reference's Evaluator (pytorch/evaluate.py:11-95) with the ranking on
the GPU: clipwise and framewise average precision, events, the submission
file and the segment metrics of one pass over a set of clips.

``sklearn.metrics.average_precision_score`` is one argsort per class on the
host; here the framewise tensor stays on the device and every class is ranked
by a segmented radix sort (csrc/rank.hip, ``sedx_average_precision_device``).
A numpy input takes the host entry (csrc/rank_host.cpp), which computes the
same bits.  The definition (include/sedx.h): non-interpolated AP over the
distinct float32 thresholds, the terms summed in float64 in one fixed order;
a class without positives has AP = NaN (the reference's environment divides
0 / 0 there and takes ``np.nanmean``; recent sklearn returns 0.0 with a
warning), a non-finite score raises ValueError as sklearn does.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .calibrate import _load_reference_csv, segment_metrics
from .inference import FRAMES_PER_SECOND, LABELS, _ptr, events_from_framewise, write_submission

# evaluate.py:45-50
SED_PARAMS = {'audio_tagging_threshold': 0.5, 'sed_high_threshold': 0.5, 'sed_low_threshold': 0.2,
              'n_smooth': 10, 'n_salt': 10}

_workspaces = {}     # device -> cached uint8 workspace tensor


def _c(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _message():
    return _lib.lib().sedx_last_error(None).decode()


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.device.type == 'cuda'


def _two_d(target, scores):
    """([M, C] target, [M, C] scores) views of [M, C] or [N, T, C] inputs."""
    if tuple(target.shape) != tuple(scores.shape):
        raise ValueError('target %s and scores %s differ in shape' % (tuple(target.shape), tuple(scores.shape)))
    if len(scores.shape) not in (2, 3):
        raise ValueError('[M, C] or [N, T, C] expected, got %s' % (tuple(scores.shape),))
    C = int(scores.shape[-1])
    return target.reshape(-1, C), scores.reshape(-1, C)


def _host(target, scores, curve, check):
    s = np.ascontiguousarray(scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else scores,
                             dtype=np.float32)
    t = target.detach().cpu().numpy() if isinstance(target, torch.Tensor) else np.asarray(target)
    t = np.ascontiguousarray(t != 0, dtype=np.uint8)
    M, C = s.shape
    ap = np.empty(C, np.float64)
    info = np.zeros((C, 3), np.int64)
    thr = np.zeros((C, M), np.float32) if curve else None
    tp = np.zeros((C, M), np.int32) if curve else None
    n = np.zeros((C, M), np.int32) if curve else None
    st = _lib.lib().sedx_average_precision(_c(s), _c(t), M, C, _c(ap), _c(info),
                                           _c(thr) if curve else None, _c(tp) if curve else None,
                                           _c(n) if curve else None)
    if st != _lib.SEDX_OK and (check or not info[:, 2].any()):
        raise ValueError(_message())
    return ap, info, thr, tp, n


def _device(target, scores, curve, check):
    dev = scores.device
    s = scores.detach().to(torch.float32).contiguous()
    t = torch.as_tensor(target, device=dev) if not isinstance(target, torch.Tensor) else target.to(dev)
    t = (t != 0).to(torch.uint8).contiguous()
    M, C = (int(d) for d in s.shape)
    L = _lib.lib()
    wsz = ctypes.c_size_t()
    if L.sedx_average_precision_workspace_size(M, C, ctypes.byref(wsz)) != _lib.SEDX_OK:
        raise ValueError(_message())
    ws = _workspaces.get(dev)
    if ws is None or ws.numel() < wsz.value:
        ws = _workspaces[dev] = torch.empty(max(wsz.value, 1), dtype=torch.uint8, device=dev)
    # ap and info share one buffer: one read-back
    out = torch.empty(4 * C, dtype=torch.int64, device=dev)
    thr = torch.zeros((C, M), dtype=torch.float32, device=dev) if curve else None
    tp = torch.zeros((C, M), dtype=torch.int32, device=dev) if curve else None
    n = torch.zeros((C, M), dtype=torch.int32, device=dev) if curve else None
    null = ctypes.c_void_p(0)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        st = L.sedx_average_precision_device(_ptr(s), _ptr(t), M, C, _ptr(out), _ptr(out[C:]),
                                             _ptr(thr) if curve else null, _ptr(tp) if curve else null,
                                             _ptr(n) if curve else null, _ptr(ws), ws.numel(), stream)
        if st == 1:
            raise ValueError(_message())
        _lib.check(st, None, 'average_precision_device')
        host = out.cpu().numpy()
    ap = host[:C].view(np.float64).copy()
    info = host[C:].reshape(C, 3).copy()
    if check and info[:, 2].any():
        bad = np.flatnonzero(info[:, 2])
        raise ValueError('average precision: %d non-finite score(s), the first in class %d'
                         % (int(info[:, 2].sum()), int(bad[0])))
    if curve:
        thr, tp, n = thr.cpu().numpy(), tp.cpu().numpy(), n.cpu().numpy()
    return ap, info, thr, tp, n


def rank(target, scores, curve=False, check=True):
    """The raw outputs of the entry points for [M, C] or [N, T, C] inputs:
    (ap float64 [C], info int64 [C, 3] = (P, K, non-finite count), thr, tp, n)
    with the curve arrays [C, M] (first K of a row valid) or None.
    check=False returns instead of raising ValueError on non-finite scores."""
    target, scores = _two_d(target, scores)
    return (_device if _is_device(scores) else _host)(target, scores, curve, check)


def ranked_counts(target, scores):
    """The precision-recall curve in integers, per class: a list of
    (thresholds float32 [K] descending, tp int64 [K], n int64 [K]) with
    tp[k] positives among the n[k] samples scoring >= thresholds[k]
    (precision tp / n, recall tp / tp[-1])."""
    _, info, thr, tp, n = rank(target, scores, True)
    return [(thr[c, :K].copy(), tp[c, :K].astype(np.int64), n[c, :K].astype(np.int64))
            for c, K in enumerate(info[:, 1].tolist())]


def average_precision(target, scores, average=None):
    """sklearn.metrics.average_precision_score(target, scores, average) for
    [M, C] or [N, T, C] inputs.  numpy inputs run on the host, a HIP tensor of
    scores on the device (current stream, cached workspace, one read-back).
    average=None: float64 [C]; 'macro': their mean (NaN propagates, as
    np.average inside sklearn); 'micro': one class of all M C samples.  A
    class without positives is NaN; a non-finite score raises ValueError."""
    if average not in (None, 'macro', 'micro'):
        raise ValueError("average must be None, 'macro' or 'micro'")
    if average == 'micro':
        target, scores = _two_d(target, scores)
        return float(rank(target.reshape(-1, 1), scores.reshape(-1, 1), False)[0][0])
    ap = rank(target, scores, False)[0]
    return float(np.average(ap)) if average == 'macro' else ap


def sed_average_precision(strong_target, framewise_output, average):
    """evaluate.py:11-29: framewise AP over (N, frames_num, classes_num)."""
    if len(strong_target.shape) != 3 or tuple(strong_target.shape) != tuple(framewise_output.shape):
        raise ValueError('strong_target %s and framewise_output %s must be equal (N, frames_num, classes_num)'
                         % (tuple(strong_target.shape), tuple(framewise_output.shape)))
    return average_precision(strong_target, framewise_output, average)


def _events(reference_events):
    return _load_reference_csv(reference_events) if isinstance(reference_events, str) else reference_events


def strong_targets(reference_events, audio_names, frames_num=1000, frames_per_second=FRAMES_PER_SECOND,
                   labels=LABELS):
    """uint8 [N, frames_num, C] as utils/features.py:143-176 builds it: an event
    sets frames [int(round(onset * fps)), int(round(offset * fps)) + 1), with
    Python's round-half-even on the float product and the slice clipped at
    frames_num by slicing.  reference_events: a ground-truth CSV path or an
    event list (calibrate.segment_targets); unknown files / labels are
    ignored, a clip without events stays zero."""
    clip = {name: i for i, name in enumerate(audio_names)}
    cls = {name: i for i, name in enumerate(labels)}
    out = np.zeros((len(audio_names), int(frames_num), len(labels)), np.uint8)
    for e in _events(reference_events):
        i, k = clip.get(e['filename']), cls.get(e['event_label'])
        if i is None or k is None:
            continue
        bgn = int(round(float(e['onset']) * frames_per_second))
        end = int(round(float(e['offset']) * frames_per_second)) + 1
        out[i, bgn:end, k] = 1
    return out


def weak_targets(reference_events, audio_names, labels=LABELS):
    """uint8 [N, C]: the class has any event in the clip (utils/features.py:124-140)."""
    clip = {name: i for i, name in enumerate(audio_names)}
    cls = {name: i for i, name in enumerate(labels)}
    out = np.zeros((len(audio_names), len(labels)), np.uint8)
    for e in _events(reference_events):
        i, k = clip.get(e['filename']), cls.get(e['event_label'])
        if i is not None and k is not None:
            out[i, k] = 1
    return out


class Evaluator(object):
    """evaluate.py:32-95.  ``model`` is a sedx.models model on a HIP device."""

    def __init__(self, model, labels=LABELS):
        self.model = model
        self.labels = labels
        self.sed_params_dict = dict(SED_PARAMS)

    def forward(self, batches):
        """pytorch_utils.forward (:25-78, return_target=True) with the outputs
        and targets concatenated on the device."""
        device = next(self.model.parameters()).device
        acc = {}
        self.model.eval()
        with torch.no_grad():
            for batch in batches:
                out = self.model(torch.as_tensor(batch['waveform'], dtype=torch.float32).to(device))
                acc.setdefault('audio_name', []).append(np.asarray(batch['audio_name']))
                acc.setdefault('clipwise_output', []).append(out['clipwise_output'])
                if 'framewise_output' in out:
                    acc.setdefault('framewise_output', []).append(out['framewise_output'])
                for key in ('target', 'strong_target'):
                    if key in batch:
                        acc.setdefault(key, []).append(torch.as_tensor(np.asarray(batch[key]) != 0).to(device))
        if not acc:
            raise ValueError('no batches')
        torch.cuda.current_stream(device).synchronize()
        self.model.check_error()      # every batch is complete: an asynchronous failure surfaces here
        return {k: (np.concatenate(v, axis=0) if k == 'audio_name' else torch.cat(v, dim=0)) for k, v in acc.items()}

    def evaluate(self, batches, reference_csv_path, submission_path, frames_per_second=FRAMES_PER_SECOND):
        """(statistics, output_dict) of evaluate.py:52-95.  batches: an iterable
        of {'audio_name', 'waveform', optionally 'target' and 'strong_target'}.
        statistics: 'clipwise_ap' (against 'target'; without one, against
        weak_targets of reference_csv_path), 'framewise_ap' when the batches
        carry 'strong_target' (as the reference), 'sed_metrics' =
        calibrate.segment_metrics of the events written to submission_path.
        output_dict: numpy arrays under the reference's keys."""
        dev = self.forward(batches)
        names = [str(n) for n in dev['audio_name'].tolist()]
        statistics = {}
        target = dev.get('target')
        if target is None:
            target = weak_targets(reference_csv_path, names, self.labels)
        statistics['clipwise_ap'] = average_precision(target, dev['clipwise_output'], average=None)
        if 'strong_target' in dev:
            statistics['framewise_ap'] = sed_average_precision(dev['strong_target'], dev['framewise_output'],
                                                               average=None)
        events = events_from_framewise(dev['framewise_output'], self.sed_params_dict, names, frames_per_second,
                                       self.labels, sort=False)
        write_submission(events, submission_path)
        statistics['sed_metrics'] = segment_metrics(events, reference_csv_path, names, self.labels)
        output_dict = {k: (v if k == 'audio_name' else v.cpu().numpy()) for k, v in dev.items()}
        return statistics, output_dict
