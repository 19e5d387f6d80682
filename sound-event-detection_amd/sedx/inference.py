"""Drivers around the model: windowed inference (predict.py), batched clip
inference (main_strong.py inference_prob), gammatone features and event
extraction.  All compute goes through libsedx.

 - predict_windows   pytorch/predict.py:297-349 (driver='predict': stride
                     1 s with --overlap, else sample_duration) and
                     pytorch/main_strong.py:786-835 (driver='main_strong':
                     clip padded to 10 s, stride overlap_value): every window
                     of every clip in ONE native batch, GPU merge at
                     int(100 * overlap_value) frames + the avg_merge divisor
                     schedule (utils/utilities.py:405-446).
 - predict_windows_ragged / predict_files   predict.py's loop over the files
                     of a directory (pytorch/predict.py:264-407): recordings
                     of DIFFERENT lengths, the windows of all of them through
                     the model together, every recording merged and
                     thresholded on its own (bit-identical to one
                     predict_windows call per recording).
 - window_starts / merge_host   the same loop control and merge on the host
                     (no GPU), for checks and host-side callers.
 - predict_windows_vote   inference_prob_vote (pytorch/main_strong.py:1058-1097):
                     binarised windows overlap-added on the GPU.
 - events_from_framewise   frame_prediction_to_event_prediction_v2
                     (pytorch/predict.py:57-121; utils/utilities.py:155-214)
                     over native activity_detection (utils/vad.py): on the
                     GPU for HIP tensors (events.hip), host C++ otherwise.
 - events_from_votes frame_binary_prediction_to_event_prediction
                     (utils/utilities.py:216-276, vad.activity_detection_binary)
                     on the GPU.
 - sweep_overlap     the [overlap, duration] sweeps of inference_prob_overlap /
                     inference_prob_vote (main_strong.py:746, :1011);
                     write_submission (utils/utilities.py:278-291).
 - gamma_features    utils/gammatone/fftweight.py:126-168 + utils/features.py:361-370
                     + utils/utilities.py:73-79, on the GPU.
 - inference_prob    pytorch/pytorch_utils.py:25-78 loop (batches of clips).
"""
import ctypes

import numpy as np
import torch

from . import _lib

FRAMES_PER_SECOND = 100   # utils/config.py:13
LABELS = ['Applause', 'Breathing', 'Chatter', 'Cheering', 'Child_speech_kid_speaking',
          'Clapping', 'Conversation', 'Cough', 'Crowd', 'Crying_sobbing',
          'Female_speech_woman_speaking', 'Laughter', 'Male_speech_man_speaking', 'Run',
          'Screaming', 'Shout', 'Sneeze', 'Walk_footsteps', 'Whispering',
          'Air_horn_truck_horn', 'Car_alarm', 'Emergency_vehicle', 'Explosion',
          'Gunshot_gunfire', 'Siren']   # utils/config.py:31

DEFAULT_PREDICT_PARAMS = {'audio_tagging_threshold': 0.099, 'sed_high_threshold': 0.5,
                          'sed_low_threshold': 0.3, 'n_smooth': 10, 'n_salt': 10}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def window_geometry(model, clip_samples, sample_duration=5, overlap_value=1.0, driver='predict', overlap=True,
                    audio_duration=None, vote=False):
    """(windows per clip, samples per full window, merged frames) of one
    windowed-driver call (sedx_window_geometry); vote=True sizes the vote
    merge (predict_windows_vote), which, unlike avg_merge, accepts a zero
    merge step."""
    nat = model.native(torch.device('cuda', torch.cuda.current_device()))
    spec = _lib.window_spec(sample_duration, overlap_value, driver, overlap, audio_duration, vote=vote)
    nw, ws, nf = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib().sedx_window_geometry(nat.h, int(clip_samples), ctypes.byref(spec), ctypes.byref(nw),
                                               ctypes.byref(ws), ctypes.byref(nf)), nat.h, 'window_geometry')
    return nw.value, ws.value, nf.value


def window_starts(sample_rate, clip_samples, sample_duration=5, overlap_value=1.0, driver='predict', overlap=True,
                  audio_duration=None):
    """The window loop of predict.py:297-338 / main_strong.py:786-832 on the
    host (sedx_window_starts, no GPU): ([sample offset], [samples fed to the
    model]) per window."""
    spec = _lib.window_spec(sample_duration, overlap_value, driver, overlap, audio_duration)
    L = _lib.lib()
    n = ctypes.c_int64()
    _lib.check(L.sedx_window_starts(int(sample_rate), int(clip_samples), ctypes.byref(spec), None, None, 0,
                                    ctypes.byref(n)), None, 'window_starts')
    st = np.zeros(max(n.value, 1), np.int64)
    ln = np.zeros(max(n.value, 1), np.int64)
    _lib.check(L.sedx_window_starts(int(sample_rate), int(clip_samples), ctypes.byref(spec),
                                    st.ctypes.data_as(ctypes.c_void_p), ln.ctypes.data_as(ctypes.c_void_p),
                                    n.value, ctypes.byref(n)), None, 'window_starts')
    return st[:n.value].tolist(), ln[:n.value].tolist()


def merge_host(windows, sample_duration, overlap_value=1.0, avg=True):
    """utilities.merge over the windows in order, then avg_merge (avg=True),
    on the host (sedx_merge_host): windows = list of [T_w, C] (or [1, T_w, C])
    float32 arrays.  Returns [1, N, C] float32, as the reference's merged."""
    ws = [np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1, np.asarray(w).shape[-1])) for w in windows]
    C = ws[0].shape[1]
    frames = np.asarray([w.shape[0] for w in ws], np.int64)
    cat = np.ascontiguousarray(np.concatenate(ws, axis=0)) if len(ws) > 1 else ws[0]
    L = _lib.lib()
    n = ctypes.c_int64()
    st = L.sedx_merge_host(cat.ctypes.data_as(ctypes.c_void_p), frames.ctypes.data_as(ctypes.c_void_p), len(ws), C,
                           int(sample_duration), float(overlap_value), int(bool(avg)), None, 0, ctypes.byref(n))
    if st != _lib.SEDX_OK:
        raise ValueError('sedx_merge_host: the reference raises here (numpy broadcast / zero range step)')
    out = np.zeros((max(n.value, 0), C), np.float32)
    _lib.check(L.sedx_merge_host(cat.ctypes.data_as(ctypes.c_void_p), frames.ctypes.data_as(ctypes.c_void_p),
                                 len(ws), C, int(sample_duration), float(overlap_value), int(bool(avg)),
                                 out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)), None, 'merge_host')
    return out[None]


def _windows(model, audio, spec, vote_thres):
    if model.training:
        raise RuntimeError('call model.eval() first')
    if audio.device.type != 'cuda':
        raise RuntimeError('windowed inference needs a HIP tensor (no CPU fallback)')
    x = audio.to(torch.float32).contiguous()
    if x.dim() == 1:
        x = x[None]
    nat = model.native(x.device)
    L = _lib.lib()
    n_clips, clip_len = x.shape
    nw, wsamp, nf = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.sedx_window_geometry(nat.h, clip_len, ctypes.byref(spec), ctypes.byref(nw), ctypes.byref(wsamp),
                                      ctypes.byref(nf)), nat.h, 'window_geometry')
    wsz = ctypes.c_size_t()
    _lib.check(L.sedx_window_workspace_size(nat.h, n_clips, clip_len, ctypes.byref(spec), ctypes.byref(wsz)),
               nat.h, 'window_workspace_size')
    ws = torch.empty(wsz.value, dtype=torch.uint8, device=x.device)
    merged = torch.empty((n_clips, nf.value, model.classes_num), dtype=torch.float32, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    if vote_thres is None:
        _lib.check(L.sedx_forward_windows(nat.h, _ptr(x), n_clips, clip_len, ctypes.byref(spec), _ptr(merged),
                                          _ptr(ws), wsz.value, stream), nat.h, 'forward_windows')
    else:
        thr = np.ascontiguousarray(_as_list(vote_thres, model.classes_num), dtype=np.float64)
        _lib.check(L.sedx_forward_windows_vote(nat.h, _ptr(x), n_clips, clip_len, ctypes.byref(spec),
                                               thr.ctypes.data_as(ctypes.c_void_p), _ptr(merged),
                                               _ptr(ws), wsz.value, stream), nat.h, 'forward_windows_vote')
    # the merged / voted batch is complete once the stream is: a GRU hand-off
    # that timed out inside this forward (NaN outputs) raises here, not at the
    # next call on the handle (or never)
    torch.cuda.current_stream(x.device).synchronize()
    model.check_error()
    return merged


def predict_windows(model, audio, sample_duration=5, overlap_value=1.0, overlap=True, driver='predict',
                    audio_duration=None):
    """Windowed inference of every clip of audio [n_clips, L] (HIP tensor, every
    clip L samples long) as ONE native batch; returns the merged + averaged
    framewise predictions [n_clips, N, classes].

    driver='predict'      pytorch/predict.py:297-349 with its arguments
                          (--sample_duration, --overlap, --overlap_value;
                          run.sh passes 5 / --overlap / 1): stride 1 s with
                          overlap, else sample_duration s; every window
                          pad_truncate'd; merged at int(100 * overlap_value)
                          frames.
    driver='main_strong'  inference_prob_overlap (main_strong.py:786-835):
                          clip pad_truncate'd to 10 s, stride overlap_value s.
    audio_duration        the loop bound (librosa.get_duration of the file);
                          default L / sample_rate."""
    spec = _lib.window_spec(sample_duration, overlap_value, driver, overlap, audio_duration)
    return _windows(model, audio, spec, None)


def predict_windows_vote(model, audio, sample_duration, overlap_value, bin_threshold, audio_duration=None):
    """inference_prob_vote window loop (pytorch/main_strong.py:1052-1100): every
    window binarised with ``bin_threshold`` (the reference passes
    sed_low_threshold, :1082) and overlap-added without averaging.  Returns
    the vote counts [n_clips, N, classes] (float32, exact integers)."""
    spec = _lib.window_spec(sample_duration, overlap_value, 'main_strong', True, audio_duration, vote=True)
    return _windows(model, audio, spec, bin_threshold)


DEFAULT_WINDOWS_PER_FORWARD = 256   # the ragged driver's chunk (DESIGN.md §4 "Ragged windowed driver")


def _i64(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.int64).reshape(-1))


def _durations(audio_durations, n_clips):
    if audio_durations is None:
        return None, None
    d = np.ascontiguousarray([0.0 if v is None else float(v) for v in audio_durations], dtype=np.float64)
    if d.shape[0] != n_clips:
        raise ValueError('audio_durations: one entry per clip (%d), got %d' % (n_clips, d.shape[0]))
    return d, d.ctypes.data_as(ctypes.c_void_p)


def ragged_window_geometry(model, lengths, sample_duration=5, overlap_value=1.0, overlap=True,
                           audio_durations=None):
    """(windows per clip [n_clips], frame_off [n_clips + 1], samples per window)
    of one predict_windows_ragged call over clips of ``lengths`` samples
    (sedx_ragged_window_geometry): clip c's merged rows are
    frame_off[c] .. frame_off[c + 1].  Raises, naming the clip's index, when
    a clip cannot run (shorter than one window, ...)."""
    nat = model.native(torch.device('cuda', torch.cuda.current_device()))
    spec = _lib.window_spec(sample_duration, overlap_value, 'predict', overlap, None)
    lens = _i64(lengths)
    n = lens.shape[0]
    _, dptr = _durations(audio_durations, n)
    nw = np.zeros(max(n, 1), np.int64)
    foff = np.zeros(n + 1, np.int64)
    wsamp, total = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib().sedx_ragged_window_geometry(
        nat.h, lens.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(spec), dptr,
        nw.ctypes.data_as(ctypes.c_void_p), foff.ctypes.data_as(ctypes.c_void_p), ctypes.byref(wsamp),
        ctypes.byref(total)), nat.h, 'ragged_window_geometry')
    return nw[:n].tolist(), foff.tolist(), wsamp.value


def _ragged_input(clips):
    """(concatenated float32 HIP tensor, lengths) of a list of 1-D HIP tensors or a (concatenated, lengths) pair."""
    if isinstance(clips, tuple) and len(clips) == 2 and isinstance(clips[0], torch.Tensor) and clips[0].dim() == 1 \
            and not isinstance(clips[1], torch.Tensor):
        cat, lengths = clips[0], [int(v) for v in clips[1]]
    else:
        clips = list(clips)
        if not clips:
            raise ValueError('predict_windows_ragged: no clips')
        if any(c.dim() != 1 for c in clips):
            raise ValueError('predict_windows_ragged: every clip is a 1-D tensor')
        lengths = [int(c.shape[0]) for c in clips]
        cat = torch.cat([c.to(torch.float32) for c in clips]) if len(clips) > 1 else clips[0]
    if cat.device.type != 'cuda':
        raise RuntimeError('windowed inference needs a HIP tensor (no CPU fallback)')
    cat = cat.to(torch.float32).contiguous()
    if cat.data_ptr() % 8:
        cat = cat.clone()   # a view at an odd sample of a larger buffer: the frontend's 8-byte loads want the base aligned
    if sum(lengths) != cat.shape[0] or min(lengths) < 0:
        raise ValueError('predict_windows_ragged: the lengths do not add up to the concatenated samples')
    return cat, lengths


def predict_windows_ragged(model, clips, sample_duration=5, overlap_value=1.0, overlap=True, audio_durations=None,
                           max_windows_per_forward=None):
    """predict.py's windowed inference (pytorch/predict.py:297-349) of
    recordings of DIFFERENT lengths in one native call
    (sedx_forward_windows_ragged).  ``clips``: a list of 1-D HIP tensors, or
    (concatenated 1-D HIP tensor, lengths).  The windows of all clips run
    through the model together, at most ``max_windows_per_forward`` per
    forward (None: all at once); every clip is merged and averaged on its
    own.  Returns a list of [N_i, classes] views of one buffer: clip i's
    merged framewise predictions, bit for bit predict_windows(clip i)[0].

    audio_durations   per-clip loop bounds in seconds (librosa.get_duration
                      of each file); default: each clip's length / sample_rate.
    A clip shorter than one window is refused (RuntimeError naming its index)."""
    if model.training:
        raise RuntimeError('call model.eval() first')
    x, lengths = _ragged_input(clips)
    n = len(lengths)
    nat = model.native(x.device)
    L = _lib.lib()
    spec = _lib.window_spec(sample_duration, overlap_value, 'predict', overlap, None)
    lens = _i64(lengths)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    _, dptr = _durations(audio_durations, n)
    foff = np.zeros(n + 1, np.int64)
    lens_p, off_p = lens.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.sedx_ragged_window_geometry(nat.h, lens_p, n, ctypes.byref(spec), dptr, None,
                                             foff.ctypes.data_as(ctypes.c_void_p), None, None),
               nat.h, 'ragged_window_geometry')
    per = int(max_windows_per_forward) if max_windows_per_forward else 0
    wsz = ctypes.c_size_t()
    _lib.check(L.sedx_ragged_window_workspace_size(nat.h, lens_p, n, ctypes.byref(spec), dptr, per,
                                                   ctypes.byref(wsz)), nat.h, 'ragged_window_workspace_size')
    ws = torch.empty(wsz.value, dtype=torch.uint8, device=x.device)
    merged = torch.empty((int(foff[n]), model.classes_num), dtype=torch.float32, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(L.sedx_forward_windows_ragged(nat.h, _ptr(x), off_p, n, ctypes.byref(spec), dptr, per, _ptr(merged),
                                             _ptr(ws), wsz.value, stream), nat.h, 'forward_windows_ragged')
    # as _windows: the batch is complete once the stream is, and a GRU hand-off
    # that timed out inside it raises here
    torch.cuda.current_stream(x.device).synchronize()
    model.check_error()
    return [merged[int(foff[c]):int(foff[c + 1])] for c in range(n)]


def gamma_features(model, audio):
    """audio [B, L] HIP tensor (pad_truncated to 10 s) -> [B, 64, T] model input."""
    if model.feature_type != 'gamma':
        raise ValueError('model was not built with feature_type="gamma"')
    x = audio.to(torch.float32).contiguous()
    nat = model.native(x.device)
    L = _lib.lib()
    B, n = x.shape
    T = ctypes.c_int64()
    _lib.check(L.sedx_gamma_features(nat.h, ctypes.c_void_p(0), B, n, ctypes.c_void_p(0),
                                     ctypes.byref(T), ctypes.c_void_p(0), 0, ctypes.c_void_p(0)),
               nat.h, 'gamma geometry')
    out = torch.empty((B, 64, T.value), dtype=torch.float32, device=x.device)
    wsz = ctypes.c_size_t()
    _lib.check(L.sedx_gamma_workspace_size(nat.h, B, n, ctypes.byref(wsz)), nat.h, 'gamma_workspace_size')
    ws = torch.empty(wsz.value, dtype=torch.uint8, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(L.sedx_gamma_features(nat.h, _ptr(x), B, n, _ptr(out), ctypes.byref(T), _ptr(ws),
                                     ws.numel(), stream), nat.h, 'gamma_features')
    return out


def _as_list(v, C):
    if isinstance(v, (list, tuple, np.ndarray)):
        return list(v)
    return [v] * C


def _event_params(params, C):
    hi_v = params.get('sed_high_threshold', None)
    hi = np.ascontiguousarray(_as_list(hi_v if hi_v is not None else 0.0, C), dtype=np.float64)
    lo_v = params.get('sed_low_threshold', None)
    use_lo = lo_v is not None
    lo = np.ascontiguousarray(_as_list(lo_v if use_lo else 0.0, C), dtype=np.float64)
    ns = np.ascontiguousarray(_as_list(params['n_smooth'], C), dtype=np.int64)
    nsalt = np.ascontiguousarray(_as_list(params['n_salt'], C), dtype=np.int64)
    return hi, lo, use_lo, ns, nsalt


def _ragged_framewise(x):
    """(rows [sum N_i, C] HIP tensor, frame_off) when x is predict_windows_ragged's list of [N_i, C] tensors or
    a (rows, frame_off) pair; else None."""
    if isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], torch.Tensor) and x[0].dim() == 2:
        return x[0], [int(v) for v in x[1]]
    if isinstance(x, list) and x and all(isinstance(v, torch.Tensor) and v.dim() == 2 for v in x):
        foff = np.concatenate([[0], np.cumsum([int(v.shape[0]) for v in x])]).tolist()
        return torch.cat(x), foff   # (one device copy of the rows, a few MB)
    return None


def _event_pairs_ragged(rows, frame_off, params):
    """sedx_events_device_ragged: (clip, class, bgn, fin), frames relative to the clip."""
    if rows.device.type != 'cuda':
        raise RuntimeError('ragged event extraction needs a HIP tensor')
    rows = rows.to(torch.float32).contiguous()
    C = rows.shape[1]
    foff = _i64(frame_off)
    n = foff.shape[0] - 1
    if n < 0 or foff[0] != 0 or foff[-1] != rows.shape[0]:
        raise ValueError('frame_off must run from 0 to the number of rows')
    hi, lo, use_lo, ns, nsalt = _event_params(params, C)
    L = _lib.lib()
    wsz = ctypes.c_size_t()
    foff_p = foff.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.sedx_events_ragged_workspace_size(foff_p, n, C, ctypes.byref(wsz)), None,
               'events_ragged_workspace_size')
    dev = rows.device
    ws = torch.empty(max(wsz.value, 1), dtype=torch.uint8, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cap = max(64, n * C * 4)
    with torch.cuda.device(dev):
        while True:
            ev = torch.empty((cap, 4), dtype=torch.int32, device=dev)
            st = L.sedx_events_device_ragged(_ptr(rows), foff_p, n, C, hi.ctypes.data_as(ctypes.c_void_p),
                                             lo.ctypes.data_as(ctypes.c_void_p), int(use_lo),
                                             ns.ctypes.data_as(ctypes.c_void_p),
                                             nsalt.ctypes.data_as(ctypes.c_void_p), _ptr(ev), cap, _ptr(info),
                                             _ptr(ws), wsz.value, stream)
            _lib.check(st, None, 'events_device_ragged')
            total, bad = (int(v) for v in info.cpu().tolist())
            if bad:
                raise RuntimeError('sedx_events_device_ragged: a run begins at the last frame after the '
                                   'find_bgn_fin_pairs quirk (the reference raises IndexError there)')
            if total <= cap:
                return ev[:total].cpu().numpy()
            cap = total


def event_pairs_device(x, params, mode=0, overlap_value=1, sample_duration=5):
    """Thresholding on the GPU (sedx_events_device): x [N, T, C] HIP tensor of
    framewise probabilities (mode 0, activity_detection) or window vote counts
    (mode 1, activity_detection_binary).  Returns int32 [n_events, 4] =
    (clip, class, bgn, fin) in the reference's (clip, class, time) order.

    x may also be predict_windows_ragged's list of [N_i, C] tensors, or
    (rows [sum N_i, C], frame_off): clips of different lengths, mode 0 only
    (sedx_events_device_ragged), frames relative to each clip."""
    rag = _ragged_framewise(x)
    if rag is not None:
        if mode != 0:
            raise ValueError('clips of different lengths: mode 0 (activity_detection) only')
        return _event_pairs_ragged(rag[0], rag[1], params)
    if x.device.type != 'cuda':
        raise RuntimeError('event_pairs_device needs a HIP tensor')
    x = x.to(torch.float32).contiguous()
    N, T, C = x.shape
    hi, lo, use_lo, ns, nsalt = _event_params(params, C)
    L = _lib.lib()
    wsz = ctypes.c_size_t()
    _lib.check(L.sedx_events_workspace_size(N, T, C, ctypes.byref(wsz)), None, 'events_workspace_size')
    dev = x.device
    ws = torch.empty(max(wsz.value, 1), dtype=torch.uint8, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cap = max(64, N * C * 4)
    with torch.cuda.device(dev):
        while True:
            ev = torch.empty((cap, 4), dtype=torch.int32, device=dev)
            st = L.sedx_events_device(_ptr(x), N, T, C, hi.ctypes.data_as(ctypes.c_void_p),
                                      lo.ctypes.data_as(ctypes.c_void_p), int(use_lo),
                                      ns.ctypes.data_as(ctypes.c_void_p),
                                      nsalt.ctypes.data_as(ctypes.c_void_p), int(mode),
                                      float(overlap_value), int(sample_duration), _ptr(ev), cap,
                                      _ptr(info), _ptr(ws), wsz.value, stream)
            _lib.check(st, None, 'events_device')
            n, bad = (int(v) for v in info.cpu().tolist())
            if bad:
                raise RuntimeError('sedx_events_device: a run begins at the last frame after the '
                                   'find_bgn_fin_pairs quirk (the reference raises IndexError there)')
            if n <= cap:
                return ev[:n].cpu().numpy()
            cap = n


def event_pairs(framewise, params):
    """activity_detection over every (clip, class): on the GPU for a HIP tensor
    (sedx_events_device), else the host C++ path (sedx_events).  framewise
    [N, T, C], or clips of different lengths as event_pairs_device takes them
    (HIP tensors only).  Returns int32 array [n_events, 4] = (clip, class, bgn, fin)."""
    if (isinstance(framewise, torch.Tensor) and framewise.device.type == 'cuda') or \
            _ragged_framewise(framewise) is not None:
        return event_pairs_device(framewise, params, mode=0)
    fw = framewise.detach().cpu().numpy() if isinstance(framewise, torch.Tensor) else np.asarray(framewise)
    fw = np.ascontiguousarray(fw, dtype=np.float32)
    N, T, C = fw.shape
    hi, lo, use_lo, ns, nsalt = _event_params(params, C)
    L = _lib.lib()
    n = ctypes.c_int64()
    cap = max(16, N * C * 4)
    while True:
        ev = np.zeros((cap, 4), dtype=np.int32)
        st = L.sedx_events(fw.ctypes.data_as(ctypes.c_void_p), N, T, C,
                           hi.ctypes.data_as(ctypes.c_void_p), lo.ctypes.data_as(ctypes.c_void_p),
                           int(use_lo), ns.ctypes.data_as(ctypes.c_void_p),
                           nsalt.ctypes.data_as(ctypes.c_void_p), ev.ctypes.data_as(ctypes.c_void_p),
                           cap, ctypes.byref(n))
        if st == _lib.SEDX_OK:
            return ev[:n.value]
        if n.value > cap:
            cap = n.value
            continue
        raise RuntimeError('sedx_events failed: a run begins at the last frame after the '
                           'find_bgn_fin_pairs quirk (the reference raises IndexError there)')


def _to_events(pairs, audio_name, frames_per_second, labels, sort):
    names = audio_name if isinstance(audio_name, (list, tuple)) else None
    out = []
    for clip, k, b, f in pairs.tolist():
        out.append({'filename': names[clip] if names else audio_name,
                    'onset': b / float(frames_per_second), 'offset': f / float(frames_per_second),
                    'event_label': labels[k]})
    if sort:
        out = sorted(out, key=lambda e: e['onset'])
    return out


def events_from_framewise(framewise, params, audio_name='test', frames_per_second=FRAMES_PER_SECOND,
                          labels=LABELS, sort=True):
    """List of {'filename','onset','offset','event_label'} exactly like
    frame_prediction_to_event_prediction_v2 (+ the stable onset sort of
    predict.py:353; main_strong.py:834 does not sort: sort=False).  For clips
    of different lengths (predict_windows_ragged's list, or (rows,
    frame_off)) ``audio_name`` is a list with one name per clip."""
    return _to_events(event_pairs(framewise, params), audio_name, frames_per_second, labels, sort)


def events_from_votes(votes, overlap_value, sample_duration, params, audio_name='test',
                      frames_per_second=FRAMES_PER_SECOND, labels=LABELS):
    """frame_binary_prediction_to_event_prediction (utils/utilities.py:216-276)
    on vote counts from predict_windows_vote, on the GPU."""
    pairs = event_pairs_device(votes, params, mode=1, overlap_value=overlap_value,
                               sample_duration=sample_duration)
    return _to_events(pairs, audio_name, frames_per_second, labels, False)


def write_submission(event_list, submission_path):
    """utils/utilities.py:278-291: one tab-separated line per event."""
    with open(submission_path, 'w') as f:
        for e in event_list:
            f.write('{}\t{}\t{}\t{}\n'.format(e['filename'], e['onset'], e['offset'], e['event_label']))


OVERLAP_SWEEP = [[0.5, 6], [0.5, 7], [1, 5], [1, 6], [1, 7]]   # main_strong.py:746, :1011


def sweep_overlap(model, audio, audio_names, params, combos=OVERLAP_SWEEP, vote=False):
    """inference_prob_overlap / inference_prob_vote parameter sweep
    (pytorch/main_strong.py:762-835, :1028-1100): for every [overlap_value,
    sample_duration] the clips (padded to 10 s) run as one windowed batch, then
    events on the GPU.  audio [n_clips, L] HIP tensor.  Returns
    {(overlap_value, sample_duration): event list} in the reference's order."""
    out = {}
    for ov, sd in combos:
        if vote:
            votes = predict_windows_vote(model, audio, sd, ov, params['sed_low_threshold'])
            out[(ov, sd)] = events_from_votes(votes, ov, sd, params, list(audio_names))
        else:
            merged = predict_windows(model, audio, sd, ov, driver='main_strong')
            out[(ov, sd)] = events_from_framewise(merged, params, list(audio_names), sort=False)
    return out


class GraphedForward:
    """The model's forward for one fixed input shape captured once in a HIP
    graph (torch.cuda.graph around the libsedx launches) and replayed: the
    same kernels, launched as one graph instead of ~17 host launches, so the
    gaps between them shrink (one 10 s clip: 0.63 -> 0.56 ms p50).  Outputs
    are the eager forward's, bit for bit.  Calls must use the captured shape;
    the returned dict aliases the graph's static outputs (copy them to keep
    them past the next call).

        g = GraphedForward(model, example_wave)   # [B, L] on the device
        out = g(wave)                             # same shape as example_wave
    """

    def __init__(self, model, example, warmup=3):
        import torch
        if getattr(model, 'pipelined', False):
            # a pipelined handle makes every forward wait on the previous
            # forward's conv-done event, recorded outside any capture: that
            # wait cannot be captured (and would leave the event half recorded)
            raise RuntimeError('GraphedForward needs model.set_pipelined(False)')
        self.model = model
        self.static_in = example.detach().clone()
        self.stream = torch.cuda.Stream(example.device)
        # the warm-up forwards on the side stream read static_in, whose clone
        # was queued on the current stream
        self.stream.wait_stream(torch.cuda.current_stream(example.device))
        with torch.no_grad(), torch.cuda.stream(self.stream):
            for _ in range(warmup):          # first launches set up per-device launch facts
                model(self.static_in)
            self.stream.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self.static_out = model(self.static_in)

    def __call__(self, wave):
        if tuple(wave.shape) != tuple(self.static_in.shape):
            raise ValueError('GraphedForward captured shape %s, got %s'
                             % (tuple(self.static_in.shape), tuple(wave.shape)))
        self.static_in.copy_(wave)
        self.graph.replay()
        return self.static_out


def inference_prob(model, waveforms, batch_size=32, device=None):
    """pytorch_utils.forward (pytorch/pytorch_utils.py:25-78): batched clip
    inference; returns numpy {'clipwise_output', 'framewise_output'}.  On a
    gamma model a 2-D batch is waveforms (model.forward_audio), a 3-D one the
    precomputed features the reference's loader hands its model."""
    device = device or torch.device('cuda', torch.cuda.current_device())
    outs = {'clipwise_output': [], 'framewise_output': []}
    with torch.no_grad():
        for i in range(0, len(waveforms), batch_size):
            x = torch.as_tensor(waveforms[i:i + batch_size], dtype=torch.float32).to(device)
            o = model.forward_audio(x) if getattr(model, 'feature_type', None) == 'gamma' and x.dim() == 2 else model(x)
            outs['clipwise_output'].append(o['clipwise_output'].cpu().numpy())
            outs['framewise_output'].append(o['framewise_output'].cpu().numpy())
            model.check_error()     # the batch is complete: an asynchronous failure surfaces here
    return {k: np.concatenate(v, axis=0) for k, v in outs.items()}


def predict_files(model, paths, params=DEFAULT_PREDICT_PARAMS, sample_duration=5, overlap=True, overlap_value=1.0,
                  out_dir=None, max_windows_per_forward=DEFAULT_WINDOWS_PER_FORWARD):
    """predict.py's directory loop (pytorch/predict.py:264-407) over WAV files
    of any duration: every file is loaded with ``audio.load(path,
    sr=model.sample_rate)``, the windows of ALL files run through the model in
    one predict_windows_ragged call (loop bounds from the decoded lengths), one
    ragged events call thresholds them, and with ``out_dir`` one
    ``<name>.xml`` per file is written through write_xml (:406).

    Returns {path: event list, sorted by onset as predict.py:353} (a
    PredictedFiles dict); its ``skipped`` attribute lists the files that
    yield no complete window.  Deviation from the reference: such files (fewer
    samples than one window of sample_duration s, an empty or unreadable
    file) are reported in ``skipped`` and do not abort the batch.  The
    reference raises on an empty file and stops; a file shorter than one
    window it runs as a single zero-padded window, which the ragged driver
    refuses: run such a file through predict_windows on its own."""
    import os
    from . import audio
    dev = next(model.parameters()).device
    sr = model.sample_rate
    need = int(sample_duration) * sr
    out = PredictedFiles()
    kept, clips = [], []
    for p in paths:
        try:
            y, _ = audio.load(p, sr=sr, device=dev)
        except RuntimeError:
            y = None   # not a WAV file the loader reads
        if y is None or y.shape[0] < need:
            out.skipped.append(p)
            continue
        kept.append(p)
        clips.append(y)
    if not kept:
        return out
    with torch.no_grad():
        merged = predict_windows_ragged(model, clips, sample_duration, overlap_value, overlap, None,
                                        max_windows_per_forward)
    pairs = event_pairs_device(merged, params, mode=0)
    per_clip = [[] for _ in kept]
    for row in pairs.tolist():
        per_clip[row[0]].append(row)
    stride = 1 if overlap else int(sample_duration)
    n_windows = ragged_window_geometry(model, [int(y.shape[0]) for y in clips], sample_duration, overlap_value,
                                       overlap)[0]
    for c, p in enumerate(kept):
        ev = _to_events(np.asarray(per_clip[c], dtype=np.int64).reshape(-1, 4), [p] * len(kept), FRAMES_PER_SECOND,
                        LABELS, True)
        out[p] = ev
        if out_dir is not None:
            # the loop's start after the last window and predict.py:355-358's end (the "Others" segment)
            duration = clips[c].shape[0] / float(sr)
            start = n_windows[c] * stride
            end = duration if duration < start + sample_duration else start + sample_duration
            name = p.split('/')[-1].split('.wav')[0]
            with open(os.path.join(out_dir, name + '.xml'), 'w') as f:
                f.write(write_xml(p, ev, start, end))
    return out


class PredictedFiles(dict):
    """predict_files' result: {path: events}; ``skipped``: the files that yield no window."""

    def __init__(self):
        super().__init__()
        self.skipped = []


def write_xml(audio_name, events, start=0, end=0):
    """XML document of pytorch/predict.py:264-407 (SoundCaptionList); the
    document is named after the file, not its path (predict.py:267)."""
    s = ['<AudioDoc name="{}">\n'.format(audio_name.split('/')[-1]), '\t<SoundCaptionList>\n']
    if events:
        for e in events:
            s.append('\t\t<SoundSegment stime="{}" dur="{}" event="{}">{}</SoundSegment>\n'.format(
                e['onset'], e['offset'] - e['onset'], e['event_label'], e['event_label']))
    else:
        s.append('\t\t<SoundSegment stime="{}" dur="{}">Others</SoundSegment>\n'.format(start, end - start))
    s.append('\t</SoundCaptionList>\n')
    s.append('</AudioDoc>')
    return ''.join(s)
