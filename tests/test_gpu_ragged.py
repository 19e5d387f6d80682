"""The ragged windowed driver on the GPU: recordings of different lengths in one
predict_windows_ragged call against predict_windows on every clip alone, bit
for bit (the frontend's item table at odd sample offsets, chunked forwards, the
zero fill at a clip's end, the per-clip merge), the ragged events kernel against
the per-clip device and host paths, predict_files over WAV files, and a GRU
hand-off time-out surfacing from the call itself.  Seeded synthetic weights."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import audio_oracle as A
from sedx import synth

pytestmark = pytest.mark.gpu

GRU, TRF = 'Cnn_9layers_Gru_FrameAtt', 'Cnn_9layers_Transformer_FrameAtt'
SEEDS = {GRU: 0, TRF: 1}
P16 = (16000, 512, 160, 64, 25, 7000)
P32 = (32000, 1024, 320, 64, 50, 14000)
# back to back: clips 1 and 2 start at odd sample offsets (81,237 and 161,237)
LENGTHS = {'16k': [81237, 80000, 112001, 163333], '32k': [170001, 160000]}
FRAMES = {GRU: 500, TRF: 496}          # a 5 s window's framewise rows

_models, _cases = {}, {}


def build(mt, preset='16k', precision=None):
    """One model per (type, preset, precision), shared by the tests of this module."""
    key = (mt, preset, precision)
    if key not in _models:
        from sedx import models
        m = getattr(models, mt)(*(P16 if preset == '16k' else P32), 25, 'logmel')
        sd = m.state_dict()
        for k, v in synth.make_state_dict(mt, seed=SEEDS[mt]).items():
            sd[k] = torch.from_numpy(v)
        m.load_state_dict(sd, strict=True)
        m = m.to('cuda').eval()
        _models[key] = m.set_precision(precision) if precision else m
    return _models[key]


def clips_of(preset, seed=77):
    lengths = LENGTHS[preset]
    sr = 16000 if preset == '16k' else 32000
    cat = synth.make_waveforms(1, seconds=sum(lengths) / float(sr), sample_rate=sr, seed=seed)[0]
    assert cat.shape[0] == sum(lengths)
    return torch.from_numpy(cat).cuda(), lengths


def case(mt, preset, precision):
    """(model, concatenated audio, lengths, every clip alone through predict_windows), computed once."""
    key = (mt, preset, precision)
    if key not in _cases:
        from sedx import inference
        m = build(mt, preset, precision)
        cat, lengths = clips_of(preset)
        off = np.concatenate([[0], np.cumsum(lengths)])
        with torch.no_grad():
            # .clone(): each file in its own allocation, as predict_files' per-file counterpart would hold it
            alone = [inference.predict_windows(m, cat[off[c]:off[c + 1]].clone()[None], 5, 1.0)[0].cpu().numpy()
                     for c in range(len(lengths))]
        _cases[key] = (m, cat, lengths, alone)
    return _cases[key]


CASES = [(GRU, '16k', None), (TRF, '16k', None), (GRU, '16k', 'exact'), (TRF, '16k', 'exact'), (GRU, '32k', None)]
CASE_IDS = ['gru', 'trf', 'gru-exact', 'trf-exact', 'gru-32k']


@pytest.mark.parametrize('mt,preset,precision', CASES, ids=CASE_IDS)
def test_per_file_identity(mt, preset, precision):
    from sedx import inference
    m, cat, lengths, alone = case(mt, preset, precision)
    with torch.no_grad():
        got = inference.predict_windows_ragged(m, (cat, lengths))
    nw, foff, wsamp = inference.ragged_window_geometry(m, lengths)
    assert wsamp == 5 * m.sample_rate and len(got) == len(lengths)
    if preset == '16k':
        assert nw == [1, 1, 3, 6]
    for c, g in enumerate(got):
        g = g.cpu().numpy()
        assert g.shape == alone[c].shape == (foff[c + 1] - foff[c], 25) and np.isfinite(g).all()
        assert g.shape[0] == FRAMES[mt] + 100 * (nw[c] - 1)
        assert np.array_equal(g, alone[c]), (c, float(np.max(np.abs(g - alone[c]))))
    # the views share one buffer, clip after clip
    assert all(got[c + 1].data_ptr() == got[c].data_ptr() + got[c].numel() * 4 for c in range(len(got) - 1))
    # a list of separate 1-D tensors is the same call
    off = np.concatenate([[0], np.cumsum(lengths)])
    with torch.no_grad():
        again = inference.predict_windows_ragged(m, [cat[off[c]:off[c + 1]] for c in range(len(lengths))])
    assert all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize('mt', [GRU, TRF], ids=['gru', 'trf'])
def test_chunked_forwards_give_identical_bits(mt):
    """11 windows in forwards of 1, of 4 (4 + 4 + 3: the item table's offset, a smaller last forward) and all at
    once."""
    from sedx import inference
    m, cat, lengths, alone = case(mt, '16k', None)
    with torch.no_grad():
        outs = [torch.cat(inference.predict_windows_ragged(m, (cat, lengths), max_windows_per_forward=k)).cpu().numpy()
                for k in (1, 4, None)]
    ref = np.concatenate(alone)
    for k, o in zip((1, 4, None), outs):
        assert np.array_equal(o, ref), k


@pytest.mark.parametrize('last', [False, True], ids=['before-loud-clip', 'last-in-buffer'])
def test_zero_fill_at_a_clips_end(last):
    """A loop bound 0.3 s past clip 0's samples: its second window's last 4,799 samples are pad_truncate's zeros,
    not the next clip's audio (+-1.0 there), and, with the clip last in an exactly allocated buffer, not a read
    past the allocation."""
    from sedx import inference
    m = build(GRU)
    short = torch.from_numpy(synth.make_waveforms(1, seconds=91201 / 16000., sample_rate=16000, seed=5)[0]).cuda()
    loud = torch.from_numpy(synth.make_waveforms(1, seconds=80000 / 16000., sample_rate=16000, seed=6)[0]).cuda()
    loud[:8000] = torch.where(torch.arange(8000, device='cuda') % 2 == 0, 1.0, -1.0)
    assert short.shape[0] == 91201
    with torch.no_grad():
        ref = inference.predict_windows(m, short.clone()[None], 5, 1.0, audio_duration=6.0)[0]
        ref_loud = inference.predict_windows(m, loud.clone()[None], 5, 1.0)[0]
        assert ref.shape[0] == 600                                  # two windows
        clips, dur = ([loud, short], [0.0, 6.0]) if last else ([short, loud], [6.0, 0.0])
        cat = torch.empty(91201 + 80000, dtype=torch.float32, device='cuda')     # exactly the samples
        torch.cat(clips, out=cat)
        got = inference.predict_windows_ragged(m, (cat, [c.shape[0] for c in clips]), audio_durations=dur)
    i = 1 if last else 0
    assert torch.equal(got[i], ref), float((got[i] - ref).abs().max())
    assert torch.equal(got[1 - i], ref_loud)
    # without the bound the clip has one window
    with torch.no_grad():
        assert inference.predict_windows_ragged(m, (cat, [c.shape[0] for c in clips]))[i].shape[0] == 500


def _series(rng, T, C=25):
    """A smooth random walk per class; quiet at the end, so that no run begins at the last frame (where the
    reference raises IndexError and every path here reports it)."""
    x = rng.uniform(0, 1, (T, C)).astype(np.float32)
    x = (np.cumsum(x - 0.5, axis=0) / 8 + 0.5).astype(np.float32)
    x[-2:] = 0.0
    return x


EVENT_PARAMS = {'sed_high_threshold': 0.55, 'sed_low_threshold': 0.35, 'n_smooth': 4, 'n_salt': 3}


def test_ragged_events_equal_every_clip_alone():
    """Clips of 500 .. 1000 rows, of 37 rows, of one row: the ragged kernel's quadruples against the device kernel
    and the host C++ on every clip alone, and the event dicts against events_from_framewise per clip."""
    from sedx import inference
    rng = np.random.default_rng(11)
    lens = [500, 496, 700, 1000, 37, 1, 130, 64, 65]
    clips = [_series(rng, T) for T in lens]
    rows = torch.from_numpy(np.concatenate(clips)).cuda()
    foff = np.concatenate([[0], np.cumsum(lens)]).tolist()
    got = inference.event_pairs_device((rows, foff), EVENT_PARAMS)
    views = [rows[foff[c]:foff[c + 1]] for c in range(len(lens))]
    assert np.array_equal(inference.event_pairs_device(views, EVENT_PARAMS), got)
    want_dev, want_host = [], []
    for c, x in enumerate(clips):
        d = inference.event_pairs_device(torch.from_numpy(x).cuda()[None], EVENT_PARAMS)
        h = inference.event_pairs(x[None], EVENT_PARAMS)
        for w, p in ((want_dev, d), (want_host, h)):
            p = p.copy()
            p[:, 0] = c
            w.append(p)
    want_dev, want_host = np.concatenate(want_dev), np.concatenate(want_host)
    assert len(got) > 100 and len(set(got[:, 0].tolist())) >= 6           # events in most clips
    assert np.array_equal(got, want_host)
    assert np.array_equal(got, want_dev)
    names = ['clip%d.wav' % c for c in range(len(lens))]
    ev = inference.events_from_framewise(views, EVENT_PARAMS, audio_name=names, sort=False)
    per_clip = []
    for c, x in enumerate(clips):
        per_clip += inference.events_from_framewise(torch.from_numpy(x).cuda()[None], EVENT_PARAMS, audio_name=names[c],
                                                    sort=False)
    assert ev == per_clip
    with pytest.raises(ValueError):
        inference.event_pairs_device((rows, foff), EVENT_PARAMS, mode=1)


def test_ragged_events_capacity_smaller_than_the_count():
    from sedx import _lib, inference
    rng = np.random.default_rng(12)
    lens = [300, 1000, 77]
    rows = torch.from_numpy(np.concatenate([_series(rng, T) for T in lens])).cuda()
    foff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    full = inference.event_pairs_device((rows, foff.tolist()), EVENT_PARAMS)
    assert len(full) > 8
    L = _lib.lib()
    hi, lo, use_lo, ns, nsalt = inference._event_params(EVENT_PARAMS, 25)
    wsz = ctypes.c_size_t()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.sedx_events_ragged_workspace_size(p(foff), 3, 25, ctypes.byref(wsz)) == 0
    ws = torch.empty(wsz.value, dtype=torch.uint8, device='cuda')
    info = torch.full((2,), -1, dtype=torch.int64, device='cuda')
    cap = 5
    ev = torch.full((cap + 3, 4), -7, dtype=torch.int32, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    st = L.sedx_events_device_ragged(ctypes.c_void_p(rows.data_ptr()), p(foff), 3, 25, p(hi), p(lo), int(use_lo), p(ns),
                                     p(nsalt), ctypes.c_void_p(ev.data_ptr()), cap, ctypes.c_void_p(info.data_ptr()),
                                     ctypes.c_void_p(ws.data_ptr()), wsz.value, stream)
    assert st == 0
    torch.cuda.synchronize()
    assert info.tolist() == [len(full), 0]                          # the total, though only 5 fit
    assert np.array_equal(ev[:cap].cpu().numpy(), full[:cap])
    assert (ev[cap:] == -7).all()                                   # nothing past the capacity


def test_predict_files(tmp_path, golden_dir):
    """Three WAV files of different lengths and one too short for a window: the events of the one ragged call are
    those of every file through audio.load + predict_windows + events_from_framewise; the short file is skipped;
    one XML per predicted file."""
    from sedx import audio, inference
    m = build(GRU)
    params = json.load(open(os.path.join(golden_dir, 'events.json')))['params_synthetic']
    seconds = {'a.wav': 5.0, 'b.wav': 100801 / 16000., 'short.wav': 3.0, 'c.wav': 8.0}
    paths = []
    for i, (name, sec) in enumerate(seconds.items()):
        wave = synth.make_waveforms(1, seconds=sec, sample_rate=16000, seed=40 + i)[0] * 0.5
        p = os.path.join(str(tmp_path), name)
        open(p, 'wb').write(A.write_wav(wave[None], 16000, 16))
        paths.append(p)
    out_dir = os.path.join(str(tmp_path), 'xml')
    os.mkdir(out_dir)
    got = inference.predict_files(m, paths, params, out_dir=out_dir)
    assert got.skipped == [paths[2]] and list(got) == [paths[0], paths[1], paths[3]]
    n_events = 0
    for p in got:
        y, _ = audio.load(p, sr=16000)
        with torch.no_grad():
            merged = inference.predict_windows(m, y[None], 5, 1.0)
        want = inference.events_from_framewise(merged, params, audio_name=p)
        assert got[p] == want, p
        n_events += len(want)
        xml = open(os.path.join(out_dir, os.path.basename(p)[:-4] + '.xml')).read()
        assert xml.startswith('<AudioDoc name="%s">' % os.path.basename(p)) and xml.endswith('</AudioDoc>')
        assert xml.count('<SoundSegment') == max(len(want), 1)
    assert n_events > 0
    assert not os.path.exists(os.path.join(out_dir, 'short.xml'))
    # chunked forwards: the same events
    assert dict(inference.predict_files(m, paths, params, max_windows_per_forward=2)) == dict(got)


def test_spin_timeout_raises_from_the_ragged_call():
    """As test_windows_spin_timeout_raises for the equal-length driver: a GRU hand-off spin that runs out inside
    the ragged forward (SEDX_TUNE_GRU_SPIN = 0) raises from predict_windows_ragged itself, and with the default
    bound the same handle is clean again."""
    from sedx import _lib, inference
    m, cat, lengths, alone = case(GRU, '16k', 'exact')
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    tune = lambda v: _lib.check(_lib.lib().sedx_set_tuning(nat.h, _lib.TUNE_GRU_SPIN, v), nat.h, 'set_tuning')
    with torch.no_grad():
        tune(0)
        try:
            with pytest.raises(RuntimeError, match='GRU'):
                inference.predict_windows_ragged(m, (cat, lengths))
        finally:
            tune(1 << 24)
        again = inference.predict_windows_ragged(m, (cat, lengths))
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(again, alone))
