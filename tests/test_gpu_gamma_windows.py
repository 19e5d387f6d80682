"""A gammatone model from raw audio on the GPU: model.forward_audio and the
windowed drivers (predict_windows, predict_windows_vote, predict_windows_ragged,
predict_files) against the oracle composition recorded in
tests/golden/gamma_windows.{json,npz} (tests/gamma_window_refs.py says what it
composes; tests/test_gamma_windows_cpu.py re-checks the fixture's conditions).

  codes      every window's int16 codes equal the oracle's in every cell (the
             fixture has no tie-guarded cell).  They are read by running the
             two-call path on the same windows: the conv input X0 the windowed
             call wrote (sedx_set_capture stage 0) equals the two-call path's X0
             bit for bit, and that path's features are the codes / 32767
  merged     within TOL of tests/test_gpu_parity.py of the oracle's merged
             framewise output (the measured value is printed); events identical
  identity   bit for bit: the ragged call against one predict_windows per clip
             and against the Python loop over windows a user needed before
             (gamma_features + forward + merge_host); forward_audio against
             gamma_features + forward at B = 1, 3, 9 (9: the item-claim path); an
             item alone against itself in the batch; a 0xFF-filled workspace;
             guard bytes around the workspace
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import gamma_refs as G
import gamma_window_refs as W
from oracle import audio_oracle as A
from oracle import sed_oracle as O
from sedx import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3                            # tests/test_gpu_parity.py
GRU = W.GRU
_models = {}


def build(preset, wseed=0):
    key = (preset, wseed)
    if key not in _models:
        from sedx import models
        p = O.PRESETS[preset]
        m = getattr(models, GRU)(p['sample_rate'], p['window_size'], p['hop_size'], 64, p['fmin'], p['fmax'], 25, 'gamma')
        sd = m.state_dict()
        for k, v in synth.make_state_dict(GRU, seed=wseed).items():
            sd[k] = torch.from_numpy(v)
        m.load_state_dict(sd, strict=True)
        _models[key] = m.to('cuda').eval()
    return _models[key]


@pytest.fixture(scope='module')
def golden(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, 'gamma_windows.json')))['cases']
    return meta, np.load(os.path.join(golden_dir, 'gamma_windows.npz'))


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def capture_x0(m, items, T, run):
    """run() with stage 0 captured -> (X0 [items, T, 64], the conv input, and run's result)."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    buf = torch.zeros((items, T, 64), dtype=torch.float32, device='cuda')
    _lib.check(L.sedx_set_capture(nat.h, 0, _p(buf), buf.numel() * 4), nat.h, 'set_capture')
    try:
        with torch.no_grad():
            out = run()
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'set_capture')
    return buf, out


def captured_codes(m, name, run):
    """The int16 codes of every window of run() [items, 64, T], read exactly: the conv input X0 that run() wrote
    (captured) equals, bit for bit, the X0 of the two-call path on the same windows (gamma_features on the
    pad_truncate'd windows, then the forward, captured too), and the two-call path's features are codes / 32767 in
    float32, so round(features * 32767) is the code.  -> (codes, run's result)"""
    from sedx import inference
    c = W.CASES[name]
    wins = np.stack([w for i in range(len(c.lengths)) for w in W.windows_of(name, i)])
    feats = inference.gamma_features(m, torch.from_numpy(wins).cuda())
    items, _, T = feats.shape
    x0_ref, _ = capture_x0(m, items, T, lambda: m(feats))
    x0, out = capture_x0(m, items, T, run)
    assert torch.equal(x0, x0_ref), float((x0 - x0_ref).abs().max())
    q = feats.double().cpu().numpy() * 32767.0
    codes = np.round(q)
    assert np.max(np.abs(q - codes)) < 1e-2          # float32(code / 32767) * 32767 is within 2e-3 of the code
    return codes.astype(np.int32), out


def oracle_codes(name):
    """[items, 64, T] int32: the oracle's codes of every window of every clip, clip by clip."""
    c = W.CASES[name]
    return np.concatenate([G.oracle(np.stack(W.windows_of(name, i)), c.preset).codes for i in range(len(c.lengths))])


def plain(events):
    return sorted((round(e['onset'], 6), round(e['offset'], 6), e['event_label']) for e in events)


def check_merged(name, clip, got, golden, what):
    meta, z = golden
    ref = z['%s_merged_%d' % (name, clip)]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print('%s %s clip %d: merged max|d| vs the oracle composition = %.3g' % (what, name, clip, e))
    assert e <= TOL
    from sedx import inference
    ev = inference.events_from_framewise(got[None], W.params(name), audio_name='clip%d' % clip)
    assert len(ev) > 0 and plain(ev) == plain(meta[name]['events'][clip])


def python_loop(m, name, clip):
    """What a user had to write before: features and a forward per window, then the host merge."""
    from sedx import inference
    c = W.CASES[name]
    outs = []
    with torch.no_grad():
        for w in W.windows_of(name, clip):
            x = torch.from_numpy(w[None]).cuda()
            outs.append(m(inference.gamma_features(m, x))['framewise_output'][0].cpu().numpy())
    return inference.merge_host(outs, c.sd, c.ov)[0]


@pytest.mark.parametrize('name', ['8k', '8k-odd'])
def test_ragged_windows(golden, name):
    """Clips of different (odd) lengths in one call: codes, merged output and events against the oracle; the call
    against one predict_windows per clip, chunked forwards and the Python loop, bit for bit."""
    from sedx import inference
    c = W.CASES[name]
    m = build(c.preset, c.wseed)
    clips = [torch.from_numpy(a).cuda() for a in W.clips(name)]
    ref = oracle_codes(name)
    codes, got = captured_codes(m, name, lambda: inference.predict_windows_ragged(m, clips, c.sd, c.ov))
    d = codes != ref
    print('%s: %d windows, int16 cells differing from the oracle: %d' % (name, ref.shape[0], int(d.sum())))
    assert d.sum() == 0
    for i, g in enumerate(got):
        g = g.cpu().numpy()
        check_merged(name, i, g, golden, 'ragged')
        with torch.no_grad():
            alone = inference.predict_windows(m, clips[i].clone()[None], c.sd, c.ov)[0].cpu().numpy()
        assert np.array_equal(g, alone), (i, float(np.max(np.abs(g - alone))))
        assert np.array_equal(g, python_loop(m, name, i)), i
    with torch.no_grad():
        for per in (1, 3):
            again = inference.predict_windows_ragged(m, clips, c.sd, c.ov, max_windows_per_forward=per)
            assert all(torch.equal(a, b) for a, b in zip(again, got)), per


def test_zero_padded_last_window(golden):
    """audio_duration past the samples: the last window's tail is pad_truncate's zeros (valid < len, the top_db
    floor), not what follows the clip in memory."""
    from sedx import inference
    name = '8k-pad'
    c = W.CASES[name]
    m = build(c.preset, c.wseed)
    # the clip inside a larger buffer of loud samples: a read past the clip would change the window's maximum
    buf = torch.full((c.lengths[0] + 16000,), 0.9, dtype=torch.float32, device='cuda')
    buf[:c.lengths[0]] = torch.from_numpy(W.clips(name)[0]).cuda()
    x = buf[:c.lengths[0]][None]
    ref = oracle_codes(name)
    codes, got = captured_codes(m, name, lambda: inference.predict_windows(m, x, c.sd, c.ov, audio_duration=c.dur[0]))
    assert (codes != ref).sum() == 0
    check_merged(name, 0, got[0].cpu().numpy(), golden, 'predict')
    assert np.array_equal(got[0].cpu().numpy(), python_loop(m, name, 0))


@pytest.mark.parametrize('spec', [0, 1], ids=['stockham', 'one-wave'])
def test_32k_windows(golden, spec):
    """nfft 2048 under both spectrum kernels (SEDX_TUNE_GAMMA_SPEC): window starts are even, so spec 1 runs the
    one-wave kernel's 8-byte loads through the item map."""
    from sedx import _lib, inference
    name = '32k'
    c = W.CASES[name]
    m = build(c.preset, c.wseed)
    m.set_tuning(_lib.TUNE_GAMMA_SPEC, spec)
    try:
        x = torch.from_numpy(W.clips(name)[0]).cuda()[None]
        ref = oracle_codes(name)
        codes, got = captured_codes(m, name, lambda: inference.predict_windows(m, x, c.sd, c.ov))
        d = codes != ref
        print('32k spec %d: int16 cells differing from the oracle: %d' % (spec, int(d.sum())))
        assert d.sum() == 0
        check_merged(name, 0, got[0].cpu().numpy(), golden, 'predict spec %d' % spec)
        # an odd base in the ragged call falls back to the Stockham kernel: the same bits
        pre =torch.from_numpy(synth.make_waveforms(1, seconds=5.0 + 1 / 32000., sample_rate=32000, seed=9)[0]).cuda()
        assert pre.shape[0] % 2 == 1
        with torch.no_grad():
            rag = inference.predict_windows_ragged(m, [pre, x[0]], c.sd, c.ov)
        assert torch.equal(rag[1], got[0])
    finally:
        m.set_tuning(_lib.TUNE_GAMMA_SPEC, 0)


def test_main_strong_and_vote(golden):
    """inference_prob_overlap's (0.5, 6) on a 10.5 s file, cut to 10 s: nine full windows and a shorter tail window
    as its own forward (its own frame count); and the vote merge of the same windows."""
    from sedx import inference
    meta, z = golden
    name = '8k-ms'
    c = W.CASES[name]
    m = build(c.preset, c.wseed)
    x = torch.from_numpy(W.clips(name)[0]).cuda()[None]
    assert inference.window_geometry(m, c.lengths[0], c.sd, c.ov, 'main_strong') == (10, 48000, 1050)
    with torch.no_grad():
        merged = inference.predict_windows(m, x, c.sd, c.ov, driver='main_strong')
        votes = inference.predict_windows_vote(m, x, c.sd, c.ov, c.low)
    check_merged(name, 0, merged[0].cpu().numpy(), golden, 'main_strong')
    v = votes[0].cpu().numpy()
    assert np.array_equal(v, z['8k-ms_votes_0'])
    ev = inference.events_from_votes(votes, c.ov, c.sd, W.params(name), ['clip0'])
    assert plain(ev) == plain(meta[name]['vote_events'][0])
    # sweep_overlap is these two calls per combination
    sw = inference.sweep_overlap(m, x, ['clip0'], W.params(name), combos=[[c.ov, c.sd]])
    assert plain(sw[(c.ov, c.sd)]) == plain(meta[name]['events'][0])


def test_predict_files(tmp_path, golden):
    """Two float32 WAV files at the model's rate (the decoded samples are the clips'): one call from paths to
    events, the events of the oracle composition."""
    from sedx import audio, inference
    meta, _ = golden
    name = '8k'
    c = W.CASES[name]
    m = build(c.preset, c.wseed)
    paths = []
    for i in (0, 1):
        p = os.path.join(str(tmp_path), 'clip%d.wav' % i)
        open(p, 'wb').write(A.write_wav(W.clips(name)[i][None], 8000, 32, 'float'))
        y, _sr = audio.load(p, sr=8000, device=torch.device('cuda'))
        assert np.array_equal(y.cpu().numpy(), W.clips(name)[i])
        paths.append(p)
    got = inference.predict_files(m, paths, W.params(name), sample_duration=c.sd, overlap_value=c.ov)
    assert got.skipped == [] and list(got) == paths
    for i, p in enumerate(paths):
        assert len(got[p]) > 0 and plain(got[p]) == plain(meta[name]['events'][i])


def _two_call(m, x):
    from sedx import inference
    with torch.no_grad():
        return m(inference.gamma_features(m, x))


@pytest.mark.parametrize('preset,L', [('8k', 16000), ('8k', 16001), ('32k', 2048 + 320 * 70)],
                         ids=['8k-2s', '8k-odd', '32k-T71'])
def test_forward_audio_is_the_two_call_path(preset, L):
    """All three outputs bit for bit at B = 1, 3 and 9 (from 8 clips the conv launches claim their items); each
    item alone equals itself in the batch; inference_prob routes a waveform batch the same way."""
    from sedx import inference
    m = build(preset)
    sr = O.PRESETS[preset]['sample_rate']
    wave = synth.make_waveforms(9, seconds=(L + 1.0) / sr, sample_rate=sr, seed=21)[:, :L]
    x9 = torch.from_numpy(np.ascontiguousarray(wave)).cuda()
    outs = {}
    for B in (1, 3, 9):
        x = x9[:B].contiguous()
        with torch.no_grad():
            got = m.forward_audio(x)
        ref = _two_call(m, x)
        assert set(got) == set(ref) == {'framewise_output', 'clipwise_output', 'embedding'}
        for k in ref:
            assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), (B, k)
        outs[B] = got
    for B in (3, 9):
        for k in outs[1]:
            assert torch.equal(outs[B][k][:1], outs[1][k]), (B, k)
    with torch.no_grad():
        alone = m.forward_audio(x9[8:9].contiguous())
    assert all(torch.equal(alone[k], outs[9][k][8:9]) for k in alone)
    ip = inference.inference_prob(m, wave[:3], batch_size=2)
    assert np.array_equal(ip['framewise_output'], outs[3]['framewise_output'].cpu().numpy())


def test_workspace_hygiene():
    """sedx_forward_audio and sedx_forward_windows on a caller's workspace filled with 0xFF, between guard bands:
    the same bits as on a clean one, the guards intact, one byte less refused."""
    from sedx import _lib
    L = _lib.lib()
    m = build('8k')
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    x = torch.from_numpy(synth.make_waveforms(3, seconds=4.0, sample_rate=8000, seed=33)).cuda()
    B, n = x.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    GUARD = 4096

    def guarded(nbytes, fill):
        buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
        buf[GUARD:GUARD + nbytes] = fill
        return buf

    def intact(buf, nbytes):
        return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())

    # the one-call forward
    wsz = ctypes.c_size_t()
    _lib.check(L.sedx_audio_workspace_size(nat.h, B, n, ctypes.byref(wsz)), nat.h, 'audio_workspace_size')
    fr, sl = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.sedx_audio_geometry(nat.h, n, None, ctypes.byref(fr), ctypes.byref(sl)), nat.h, 'audio_geometry')
    res = []
    for fill in (0x00, 0xFF):
        ws = guarded(wsz.value, fill)
        fw = torch.empty((B, fr.value, 25), dtype=torch.float32, device='cuda')
        cl = torch.empty((B, 25), dtype=torch.float32, device='cuda')
        _lib.check(L.sedx_forward_audio(nat.h, _p(x), B, n, _p(fw), _p(cl), None, ctypes.c_void_p(ws.data_ptr() + GUARD),
                                        wsz.value, stream), nat.h, 'forward_audio')
        torch.cuda.synchronize()
        assert intact(ws, wsz.value)
        res.append((fw, cl))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    with torch.no_grad():
        own = m.forward_audio(x)
    assert torch.equal(own['framewise_output'], res[0][0])
    assert L.sedx_forward_audio(nat.h, _p(x), B, n, _p(fw), _p(cl), None, ctypes.c_void_p(ws.data_ptr() + GUARD),
                                wsz.value - 1, stream) == 1 and b'workspace too small' in L.sedx_last_error(nat.h)
    # what the size queries refuse the forwards refuse: a clip shorter than the FFT, fewer than 8 frames
    for bad in (511, 512 + 80 * 6):
        assert L.sedx_audio_workspace_size(nat.h, B, bad, ctypes.byref(ctypes.c_size_t())) == 1
        msg = L.sedx_last_error(nat.h)
        assert L.sedx_forward_audio(nat.h, _p(x), B, bad, _p(fw), _p(cl), None, None, 0, stream) == 1
        assert L.sedx_last_error(nat.h) == msg
    # the windowed driver
    spec = _lib.window_spec(2, 1.0)
    _lib.check(L.sedx_window_workspace_size(nat.h, B, n, ctypes.byref(spec), ctypes.byref(wsz)), nat.h, 'window size')
    res = []
    for fill in (0x00, 0xFF):
        ws = guarded(wsz.value, fill)
        merged = torch.empty((B, 400, 25), dtype=torch.float32, device='cuda')
        _lib.check(L.sedx_forward_windows(nat.h, _p(x), B, n, ctypes.byref(spec), _p(merged),
                                          ctypes.c_void_p(ws.data_ptr() + GUARD), wsz.value, stream), nat.h, 'windows')
        torch.cuda.synchronize()
        assert intact(ws, wsz.value)
        res.append(merged)
    assert torch.equal(res[0], res[1]) and bool(torch.isfinite(res[0]).all())
