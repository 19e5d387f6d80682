"""Fused segment counts on the GPU (csrc/calib.hip) and the threshold
optimiser on a HIP tensor: device == host entry bit for bit (integer counts,
float64 scores), over the bitmap word boundaries, the register / re-read
paths (T <= 1024 / longer), partial workgroups and the `bad` column.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from sedx import _lib, calibrate, inference, synth

pytestmark = pytest.mark.gpu

GRU = 'Cnn_9layers_Gru_FrameAtt'


def _series(rng, N, T, C):
    fw = rng.uniform(0, 1, (N, T, C)).astype(np.float32)
    return (np.cumsum(fw - 0.5, axis=1) / 8 + 0.5).astype(np.float32)


def _case(rng, N, T, C, V, seg):
    fw = _series(rng, N, T, C)
    S = (T + seg - 1) // seg
    targets = (rng.uniform(0, 1, (N, S, C)) < 0.4).astype(np.uint8)
    high = rng.uniform(0.4, 0.7, (V, C))
    low = rng.uniform(-0.1, 0.4, (V, C))
    return fw, targets, high, low, rng.integers(0, 12, C), rng.integers(0, 12, C)


def _both(fw, targets, high, low, ns, nsalt, seg):
    host = calibrate.segment_counts(fw, targets, high, low, ns, nsalt, seg)
    dev = calibrate.segment_counts(torch.from_numpy(fw).cuda(), targets, high, low, ns, nsalt, seg)
    assert dev.dtype == np.int64 and dev.shape == host.shape
    return host, dev


@pytest.mark.parametrize('T', [1, 63, 64, 65, 100, 101, 999, 1000, 1001, 6400])
def test_device_counts_match_host(T):
    rng = np.random.default_rng(77 + T)
    for seg in (100, 64, 7):
        if (T + seg - 1) // seg > 64:
            continue
        for N, C, V in ((1, 1, 11), (3, 7, 1), (9, 25, 11)):
            if T == 6400:
                N = min(N, 3)
            fw, targets, high, low, ns, nsalt = _case(rng, N, T, C, V, seg)
            host, dev = _both(fw, targets, high, low, ns, nsalt, seg)
            np.testing.assert_array_equal(dev, host, err_msg='T=%d seg=%d N=%d C=%d V=%d' % (T, seg, N, C, V))


def test_device_counts_structured_series():
    """All-on, all-off, alternating, 64-frame blocks and last-frame-only series
    (the `bad` column), with a positive and a negative low threshold."""
    rng = np.random.default_rng(5)
    for T in (1, 2, 63, 64, 65, 127, 128, 129, 1000, 1024, 1025, 4096):
        C = 7
        seg = max(1, (T + 63) // 64)
        fw = _series(rng, 3, T, C)
        fw[0, :, 0] = 0.9
        fw[0, :, 1] = 0.1
        fw[0, :, 2] = np.where(np.arange(T) % 2 == 0, 0.9, 0.1)
        fw[0, :, 3] = np.where((np.arange(T) // 64) % 2 == 0, 0.9, 0.35)
        fw[0, :, 4] = np.where(np.arange(T) >= T - 1, 0.9, 0.1)
        fw[1, :, 4] = np.where((np.arange(T) >= T - 1) | (np.arange(T) < T // 2), 0.9, 0.1)   # 2nd run at the last frame
        S = (T + seg - 1) // seg
        targets = (rng.uniform(0, 1, (3, S, C)) < 0.5).astype(np.uint8)
        high = np.full((3, C), 0.5)
        low = np.stack([np.full(C, 0.3), np.full(C, -0.1), np.full(C, 0.45)])
        host, dev = _both(fw, targets, high, low, int(rng.integers(0, 4)), int(rng.integers(0, 4)), seg)
        np.testing.assert_array_equal(dev, host, err_msg='T=%d' % T)
        if T >= 4:
            assert host[0, 4, 3] >= 1, T      # the `bad` column is exercised


def test_device_counts_dirty_buffers():
    """The entry point zeroes d_counts and owns the workspace contents."""
    rng = np.random.default_rng(9)
    N, T, C, V, seg = 5, 333, 6, 4, 50
    fw, targets, high, low, ns, nsalt = _case(rng, N, T, C, V, seg)
    host = calibrate.segment_counts(fw, targets, high, low, ns, nsalt, seg)
    L = _lib.lib()
    x = torch.from_numpy(fw).cuda()
    masks = torch.from_numpy(calibrate.pack_targets(targets).view(np.int64)).cuda()
    wsz = ctypes.c_size_t()
    assert L.sedx_segment_counts_workspace_size(N, T, C, V, ctypes.byref(wsz)) == _lib.SEDX_OK
    ws = torch.full((wsz.value,), 0xFF, dtype=torch.uint8, device='cuda')
    counts = torch.full((V, C, 4), -1, dtype=torch.int64, device='cuda')       # 0xFF bytes
    ns64, nsalt64 = np.ascontiguousarray(ns, np.int64), np.ascontiguousarray(nsalt, np.int64)
    c = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    st = L.sedx_segment_counts_device(p(x), N, T, C, p(masks), seg, V, c(high), c(low), c(ns64), c(nsalt64),
                                      p(counts), p(ws), wsz.value, stream)
    assert st == _lib.SEDX_OK
    np.testing.assert_array_equal(counts.cpu().numpy(), host)
    # limits: the device entry refuses what the host entry refuses
    for args in ((6401, 100, 1), (100, 100, 0), (100, 100, 65)):
        st = L.sedx_segment_counts_device(p(x), 1, args[0], 1, p(masks), args[1], args[2], c(high), c(low), c(ns64),
                                          c(nsalt64), p(counts), p(ws), wsz.value, stream)
        assert _lib.STATUS[st] == 'EINVAL', args


def test_device_counts_rebuilt_from_event_pairs():
    """V = 1 counts equal the counts rebuilt from inference.event_pairs on the GPU."""
    rng = np.random.default_rng(13)
    N, T, C, seg = 4, 700, 25, 100
    fw, targets, high, low, ns, nsalt = _case(rng, N, T, C, 1, seg)
    low = np.abs(low)
    fw[:, -1] = fw[:, -2]                 # no run can begin at the last frame: no bad series
    x = torch.from_numpy(fw).cuda()
    dev = calibrate.segment_counts(x, targets, high, low, ns, nsalt, seg)
    params = {'sed_high_threshold': high[0].tolist(), 'sed_low_threshold': low[0].tolist(),
              'n_smooth': [int(v) for v in ns], 'n_salt': [int(v) for v in nsalt]}
    pairs = inference.event_pairs(x, params)
    est = np.zeros((N, 7, C), bool)
    for n, k, b, f in pairs.tolist():
        est[n, b // seg:-(-f // seg), k] = True
    ref = targets != 0
    want = np.stack([(est & ref).sum(axis=(0, 1)), (est & ~ref).sum(axis=(0, 1)), (ref & ~est).sum(axis=(0, 1)),
                     np.zeros(C, np.int64)], axis=1)
    np.testing.assert_array_equal(dev[0], want)
    np.testing.assert_array_equal(calibrate.segment_counts_fallback(x, targets, high, low, ns, nsalt, seg), dev)


def test_optimizer_on_device_reproduces_reference_trajectory(golden_dir):
    g = json.load(open(os.path.join(golden_dir, 'calibrate_kat.json')))
    data = synth.make_calibration_set(g['n_clips'], g['frames'], g['classes'], seed=g['seed'])
    assert hashlib.sha256(data['framewise'].tobytes() + data['targets'].tobytes()).hexdigest() == g['sha256']
    score, params, record = calibrate.optimize_sed_thresholds(
        torch.from_numpy(data['framewise']).cuda(), data['targets'], learning_rate=g['learning_rate'],
        epochs=g['epochs'], step=g['step'], max_search=g['max_search'])
    for i, want in enumerate(g['record']):
        assert record[i]['score'] == want['score'], i
        np.testing.assert_allclose(record[i]['thresholds'], want['thresholds'], rtol=0, atol=1e-12)
    assert score == g['final_score']
    assert params['audio_tagging_threshold'] == [0.5] * g['classes']


def test_optimizer_device_equals_host_on_model_outputs():
    """Two epochs on the GRU model's framewise outputs of 4 synthetic 10 s
    clips: the device and the host path give the same record."""
    from sedx import models
    m = getattr(models, GRU)(16000, 512, 160, 64, 25, 7000, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(GRU, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    m = m.to('cuda').eval()
    wave = synth.make_waveforms(4, seconds=10.0, sample_rate=16000, seed=21)
    with torch.no_grad():
        fw = m(torch.from_numpy(wave).cuda())['framewise_output']
    N, T, C = fw.shape
    # thresholds at each class's own level (random-init outputs move little), so that events
    # exist and probes change them
    host_fw = fw.cpu().numpy()
    level = np.median(host_fw, axis=(0, 1))
    rng = np.random.default_rng(2)
    targets = (rng.uniform(0, 1, (N, (T + 99) // 100, C)) < 0.5).astype(np.uint8)
    init = {'sed_high_threshold': level.tolist(), 'sed_low_threshold': (level - 0.01).tolist()}
    kw = dict(init=init, epochs=2, step=0.005, learning_rate=5e-3)
    try:
        host = calibrate.optimize_sed_thresholds(host_fw, targets, **kw)
    except RuntimeError:
        with pytest.raises(RuntimeError):
            calibrate.optimize_sed_thresholds(fw, targets, **kw)
        return
    dev = calibrate.optimize_sed_thresholds(fw, targets, **kw)
    assert dev[0] == host[0] and dev[1] == host[1] and dev[2] == host[2]
    assert host[0] > 0.0
