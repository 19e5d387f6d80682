"""Average precision ranked on the GPU (csrc/rank.hip) and the Evaluator on
top of it.  For every case: `ap` of the device entry is bit-identical to the
host entry's (csrc/rank_host.cpp), `info` and the curve are equal, and `ap` is
within evaluate_refs.bound(K) = 8 (K + 4) 2^-53 of sklearn on every class with
P >= 1 (a class with P = 0 is never compared with sklearn, which says 0.0
there: NaN and info are asserted instead).  Cases aim at the radix tile
(sedx_rank_tile), the wavefront width, each digit pass on its own, presorted
and x8-repeated scores, signs / zeros / denormals, a bin counter's width
(70 000 equal scores), and the class-group boundary of the workspace.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score

import evaluate_refs as R
from sedx import _lib, calibrate, evaluate, inference, models, synth

pytestmark = pytest.mark.gpu

GRU = 'Cnn_9layers_Gru_FrameAtt'


def _tile():
    return int(_lib.lib().sedx_rank_tile())


def _check(t, s, empty=None, nonfinite=None, what=''):
    """Device == host (ap bits, info, whole curve arrays); ap vs sklearn."""
    d_ap, d_info, d_thr, d_tp, d_n = evaluate.rank(t, torch.from_numpy(s).cuda(), curve=True, check=False)
    h_ap, h_info, h_thr, h_tp, h_n = evaluate.rank(t, s, curve=True, check=False)
    assert d_ap.dtype == np.float64 and d_info.dtype == np.int64
    np.testing.assert_array_equal(d_info, h_info, err_msg=what)
    np.testing.assert_array_equal(d_ap.view(np.uint64), h_ap.view(np.uint64), err_msg=what)
    np.testing.assert_array_equal(d_thr.view(np.uint32), h_thr.view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(d_tp, h_tp, err_msg=what)
    np.testing.assert_array_equal(d_n, h_n, err_msg=what)
    M, C = s.shape
    skipped = []
    for c in range(C):
        P, K, bad = (int(v) for v in d_info[c])
        assert P == int(t[:, c].sum()), what
        if c == nonfinite:
            assert bad > 0 and K == 0 and np.isnan(d_ap[c]), what
            skipped.append(c)
            continue
        assert bad == 0, what
        if P == 0:
            assert c == empty and np.isnan(d_ap[c]) and K >= 1, what
            skipped.append(c)
            continue
        sk = average_precision_score(t[:, c], s[:, c])
        err = abs(d_ap[c] - sk)
        assert err <= R.bound(K), '%s class %d: |ap - sklearn| = %.3g > %.3g (K = %d)' % (what, c, err, R.bound(K), K)
    # nothing but the designated classes was left out of the sklearn comparison
    assert sorted(skipped) == sorted(c for c in (empty, nonfinite) if c is not None), what
    return d_ap, d_info


def _sizes():
    t = 4096   # asserted equal to sedx_rank_tile() in the test
    out = []
    for M in (1, 2, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 3 * t + 5):
        for C in (1, 7, 25, 527):
            if M * C <= 2200000:
                out.append((M, C))
    return out


@pytest.mark.parametrize('M,C', _sizes())
def test_size_sweep(M, C):
    assert _tile() == 4096           # the sweep above is built from this value
    for kind in ('uniform', 'coarse'):
        t, s = R.make_case(M, C, 1000 + M + C, kind)
        _check(t, s, what='%s M=%d C=%d' % (kind, M, C))


@pytest.mark.parametrize('byte', [0, 1, 2, 3])
def test_one_digit_pass_decides(byte):
    t, s = R.digit_case(2 * _tile() + 77, 7, byte, 40 + byte)
    bits = s.view(np.uint32)
    assert np.all((bits ^ bits[0, 0]) & ~(np.uint32(0xff) << np.uint32(8 * byte)) == 0)
    _check(t, s, what='byte %d' % byte)


@pytest.mark.parametrize('kind', ['ascending', 'descending', 'x8', 'mixed'])
def test_orderings_and_values(kind):
    t, s = R.make_case(3 * _tile() + 5, 7, 7, kind)
    if kind == 'mixed':
        assert (s == 0).any() and np.signbit(s[s == 0]).any() and (np.abs(s[s != 0]) < 1e-38).any()
    _check(t, s, what=kind)


def test_framewise_shape_x8():
    """[N, T, C] as it lies, scores repeated x8 along T."""
    rng = np.random.RandomState(3)
    N, T, C = 6, 1000, 25
    s = np.repeat(rng.rand(N, T // 8, C).astype(np.float32), 8, axis=1)
    t = (rng.rand(N, T, C) < 0.2).astype(np.uint8)
    t[0, 0, :] = 1
    ap = evaluate.sed_average_precision(torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda(), None)
    host = evaluate.sed_average_precision(t, s, None)
    np.testing.assert_array_equal(ap.view(np.uint64), host.view(np.uint64))
    sk = average_precision_score(t.reshape(-1, C), s.reshape(-1, C), average=None)
    assert np.all(np.abs(ap - sk) <= R.bound(N * T // 8))
    with pytest.raises(ValueError):
        evaluate.sed_average_precision(torch.from_numpy(t[:, :-1]).cuda(), torch.from_numpy(s).cuda(), None)


def test_all_scores_equal_70000():
    """One run of 70 000 equal keys: a 16-bit bin counter would wrap."""
    t, s = R.make_case(70000, 1, 5, 'equal')
    ap, info = _check(t, s, what='equal')
    P = int(t.sum())
    assert info[0].tolist() == [P, 1, 0] and ap[0] == P / 70000.0


def test_empty_full_and_nonfinite_classes():
    M, C = _tile() + 33, 7
    t, s = R.make_case(M, C, 11, 'uniform', empty=2, full=4)
    ap, info = _check(t, s, empty=2, what='empty/full')
    assert info[2, 0] == 0 and info[4, 0] == M and ap[4] == 1.0
    clean = ap.copy()
    s2 = s.copy()
    s2[[5, 900, M - 1], 5] = [np.nan, np.inf, -np.inf]
    ap2, info2 = _check(t, s2, empty=2, nonfinite=5, what='non-finite')
    assert info2[5].tolist() == [int(t[:, 5].sum()), 0, 3]
    keep = [c for c in range(C) if c not in (2, 5)]
    np.testing.assert_array_equal(ap2[keep].view(np.uint64), clean[keep].view(np.uint64))
    with pytest.raises(ValueError, match='non-finite'):
        evaluate.average_precision(t, torch.from_numpy(s2).cuda())


def test_column_position_and_class_count_do_not_change_the_bits():
    M = _tile() + 1
    t, s = R.make_case(M, 25, 21, 'coarse')
    ap25 = evaluate.average_precision(t, torch.from_numpy(s).cuda())
    for c in (0, 13, 24):
        alone = evaluate.average_precision(t[:, c:c + 1].copy(), torch.from_numpy(s[:, c:c + 1].copy()).cuda())
        assert alone.view(np.uint64)[0] == ap25.view(np.uint64)[c]
        t7, s7 = R.make_case(M, 7, 22, 'uniform')
        t7[:, 5], s7[:, 5] = t[:, c], s[:, c]
        moved = evaluate.average_precision(t7, torch.from_numpy(s7).cuda())
        assert moved.view(np.uint64)[5] == ap25.view(np.uint64)[c]


def test_class_groups():
    """M large enough that 25 classes do not fit one group of the workspace."""
    M, C = 220000, 25
    t, s = R.make_case(M, C, 31, 'x8', empty=24)
    wsz = ctypes.c_size_t()
    assert _lib.lib().sedx_average_precision_workspace_size(M, C, ctypes.byref(wsz)) == 0
    assert wsz.value < 14 * M * C            # fewer than C classes are resident
    _check(t, s, empty=24, what='groups')
    # average= forms on the device
    keep = np.arange(C - 1)
    d = torch.from_numpy(s[:, keep].copy()).cuda()
    sk = average_precision_score(t[:, keep], s[:, keep], average='macro')
    assert abs(evaluate.average_precision(t[:, keep], d, 'macro') - sk) <= R.bound(M // 8 + 8)
    assert np.isnan(evaluate.average_precision(t, torch.from_numpy(s).cuda(), 'macro'))
    tm, sm = t[:20000, keep], s[:20000, keep]
    micro = evaluate.average_precision(tm, torch.from_numpy(sm.copy()).cuda(), 'micro')
    assert abs(micro - average_precision_score(tm, sm, average='micro')) <= R.bound(tm.size)


def _raw(L, t, s, ws, ws_bytes):
    M, C = s.shape
    out = torch.empty(4 * C, dtype=torch.int64, device='cuda')
    null = ctypes.c_void_p(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    st = L.sedx_average_precision_device(ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(t.data_ptr()), M, C,
                                         ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out[C:].data_ptr()),
                                         null, null, null, ctypes.c_void_p(ws.data_ptr()), ws_bytes, stream)
    return st, out


def test_workspace_too_small_and_argument_errors():
    L = _lib.lib()
    t, s = R.make_case(1000, 3, 1, 'uniform')
    dt, ds = torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda()
    wsz = ctypes.c_size_t()
    assert L.sedx_average_precision_workspace_size(1000, 3, ctypes.byref(wsz)) == 0
    ws = torch.empty(wsz.value, dtype=torch.uint8, device='cuda')
    st, _ = _raw(L, dt, ds, ws, wsz.value - 1)
    assert st == 1 and b'workspace too small' in L.sedx_last_error(None)
    assert L.sedx_average_precision_workspace_size(0, 3, ctypes.byref(wsz)) == 1
    assert b'M = 0' in L.sedx_last_error(None)
    assert L.sedx_average_precision_workspace_size(10, 65536, ctypes.byref(wsz)) == 1
    assert b'C = 65536' in L.sedx_last_error(None)
    st, out = _raw(L, dt, ds, ws, ws.numel())
    assert st == 0
    torch.cuda.synchronize()


def test_two_calls_on_one_stream_without_a_sync():
    L = _lib.lib()
    M, C = 2 * _tile() + 3, 7
    ta, sa = R.make_case(M, C, 51, 'uniform')
    tb, sb = R.make_case(M, C, 52, 'coarse')
    wsz = ctypes.c_size_t()
    assert L.sedx_average_precision_workspace_size(M, C, ctypes.byref(wsz)) == 0
    ws = torch.empty(wsz.value, dtype=torch.uint8, device='cuda')
    dev = [(torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda()) for t, s in ((ta, sa), (tb, sb))]
    torch.cuda.synchronize()
    outs = []
    for dt, ds in dev:                       # the same workspace, no host sync in between
        st, out = _raw(L, dt, ds, ws, ws.numel())
        assert st == 0
        outs.append(out)
    torch.cuda.synchronize()
    for out, (t, s) in zip(outs, ((ta, sa), (tb, sb))):
        host = out.cpu().numpy()
        h_ap, h_info = evaluate.rank(t, s)[:2]
        np.testing.assert_array_equal(host[:C].view(np.uint64), h_ap.view(np.uint64))
        np.testing.assert_array_equal(host[C:].reshape(C, 3), h_info)


def test_evaluator_end_to_end(tmp_path):
    m = getattr(models, GRU)(16000, 512, 160, 64, 25, 7000, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(GRU, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd)
    m = m.to('cuda:0').eval()
    wave = synth.make_waveforms(3, seconds=1.0, sample_rate=16000, seed=9)
    names = ['clip%d.wav' % i for i in range(3)]
    labels = inference.LABELS
    rng = np.random.RandomState(4)
    rows = []
    for i, name in enumerate(names):
        for k in rng.choice(25, size=9, replace=False):
            on = round(float(rng.uniform(0, 0.6)), 3)
            rows.append((name, on, round(on + float(rng.uniform(0.05, 0.4)), 3), labels[k]))
    csv = str(tmp_path / 'reference.csv')
    with open(csv, 'w') as f:
        for r in rows:
            f.write('%s\t%s\t%s\t%s\n' % r)
    strong = evaluate.strong_targets(csv, names, frames_num=100)
    weak = evaluate.weak_targets(csv, names)
    assert strong.shape == (3, 100, 25) and np.array_equal(strong.any(axis=1), weak != 0)
    batches = [{'audio_name': np.array(names[:2]), 'waveform': wave[:2], 'target': weak[:2],
                'strong_target': strong[:2]},
               {'audio_name': np.array(names[2:]), 'waveform': wave[2:], 'target': weak[2:],
                'strong_target': strong[2:]}]
    sub = str(tmp_path / 'submission.csv')
    stats, out = evaluate.Evaluator(m).evaluate(batches, csv, sub, 100)

    assert set(out) == {'audio_name', 'clipwise_output', 'framewise_output', 'target', 'strong_target'}
    assert out['audio_name'].tolist() == names
    assert out['clipwise_output'].shape == (3, 25) and out['framewise_output'].shape == (3, 100, 25)
    assert out['target'].shape == (3, 25) and out['strong_target'].shape == (3, 100, 25)
    assert all(isinstance(v, np.ndarray) for v in out.values())
    assert np.array_equal(out['strong_target'] != 0, strong != 0)

    for key, tgt, scr, K in (('clipwise_ap', weak, out['clipwise_output'], 3),
                             ('framewise_ap', strong.reshape(-1, 25), out['framewise_output'].reshape(-1, 25), 300)):
        ap = stats[key]
        assert ap.shape == (25,) and ap.dtype == np.float64
        for c in range(25):
            if tgt[:, c].sum() == 0:
                assert np.isnan(ap[c])
            else:
                assert abs(ap[c] - average_precision_score(tgt[:, c], scr[:, c])) <= R.bound(K), (key, c)
    assert np.isfinite(stats['framewise_ap']).sum() >= 9

    events = inference.events_from_framewise(torch.from_numpy(out['framewise_output']).cuda(), evaluate.SED_PARAMS,
                                             names, 100, labels, sort=False)
    by_hand = str(tmp_path / 'by_hand.csv')
    inference.write_submission(events, by_hand)
    assert open(sub).read() == open(by_hand).read()
    assert stats['sed_metrics'] == calibrate.segment_metrics(events, csv, names)
