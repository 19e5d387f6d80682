"""SED threshold calibration on the host entry (sedx.calibrate, csrc/segments.cpp):
the optimiser against the reference's recorded trajectory
(tools/make_golden_calibrate.py), segment counts against a brute-force count
over the CPU oracle's activity_detection, the ABI's limits, the per-candidate
fallback, targets and metrics.  Integer counts and scores must be equal.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import sed_oracle as O
from sedx import _lib, calibrate, inference, synth


def _series(rng, N, T, C):
    fw = rng.uniform(0, 1, (N, T, C)).astype(np.float32)
    return (np.cumsum(fw - 0.5, axis=1) / 8 + 0.5).astype(np.float32)


def brute_counts(fw, targets, high, low, ns, nsalt, seg):
    """activity_detection per series (CPU oracle), then a per-segment loop.
    Thresholds are rounded to float32 first: the library compares in float32."""
    N, T, C = fw.shape
    S = (T + seg - 1) // seg
    V = high.shape[0]
    out = np.zeros((V, C, 4), np.int64)
    for v in range(V):
        for n in range(N):
            for k in range(C):
                x = fw[n, :, k]
                try:
                    pairs = O.activity_detection(x, np.float32(high[v, k]), np.float32(low[v, k]), int(ns[k]),
                                                 int(nsalt[k]))
                except IndexError:
                    out[v, k, 3] += 1
                    continue
                for s in range(S):
                    est = any(b < (s + 1) * seg and f > s * seg and f > b for b, f in pairs)
                    ref = bool(targets[n, s, k])
                    out[v, k, 0] += est and ref
                    out[v, k, 1] += est and not ref
                    out[v, k, 2] += ref and not est
    return out


def _case(rng, N, T, C, V, seg):
    fw = _series(rng, N, T, C)
    S = (T + seg - 1) // seg
    targets = (rng.uniform(0, 1, (N, S, C)) < 0.4).astype(np.uint8)
    high = rng.uniform(0.4, 0.7, (V, C))
    low = rng.uniform(-0.1, 0.4, (V, C))
    ns = rng.integers(0, 12, C)
    nsalt = rng.integers(0, 12, C)
    return fw, targets, high, low, ns, nsalt


SHAPES = [(T, seg, C, V)
          for T in (1, 63, 64, 65, 100, 101, 999, 1000, 1001, 6400)
          for seg in (100, 64, 7) if (T + seg - 1) // seg <= 64
          for C, V in ((1, 11), (7, 1), (25, 11))]


@pytest.mark.parametrize('T,seg,C,V', SHAPES)
def test_segment_counts_match_brute_force(T, seg, C, V):
    rng = np.random.default_rng(1000 * T + 10 * seg + C + V)
    N = 2 if T < 6400 else 1
    fw, targets, high, low, ns, nsalt = _case(rng, N, T, C, V, seg)
    got = calibrate.segment_counts(fw, targets, high, low, ns, nsalt, seg)
    assert got.dtype == np.int64 and got.shape == (V, C, 4)
    np.testing.assert_array_equal(got, brute_counts(fw, targets, high, low, ns, nsalt, seg))
    # packed masks are the same input
    np.testing.assert_array_equal(
        calibrate.segment_counts(fw, calibrate.pack_targets(targets), high, low, ns, nsalt, seg), got)


def test_bad_series_is_counted_and_adds_nothing():
    T, C = 200, 3
    fw = np.full((2, T, C), 0.05, np.float32)
    fw[0, 10:60, 0] = 0.9                 # an event, then a run that begins at the last frame
    fw[0, -1, 0] = 0.9
    fw[1, 10:60, 0] = 0.9
    fw[1, 20:90, 1] = 0.9
    targets = np.ones((2, 2, C), np.uint8)
    got = calibrate.segment_counts(fw, targets, 0.5, 0.1, 1, 1, 100)
    want = brute_counts(fw, targets, np.full((1, C), 0.5), np.full((1, C), 0.1), [1] * C, [1] * C, 100)
    np.testing.assert_array_equal(got, want)
    assert got[0, 0].tolist() == [1, 0, 1, 1]          # clip 0 of class 0 is bad, clip 1 counts
    assert got[0, 1].tolist() == [1, 0, 3, 0]


def _raw_counts(N, T, C, seg, V):
    L = _lib.lib()
    fw = np.zeros((N, T, C), np.float32)
    tg = np.zeros((N, C), np.uint64)
    hi = np.full((max(V, 1), C), 0.5)
    lo = np.full((max(V, 1), C), 0.1)
    ns = np.full(C, 10, np.int64)
    counts = np.zeros((max(V, 1), C, 4), np.int64)
    c = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    st = L.sedx_segment_counts(c(fw), N, T, C, c(tg), seg, V, c(hi), c(lo), c(ns), c(ns), c(counts))
    return st, L.sedx_last_error(None).decode()


def test_limits_return_einval_with_a_message():
    assert _raw_counts(1, 6400, 2, 100, 1)[0] == _lib.SEDX_OK
    for args, word in (((1, 6401, 2, 100, 1), 'segments'), ((1, 100, 2, 100, 0), 'variants'),
                       ((1, 100, 2, 100, 65), 'variants'), ((1, 100, 2, 0, 1), 'segment_frames')):
        st, msg = _raw_counts(*args)
        assert _lib.STATUS[st] == 'EINVAL', args
        assert word in msg, (args, msg)
    assert _raw_counts(1, 100, 2, 100, 64)[0] == _lib.SEDX_OK


def test_fallback_matches_fused_and_takes_over_past_the_limits():
    rng = np.random.default_rng(3)
    fw, targets, high, low, ns, nsalt = _case(rng, 3, 500, 7, 11, 100)
    fw[1, :, 2] = -0.5
    fw[1, 10:60, 2] = 0.9
    fw[1, -1, 2] = 0.9                    # a second run at the last frame: bad in every variant
    fused = calibrate.segment_counts(fw, targets, high, low, ns, nsalt, 100)
    assert fused[:, 2, 3].tolist() == [1] * 11
    np.testing.assert_array_equal(calibrate.segment_counts_fallback(fw, targets, high, low, ns, nsalt, 100), fused)
    # S = 72 > 64 and V = 65 > 64: segment_counts itself takes the per-candidate path
    fw, targets, high, low, ns, nsalt = _case(rng, 1, 500, 3, 2, 7)
    np.testing.assert_array_equal(calibrate.segment_counts(fw, targets, high, low, ns, nsalt, 7),
                                  brute_counts(fw, targets, high, low, ns, nsalt, 7))
    fw, targets, high, low, ns, nsalt = _case(rng, 1, 120, 2, 65, 100)
    got = calibrate.segment_counts(fw, targets, high, low, ns, nsalt, 100)
    np.testing.assert_array_equal(got[:64], calibrate.segment_counts(fw, targets, high[:64], low[:64], ns, nsalt, 100))
    np.testing.assert_array_equal(got[64:], calibrate.segment_counts(fw, targets, high[64:], low[64:], ns, nsalt, 100))


def test_segment_targets_grid(tmp_path):
    labels = ['a', 'b']
    ev = [{'filename': 'f0', 'onset': 0.999, 'offset': 1.0, 'event_label': 'a'},
          {'filename': 'f1', 'onset': 2.0, 'offset': 3.001, 'event_label': 'b'},
          {'filename': 'f1', 'onset': 8.5, 'offset': 30.0, 'event_label': 'a'},
          {'filename': 'other', 'onset': 0.0, 'offset': 5.0, 'event_label': 'a'}]
    t = calibrate.segment_targets(ev, ['f0', 'f1'], labels, n_segments=10)
    assert t.dtype == np.uint8 and t.shape == (2, 10, 2)
    assert t[0, :, 0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]      # onset 0.999 -> segment 0, offset 1.0 -> end 1
    assert t[1, :, 1].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0]      # offset 1.001 past the grid line -> end + 1
    assert t[1, :, 0].tolist() == [0] * 8 + [1, 1]
    assert int(t.sum()) == 5
    masks = calibrate.pack_targets(t)
    assert masks.dtype == np.uint64 and masks.tolist() == [[1, 0], [0x300, 0xC]]
    p = tmp_path / 'ref.csv'
    p.write_text(''.join('%s\t%s\t%s\t%s\n' % (e['filename'], e['onset'], e['offset'], e['event_label']) for e in ev))
    np.testing.assert_array_equal(calibrate.segment_targets(str(p), ['f0', 'f1'], labels, 10), t)


def test_metrics_and_error_rate_hand_made():
    labels = ['a', 'b']
    # three segments; reference: a in 0-1, b in 1-2; estimate: a in 0, b in 0, a in 2
    ref = [{'filename': 'f', 'onset': 0.0, 'offset': 2.0, 'event_label': 'a'},
           {'filename': 'f', 'onset': 1.0, 'offset': 3.0, 'event_label': 'b'}]
    est = [{'filename': 'f', 'onset': 0.2, 'offset': 0.9, 'event_label': 'a'},
           {'filename': 'f', 'onset': 0.1, 'offset': 0.5, 'event_label': 'b'},
           {'filename': 'f', 'onset': 2.5, 'offset': 2.6, 'event_label': 'a'}]
    m = calibrate.segment_metrics(est, ref, ['f'], labels, n_segments=3)
    # segment 0: tp a, fp b; segment 1: fn a, fn b; segment 2: fp a, fn b
    ov = m['overall']
    assert (ov['Ntp'], ov['Nfp'], ov['Nfn']) == (1, 2, 3)
    assert ov['precision'] == 1 / 3 and ov['recall'] == 1 / 4
    assert ov['f_measure'] == 2 * (1 / 3) * (1 / 4) / (1 / 3 + 1 / 4)
    er = m['error_rate']
    # seg 0: I = 1; seg 1: D = 2; seg 2: S = 1 -> ER = 4 / 4
    assert (er['Nsubs'], er['Ndel'], er['Nins'], er['Nref']) == (1, 2, 1, 4)
    assert er['error_rate'] == 1.0 and er['substitution_rate'] == 0.25
    assert m['class_wise']['f_measure'][1] == 0.0        # Ntp = 0 -> 0.0 by definition here
    c = calibrate.segment_metrics(np.array([[1, 1, 1, 0], [0, 1, 2, 0]]))
    assert c['overall'] == ov and 'error_rate' not in c


@pytest.fixture(scope='module')
def kat(golden_dir):
    g = json.load(open(os.path.join(golden_dir, 'calibrate_kat.json')))
    data = synth.make_calibration_set(g['n_clips'], g['frames'], g['classes'], seed=g['seed'])
    sha = hashlib.sha256(data['framewise'].tobytes() + data['targets'].tobytes()).hexdigest()
    assert sha == g['sha256']
    return g, data


def test_optimizer_reproduces_reference_trajectory(kat):
    g, data = kat
    score, params, record = calibrate.optimize_sed_thresholds(
        data['framewise'], data['targets'], learning_rate=g['learning_rate'], epochs=g['epochs'], step=g['step'],
        max_search=g['max_search'])
    C = g['classes']
    assert len(record) == g['epochs']
    for i, want in enumerate(g['record']):
        assert record[i]['score'] == want['score'], i
        np.testing.assert_allclose(record[i]['thresholds'], want['thresholds'], rtol=0, atol=1e-12)
    assert score == g['final_score']
    # the inert tagging entries stay exactly at their initial value
    assert params['audio_tagging_threshold'] == [0.5] * C
    assert record[g['epochs'] - 1]['thresholds'][:C] == [0.5] * C
    assert params['sed_high_threshold'] == record[g['epochs'] - 1]['thresholds'][C:2 * C]
    assert all(h != 0.3 for h in params['sed_high_threshold']) and all(v != 0.1 for v in params['sed_low_threshold'])
    assert (params['n_smooth'], params['n_salt']) == (10, 10)
    # the dictionary is what events_from_framewise takes
    ev = inference.events_from_framewise(data['framewise'][:1], params)
    assert ev and set(ev[0]) == {'filename', 'onset', 'offset', 'event_label'}
    # the truth's event list gives the same targets
    names = ['clip%d' % n for n in range(g['n_clips'])]
    lst = [{'filename': names[n], 'onset': b / 100.0, 'offset': f / 100.0, 'event_label': inference.LABELS[k]}
           for n, k, b, f in data['events']]
    np.testing.assert_array_equal(calibrate.segment_targets(lst, names, inference.LABELS, 10), data['targets'])


def test_bad_series_raises_on_reached_probe_only():
    """One class, T = 300.  `base`: a run begins at the last frame at the
    initial high threshold.  `spec`: frames 260..297 and 299 are 0.9 and frame
    298 is 0.35, so high probes 1-2 (0.32, 0.34) see one run to the end and
    probes 3-5 (>= 0.36) a run that begins at the last frame; an 0.31 event in
    segment 0 disappears at probe 1 and changes the score there (cnt = 1), so
    probes 3-5 are speculative.  `reached`: without that event probes 1-2 leave
    the score alone and the loop reaches probe 3."""
    T = 300
    targets = np.zeros((1, 3, 1), np.uint8)
    targets[0, 1, 0] = 1
    base = np.full((1, T, 1), 0.05, np.float32)
    base[0, 100:200, 0] = 0.9
    base[0, -1, 0] = 0.31
    with pytest.raises(RuntimeError, match='find_bgn_fin_pairs quirk'):
        calibrate.optimize_sed_thresholds(base, targets, epochs=1)
    spec = np.full((1, T, 1), 0.05, np.float32)
    spec[0, 100:200, 0] = 0.9
    spec[0, 20:60, 0] = 0.31
    spec[0, 260:298, 0] = 0.9
    spec[0, 298, 0] = 0.35
    spec[0, 299, 0] = 0.9
    counts = calibrate.segment_counts(spec, targets, [[0.3], [0.32], [0.34], [0.36]], [[0.1]] * 4)
    assert counts[:, 0].tolist() == [[1, 2, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 1]]
    score, params, record = calibrate.optimize_sed_thresholds(spec, targets, epochs=1)
    assert score == 0.5 and params['sed_high_threshold'][0] != 0.3
    reached = spec.copy()
    reached[0, 20:60, 0] = 0.05
    with pytest.raises(RuntimeError, match='find_bgn_fin_pairs quirk'):
        calibrate.optimize_sed_thresholds(reached, targets, epochs=1)


def test_package_exports_calibration_entry_points():
    import sedx
    for name in ('optimize_sed_thresholds', 'segment_counts', 'segment_metrics', 'segment_targets'):
        assert getattr(sedx, name) is getattr(calibrate, name)
