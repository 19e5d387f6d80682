"""CPU-only checks of the product's host side: the C-ABI library loads and
exports every symbol include/sedx.h declares, the native event extraction
(host C++) matches the reference's vad known answers, and the model classes
keep the reference state_dict contract.  No GPU compute is called."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import sed_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(REPO, 'include', 'sedx.h')).read()
    return sorted(set(re.findall(r'\b(sedx_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    from sedx import _lib
    L = _lib.lib()
    syms = _header_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(_lib.EXPORTS) == syms
    assert b'gfx950' in L.sedx_version()


def test_state_dict_contract():
    from sedx import models
    exp = {'Cnn_9layers_Gru_FrameAtt': (73, 6178336), 'Cnn_9layers_Transformer_FrameAtt': (75, 6047264)}
    for mt, (nk, ne) in exp.items():
        m = getattr(models, mt)(16000, 512, 160, 64, 25, 7000, 25, 'logmel')
        sd = m.state_dict()
        assert len(sd) == nk and sum(v.numel() for v in sd.values()) == ne
        fr = O.frontend_state('16k')
        for k, v in fr.items():
            np.testing.assert_allclose(sd[k].numpy(), v, rtol=2e-6, atol=2e-7)


def test_frontend_construction_matches_reference(golden_dir):
    from sedx import stft
    g = np.load(os.path.join(golden_dir, 'frontend.npz'))
    for q, p in O.PRESETS.items():
        w = stft.mel_weights(p['sample_rate'], p['window_size'], 64, p['fmin'], p['fmax'])
        np.testing.assert_allclose(w, g['melW_' + q], rtol=2e-6, atol=1e-9)


def test_native_events_match_vad_kat(golden_dir):
    from sedx import inference
    kat = json.load(open(os.path.join(golden_dir, 'vad_kat.json')))
    for case in kat:
        if 'x' not in case:
            continue
        x = np.asarray(case['x'], np.float32)[None, :, None]
        params = {'sed_high_threshold': case['thres'], 'sed_low_threshold': case['low_thres'],
                  'n_smooth': case['n_smooth'], 'n_salt': case['n_salt']}
        try:
            got = inference.event_pairs(x, params)[:, 2:].tolist()
        except RuntimeError:
            got = 'raises'
        # the reference is run on float64 arrays here; float32 compare is identical
        # unless a value sits within float32 rounding of a threshold
        assert got == case['pairs'], case


def test_native_events_match_golden_events(golden_dir):
    from sedx import inference
    ev = json.load(open(os.path.join(golden_dir, 'events.json')))
    for mt in ('Cnn_9layers_Gru_FrameAtt', 'Cnn_9layers_Transformer_FrameAtt'):
        merged = np.load(os.path.join(golden_dir, 'windowed_%s.npz' % mt))['merged_5_1']
        for which in ('default', 'synthetic'):
            got = inference.events_from_framewise(merged, ev['params_' + which])
            assert got == ev[mt][which]


def test_native_events_match_long_file_goldens(golden_dir):
    """Host C++ events over the reference's long-file merges (183 / 131
    windows, 18,700 / 7,100 frames; oracle/make_golden_long.py)."""
    from sedx import inference
    ev = json.load(open(os.path.join(golden_dir, 'long_events.json')))
    for case, c in ev['cases'].items():
        g = np.load(os.path.join(golden_dir, 'long_%s.npz' % case))
        for mt in ('Cnn_9layers_Gru_FrameAtt', 'Cnn_9layers_Transformer_FrameAtt'):
            for which in ('default', 'synthetic'):
                got = inference.events_from_framewise(g[mt], ev['params_' + which])
                assert got == c[mt][which], (case, mt, which)


def test_events_random_vs_oracle():
    from sedx import inference
    rng = np.random.default_rng(3)
    for _ in range(20):
        fw = rng.uniform(0, 1, (2, 200, 25)).astype(np.float32)
        fw = np.cumsum(fw - 0.5, axis=1) / 8 + 0.5
        fw = fw.astype(np.float32)
        params = {'sed_high_threshold': rng.uniform(0.4, 0.7, 25).tolist(),
                  'sed_low_threshold': rng.uniform(0.1, 0.4, 25).tolist(),
                  'n_smooth': int(rng.integers(0, 12)), 'n_salt': int(rng.integers(0, 12))}
        try:
            got = inference.events_from_framewise(fw, params)
        except RuntimeError:
            with pytest.raises(IndexError):
                O.events_from_framewise(fw, params)
            continue
        assert got == O.events_from_framewise(fw, params)


def test_window_geometry_host_rules():
    # loop control of predict.py:297-338 on the oracle side
    assert O.window_starts(10.0, 5, 1) == [0, 1, 2, 3, 4, 5]
    assert len(O.window_starts(10.0, 6, 0.5)) == 9
    assert O.window_starts(3.0, 5, 1) == [0]


DRIVER_CASES = [  # (driver, overlap, sample_duration, overlap_value, seconds)
    ('predict', True, 5, 1.0, 10.0), ('predict', True, 5, 0.5, 23.0), ('predict', False, 5, 1.0, 23.0),
    ('predict', False, 5, 0.7, 17.3), ('predict', True, 6, 0.5, 71.3), ('predict', True, 5, 1.0, 187.37),
    ('predict', True, 5, 1.0, 3.2), ('main_strong', True, 5, 0.7, 10.0), ('main_strong', True, 6, 0.9, 10.0),
    ('main_strong', True, 7, 1.3, 10.0), ('main_strong', True, 5, 0.1, 10.0), ('main_strong', True, 5, 0.3, 9.9),
    ('main_strong', True, 5, 1.0, 12.3), ('main_strong', True, 6, 0.5, 8.7), ('main_strong', True, 7, 0.9, 14.1)]


@pytest.mark.parametrize('driver,overlap,sd,ov,secs', DRIVER_CASES)
def test_native_window_starts_match_reference_loops(driver, overlap, sd, ov, secs):
    """sedx_window_starts (host C++, no GPU) against the reference's loop
    control restated in the oracle: predict.py:297-338 strides 1 s with
    --overlap, else sample_duration; main_strong.py:790-832 strides
    overlap_value (float64 running start) over the clip padded to 10 s and
    feeds windows past 10 s shorter."""
    from sedx import inference
    L = int(round(secs * 16000))
    starts, lens = inference.window_starts(16000, L, sd, ov, driver, overlap)
    ref = O.window_starts(L / 16000., sd, O.driver_stride(driver, sd, ov, overlap))
    assert starts == [int(s * 16000) for s in ref]
    for s, n in zip(starts, lens):
        want = sd * 16000 if driver == 'predict' else max(0, min(s + sd * 16000, 160000) - s)
        assert n == want


def _ref_merge_all(wins, sd, ov, avg):
    merged = wins[0].copy()
    for k in range(2, len(wins) + 1):
        merged = O.merge(merged if k > 2 else wins[0], wins[k - 1], sd, k, ov)
    return O.avg_merge(merged, sd, ov) if avg else merged


@pytest.mark.parametrize('seed', range(40))
def test_native_merge_matches_numpy_merge(seed):
    """sedx_merge_host (the host plan the GPU merge runs by) against
    utilities.merge / avg_merge (restated in the oracle, numpy semantics) on
    random windows, bit for bit: random window counts and lengths (incl.
    ragged last windows), steps below / at / above the window length
    (numpy's clamped slicing concatenates; broadcasting of a 1-frame
    operand), float and zero steps; where numpy raises, sedx raises."""
    from sedx import inference
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 12))
    tw = int(rng.choice([1, 2, 40, 96, 100, 296, 400, 496, 500]))
    frames = [tw] * n
    if rng.random() < 0.4:                     # shorter trailing windows (main_strong past 10 s)
        for j in range(int(rng.integers(1, 3))):
            frames[-1 - j % n] = int(rng.integers(1, tw + 1))
    sd = int(rng.integers(1, 8))
    ov = float(rng.choice([0.5, 0.7, 0.9, 1.0, 1.3, 1.4, 1.9, 2.0, 3.0, 4.99, 5.0, 6.0, 10.0, 0.004, -0.5]))
    avg = bool(rng.random() < 0.7)
    C = 3
    wins = [rng.uniform(0, 1, (1, f, C)).astype(np.float32) for f in frames]
    try:
        ref = _ref_merge_all(wins, sd, ov, avg)
    except ValueError:
        with pytest.raises(ValueError):
            inference.merge_host(wins, sd, ov, avg)
        return
    got = inference.merge_host(wins, sd, ov, avg)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got, ref.astype(np.float32))


def test_native_merge_float_overlap_steps():
    """int(100 * overlap_value) in float64: 70 / 90 / 130 / 140 / 190
    frames (a float32 overlap_value would give 69 / 89 / ...)."""
    from sedx import inference
    for ov, step in ((0.7, 70), (0.9, 90), (1.3, 130), (1.4, 140), (1.9, 190)):
        assert int(100 * ov) == step
        wins = [np.ones((1, 500, 1), np.float32)] * 3
        got = inference.merge_host(wins, 5, ov, avg=False)
        assert got.shape[1] == 500 + 2 * step


def _create_handle(L, model_type):
    import ctypes
    from sedx import _lib
    cfg = _lib.SedxConfig(model_type, 0, 16000, 512, 160, 64, 50.0, 7000.0, 25)
    h = ctypes.c_void_p()
    assert L.sedx_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    return h


def test_workspace_sizes_against_the_recorded_grid(golden_dir):
    """sedx_workspace_size, sedx_output_geometry and sedx_window_workspace_size
    (no GPU) over the grid tools/make_golden_workspace.py recorded from the
    library before the model table: 16 models x 3 precisions x
    SEDX_TUNE_WINO_BLOCK1 x SEDX_TUNE_WINO_F43 x 5 (clips, samples), and one
    window spec per model.  Sizes and geometry are equal; where a model refuses
    a pair, both queries' statuses are."""
    import ctypes
    from sedx import _lib
    g = json.load(open(os.path.join(golden_dir, 'workspace_sizes.json')))
    assert len(g['models']) == 16 and len(g['rows']) == 16 * 3 * 3 * 3 * 5 and len(g['window_bytes']) == 16
    L = _lib.lib()
    handles = {}
    for mt, prec, b1, f43, B, n, *want in g['rows']:
        h = handles.get(mt) or handles.setdefault(mt, _create_handle(L, mt))
        assert L.sedx_set_precision(h, prec) == 0
        assert L.sedx_set_tuning(h, _lib.TUNE_WINO_BLOCK1, b1) == 0 and L.sedx_set_tuning(h, _lib.TUNE_WINO_F43, f43) == 0
        wsz, fr, sl = ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_int64()
        st = [L.sedx_workspace_size(h, B, n, ctypes.byref(wsz)), L.sedx_output_geometry(h, n, ctypes.byref(fr), ctypes.byref(sl))]
        got = [wsz.value, fr.value, sl.value] if st == [0, 0] else ['refused'] + st
        assert got == want, (mt, prec, b1, f43, B, n, got, want)
    assert sorted(handles) == g['models']
    w = g['window']
    spec = _lib.window_spec(w['sample_duration'], w['overlap_value'])
    for mt, want in zip(g['models'], g['window_bytes']):
        h = _create_handle(L, mt)                     # default tuning, as recorded
        wsz = ctypes.c_size_t()
        assert L.sedx_window_workspace_size(h, w['n_clips'], w['samples'], ctypes.byref(spec), ctypes.byref(wsz)) == 0
        assert wsz.value == want, (mt, wsz.value, want)
        L.sedx_destroy(h)
    for h in handles.values():
        L.sedx_destroy(h)


def test_model_shapes_against_the_recorded_answers(golden_dir):
    """What every model type answers about shapes (no GPU), against what
    tools/make_golden_model_shapes.py recorded from the library before the
    model table: for every T of 1 .. 1400 and both sides of each large limit,
    the status and (frames, seq) of sedx_output_geometry, the status of
    sedx_workspace_size, the status and row count of sedx_gemm_launch_plan and
    the sedx_last_error text of every refusal, all equal; the GEMM rows
    themselves at two shapes in two precision modes, equal; and
    sedx_window_geometry for four window specs: status and answers equal, the
    message compared by the substrings other tests assert on it (the one
    reason is now worded once: "window N: <the forward's reason>")."""
    import importlib.util
    from sedx import _lib
    spec = importlib.util.spec_from_file_location('make_golden_model_shapes',
                                                  os.path.join(REPO, 'tools', 'make_golden_model_shapes.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g = json.load(open(os.path.join(golden_dir, 'model_shapes.json')))
    assert (g['t_range'], g['large'], g['gemm_points'], g['ncu']) == (tool.T_RANGE, [list(p) for p in tool.LARGE],
                                                                    [list(p) for p in tool.GEMM_POINTS], tool.NCU)
    assert g['windows'] == [list(w) for w in tool.WINDOWS] and sorted(map(int, g['models'])) == tool.MODELS
    assert os.path.getsize(os.path.join(golden_dir, 'model_shapes.json')) < os.path.getsize(
        os.path.join(golden_dir, 'vad_kat.json'))
    L = _lib.lib()
    pts = tool.points()
    refusing_window = 0
    for mt in tool.MODELS:
        want = g['models'][str(mt)]
        h = tool.create(L, mt)
        cols = {name: tool.unrle(runs) for name, runs in want['columns'].items()}
        assert all(len(c) == len(pts) for c in cols.values()) and sorted(cols) == sorted(tool.COLUMNS)
        for i, (B, T) in enumerate(pts):
            got = tool.point(L, h, B, T)
            assert got == [cols[name][i] for name in tool.COLUMNS], (mt, B, T, got)
        assert tool.gemm_section(L, h) == want['gemm'], mt
        for w, rec in zip(tool.WINDOWS, want['windows']):
            got = tool.window(L, h, *w)
            assert got[0] == rec[0] and got[2:] == rec[2:], (mt, w, got, rec)
            assert (got[1] == '') == (rec[1] == '')
            for key in ('multiple of 32', 'x12', '1000', '5000', 'reflect padding'):
                assert (key in got[1]) == (key in rec[1]), (mt, w, key, got[1], rec[1])
            # too few frames for the trunk's pools: "too short", or the VGGish trunk's wording of it
            assert ('too short' in rec[1]) == ('too short' in got[1] or 'pooling stages need 16' in got[1]), (mt, w, got[1])
            refusing_window += rec[0] != 0
        L.sedx_destroy(h)
    assert refusing_window >= len(tool.MODELS)          # every model has a window spec it refuses


def test_conv_launch_plan_against_the_recorded_launches(golden_dir):
    """sedx_conv_launch_plan (no GPU) equals, field by field, what the conv
    launchers decided before the decisions moved into the plan
    (tools/make_golden_conv_launches.py, recorded from an instrumented build
    of that commit): default tuning at 256 CUs over the GPU sweep's shapes, the
    bench shapes and two batches that split stage 2; SEDX_TUNE_WINO_F43 x
    _BLOCK1 x _ORDER at 256 CUs and the default at 64 and 304 CUs over 16
    shapes.  Launches of the exact launcher (block 1 with
    SEDX_TUNE_WINO_BLOCK1 0) were not recorded: their rows carry the layer only."""
    import launch_plan as LP
    from sedx import _lib
    g = json.load(open(os.path.join(golden_dir, 'conv_launches.json')))
    assert len(g['cases']) == 143 + 27 * 16 + 2 * 16
    for b1, f43, order, ncu, B, T, ids in g['cases']:
        st, rows = LP.conv_launches(B, T, ncu, [(_lib.TUNE_WINO_BLOCK1, b1), (_lib.TUNE_WINO_F43, f43),
                                                (_lib.TUNE_WINO_ORDER, order)])
        assert st == 0
        exact = [r for r in rows if r['family'] == _lib.CONV_FAMILY['exact']]
        assert [r['stage'] for r in exact] == ([2] if b1 == 0 else []) and all(r['nwg'] == 0 for r in exact)
        got = [[r[c] for c in g['columns']] for r in rows if r not in exact]
        assert got == [g['rows'][i] for i in ids], (b1, f43, order, ncu, B, T)


def test_conv_launch_plan_refusals():
    """A shape the forward refuses (no frame left after the third pool) and a
    row buffer that is too small are SEDX_EINVAL; the latter still reports the
    row count."""
    import ctypes
    import launch_plan as LP
    from sedx import _lib
    assert LP.conv_launches(2, 7, 256)[0] == 1                       # T3 = 0
    st, rows = LP.conv_launches(2, 8, 256)
    assert st == 0 and len(rows) == 7
    st, rows = LP.conv_launches(2, 8, 256, capacity=6)
    assert st == 1 and len(rows) == 6
    n = ctypes.c_int32()
    assert _lib.lib().sedx_conv_launch_plan(LP._h(), 200, 1000 * 160, 256, None, 0, ctypes.byref(n)) == 1
    assert n.value == 8                                              # stage 2 splits under F(4x4)'s byte limit
    assert b'capacity' in _lib.lib().sedx_last_error(LP._h())


GEMM_MS = (1, 128, 256, 257, 896, 897, 1280, 1281, 1408)


def _gemm_rule(M, K, N, act, ncu):
    """The fp32 GEMM launcher's rule, restated: (kernel, grid_x, grid_y)."""
    up = lambda a, b: (a + b - 1) // b
    if N <= 64 and act == 0 and K % 256 == 0 and N % 32 == 0:      # the head projection, every M
        return 'ksplit', up(M, 32), N // 32
    if up(M, 128) * (N // 64) < ncu and K % 64 == 0 and N % 32 == 0:   # the 128 x 64 tiles leave CUs empty
        return 'one_wave', up(M, 32), N // 32
    return 'tiled', up(M, 128), N // 64


def test_gemm_launch_plan_is_the_restated_rule():
    """sedx_gemm_launch_plan (no GPU) equals, field by field, the launcher's
    rule written out above, at 256 CUs (and 64, 304) for M at both sides of
    every switch between the one-wave and the tiled kernel, on the two 14-layer
    handles and a 9-layer one; M = B clips of one sequence frame, and the same
    M as B / 32 clips of 32 sequence frames."""
    import launch_plan as LP
    gemms = {LP.GRU14: [(9, 2048, 6144, 0), (10, 2048, 64, 0)],
             LP.TRF14: [(9, 2048, 1536, 0), (9, 512, 2048, 1), (10, 2048, 64, 0)],
             LP.GRU9: [(9, 512, 1536, 0), (10, 512, 64, 0)]}
    for mt, want in gemms.items():
        t1 = 8 if mt == LP.GRU9 else 32                     # frames of one sequence frame
        for ncu in (256, 64, 304):
            for M in GEMM_MS:
                shapes = [(M, t1)] + ([(M // 32, 32 * t1)] if M % 32 == 0 else [])
                for B, T in shapes:
                    st, rows, n = LP.gemm_launches(mt, B, T, ncu)
                    assert st == 0 and n == len(rows) == len(want), (mt, B, T, st, n)
                    for r, (stage, K, N, act) in zip(rows, want):
                        kern, gx, gy = _gemm_rule(M, K, N, act, ncu)
                        assert r == {'stage': stage, 'M': M, 'K': K, 'N': N, 'act': act, 'kernel': kern,
                                     'grid_x': gx, 'grid_y': gy}, (mt, B, T, ncu, r)


def test_gemm_kernel_thresholds_at_256_cus():
    """Where the tiled kernel takes over on a 256-CU device, as literals: the
    14-layer GRU projection (N = 6144) from M = 257, the 14-layer Transformer's
    q|k|v projection (N = 1536) from 1281 and its fc (N = 2048) from 897, the
    9-layer projections (K = 512, N = 1536) from 1281; the head projection is
    the K-split kernel at every M."""
    import launch_plan as LP
    first_tiled = {(LP.GRU14, 'gru-proj'): 257, (LP.TRF14, 'mha-qkv'): 1281, (LP.TRF14, 'mha-fc'): 897,
                   (LP.GRU9, 'gru-proj'): 1281}
    for (mt, name), m0 in first_tiled.items():
        t1 = 8 if mt == LP.GRU9 else 32
        for M in GEMM_MS + (m0 - 1, m0, 2048):
            k = LP.gemm_kernels(mt, M, t1, 256)
            assert k[name] == ('tiled' if M >= m0 else 'one_wave'), (mt, name, M, k)
            assert k['head'] == 'ksplit'
    # a batch of 32 ten-second clips (T5 = 31, M = 992)
    assert LP.gemm_kernels(LP.GRU14, 32, 1001, 256) == {'gru-proj': 'tiled', 'head': 'ksplit'}
    assert LP.gemm_kernels(LP.TRF14, 32, 1001, 256) == {'mha-qkv': 'one_wave', 'mha-fc': 'tiled', 'head': 'ksplit'}
    assert LP.gemm_reachable(LP.GRU14, 256) == {('gru-proj', 'one_wave'), ('gru-proj', 'tiled'), ('head', 'ksplit')}
    assert LP.gemm_reachable(LP.TRF14, 256) == {('mha-qkv', 'one_wave'), ('mha-qkv', 'tiled'), ('mha-fc', 'one_wave'),
                                                ('mha-fc', 'tiled'), ('head', 'ksplit')}


def test_gemm_launch_plan_answers_for_every_model_family():
    """One row per GEMM launch of the sequence layer and head of every model
    type, in launch order; the split-bf16 and Conformer launchers' rows carry
    the GEMM only."""
    import launch_plan as LP
    # model type -> (stage, K, N, act) rows at 25 classes
    proj, fc, att, fch = (9, 512, 1536, 0), (9, 512, 512, 1), (10, 512, 64, 0), (10, 512, 64, 0)
    cf_block = [(9, 144, 576, 0), (9, 576, 144, 0), (9, 144, 432, 0), (9, 144, 144, 0), (9, 144, 288, 0),
                (9, 144, 144, 0), (9, 144, 576, 0), (9, 576, 144, 0)]
    cf = [(9, 144, 144, 0)] * 3 + [(9, 512, 144, 0)] + cf_block * 3 + [(10, 144, 64, 0)]
    want = {0: [proj, att], 1: [proj, fc, att], 2: [fch], 3: [fch], 4: [att], 5: [proj, fch], 6: [proj, fc, fch],
            7: cf, 8: cf, 10: [(9, 2048, 6144, 0), (10, 2048, 64, 0)],
            11: [(9, 2048, 1536, 0), (9, 512, 2048, 1), (10, 2048, 64, 0)], 13: [(10, 2048, 64, 0)]}
    B, T = 3, 65                                            # T3 = 8, T5 = 2; not a multiple of 32 (model 13)
    for mt, gemms in want.items():
        M = B * (2 if mt >= 10 else 8)
        for prec in ('winograd', 'x3'):
            st, rows, n = LP.gemm_launches(mt, B, T, 256, precision=prec)
            assert st == 0 and n == len(rows) == len(gemms), (mt, prec, st, n)
            assert [(r['stage'], r['K'], r['N'], r['act']) for r in rows] == gemms, (mt, prec)
            for i, r in enumerate(rows):
                m_row = 8 if mt in (7, 8) and i < 3 else M          # r_net runs on one clip's positions
                kern = 'conformer' if mt in (7, 8) else 'x3' if prec == 'x3' and mt < 7 else \
                    _gemm_rule(M, r['K'], r['N'], r['act'], 256)[0]
                assert r['M'] == m_row and r['kernel'] == kern, (mt, prec, r)
                assert (r['grid_x'] > 0) == (kern in ('tiled', 'one_wave', 'ksplit')), (mt, prec, r)


def test_gemm_launch_plan_refusals():
    """The conv query's contract: a shape the forward refuses and a row buffer
    that is too small are SEDX_EINVAL, the latter still reporting the row count."""
    import ctypes
    import launch_plan as LP
    from sedx import _lib
    assert LP.gemm_launches(LP.TRF14, 2, 31, 256)[0] == 1            # T5 = 0
    assert LP.gemm_launches(LP.GRU9, 2, 7, 256)[0] == 1              # T3 = 0
    st, rows, n = LP.gemm_launches(LP.TRF14, 2, 32, 256, capacity=2)
    assert (st, len(rows), n) == (1, 2, 3)
    assert b'capacity' in _lib.lib().sedx_last_error(LP.gemm_handle(LP.TRF14))
    assert LP.gemm_launches(LP.TRF14, 2, 32, 256, capacity=0)[::2] == (1, 3)
    L, h, k = _lib.lib(), LP.gemm_handle(LP.TRF14), ctypes.c_int32()
    assert L.sedx_gemm_launch_plan(h, 0, 31 * 160, 256, None, 0, ctypes.byref(k)) == 1    # no clip
    assert L.sedx_gemm_launch_plan(h, 2, 31 * 160, 256, None, 4, ctypes.byref(k)) == 1    # capacity without rows
    assert L.sedx_gemm_launch_plan(h, 2, 31 * 160, 256, None, 0, None) == 1
    assert L.sedx_gemm_launch_plan(None, 2, 31 * 160, 256, None, 0, ctypes.byref(k)) == 1


def test_invalid_setter_values_are_einval_before_any_device_call():
    """sedx_set_pipelined / sedx_set_profiling range-check `on` before they
    touch HIP: without a GPU an invalid value is SEDX_EINVAL (1), not the
    SEDX_EHIP (3) of a failed event creation."""
    from sedx import _lib
    L = _lib.lib()
    h = _create_handle(L, 0)
    assert L.sedx_set_pipelined(h, 3) == 1 and L.sedx_set_pipelined(h, -1) == 1
    assert L.sedx_set_profiling(h, 3) == 1 and L.sedx_set_profiling(h, -1) == 1
    assert L.sedx_set_pipelined(h, 0) == 0 and L.sedx_set_profiling(h, 0) == 0
    L.sedx_destroy(h)


def test_no_packed_fp32_in_any_kernel():
    """Every kernel's gfx950 ISA is free of packed FP32 VALU (v_pk_add/mul/
    fma_f32): measured on MI355X, packed FP32 beside MFMA waves on the same
    SIMD returns wrong values (tools/fe_race.cpp; sedx_internal.h "packed
    FP32").  `make isa-check` compiles each .hip with the library's flags
    (-fno-slp-vectorize -fno-vectorize) and greps the assembly."""
    import shutil
    import subprocess
    if shutil.which('/opt/rocm/bin/hipcc') is None:
        pytest.skip('needs hipcc')
    pkg = os.path.join(REPO, 'sound-event-detection_amd')
    r = subprocess.run(['make', '-s', '-C', pkg, '-j8', 'isa-check'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'no packed FP32 VALU' in r.stdout


def test_dataparallel_replicas_reuse_the_source_handle(monkeypatch):
    """torch.nn.DataParallel (pytorch/predict.py:239) re-replicates the model on
    every forward, each replica holding freshly broadcast parameter copies
    (new data_ptrs).  The handle cache is shared with the replicas and keyed
    on the SOURCE module's parameters, so a replica does not re-pack the
    weights (no sedx_load_param); an in-place update of the source does."""
    import copy
    import io
    from sedx import models, synth

    loads = []

    class FakeNative(object):          # stands in for the libsedx handle (no GPU here)
        def __init__(self, cfg, idx):
            self.device_index, self.signature, self.precision, self.h = idx, None, 'winograd', None

        def load(self, sd):
            loads.append(len(sd))

    monkeypatch.setattr(models, '_Native', FakeNative)
    mt = 'Cnn_9layers_Gru_FrameAtt'
    m = getattr(models, mt)(16000, 512, 160, 64, 25, 7000, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd)
    m.eval()
    dev = torch.device('cuda', 0)
    m.native(dev)
    assert len(loads) == 1
    m.native(dev)
    assert len(loads) == 1
    def replicate(mod):
        """torch.nn.parallel.replicate for one device without a GPU: every
        module replicated, parameters and buffers broadcast copies (same
        values, new storage)"""
        r = mod._replicate_for_data_parallel()
        r._parameters = {k: (p.detach().clone() if p is not None else None) for k, p in mod._parameters.items()}
        r._buffers = {k: (b.clone() if b is not None else None) for k, b in mod._buffers.items()}
        r._modules = {k: replicate(c) for k, c in mod._modules.items()}
        return r

    for _ in range(3):                 # one replica per DataParallel call
        r = replicate(m)
        assert r._natives is m._natives and r._weights_source() is m
        assert r._signature() != m._signature()
        assert r.native(dev) is m._natives[0]
    assert len(loads) == 1
    with torch.no_grad():
        m.conv_block2.conv1.weight.mul_(1.0)   # in-place update of the source
    replicate(m).native(dev)
    assert len(loads) == 2
    # copies / pickles start with their own empty cache
    c = copy.deepcopy(m)
    assert isinstance(c._natives, models._HandleCache) and len(c._natives) == 0
    assert c._weights_source() is c
    buf = io.BytesIO()
    torch.save(m, buf)


def test_weights_signature_follows_every_change(monkeypatch):
    """The packed weights of a handle are re-made after any change the forward
    must see, and only then: the per-call check (models._SedModel._signature)
    re-walks the state_dict only after a parameter / buffer / submodule was
    registered anywhere, and otherwise re-reads the cached tensors' storage
    and version — so an in-place update, a `.data` swap, a replaced Parameter
    and a new buffer each re-pack once, and a plain repeat does not."""
    import torch
    from sedx import models

    loads = []

    class FakeNative(object):          # stands in for the libsedx handle (no GPU here)
        def __init__(self, cfg, idx):
            self.device_index, self.signature, self.precision, self.h = idx, None, 'winograd', None

        def load(self, sd):
            loads.append(sorted(sd))

    monkeypatch.setattr(models, '_Native', FakeNative)
    m = models.Cnn_9layers_Gru_FrameAtt(16000, 512, 160, 64, 25, 7000, 25, 'logmel').eval()
    dev = torch.device('cuda', 0)

    def packs():
        m.native(dev)
        return len(loads)

    assert packs() == 1 and packs() == 1
    with torch.no_grad():
        m.conv_block3.conv2.weight.mul_(0.5)               # in place: version counter
    assert packs() == 2 and packs() == 2
    m.bn0.weight.data = m.bn0.weight.data.clone()         # new storage, no registration
    assert packs() == 3
    m.att_block.cla.bias = torch.nn.Parameter(torch.zeros(25))   # replaced Parameter (registration hook)
    assert packs() == 4 and packs() == 4
    m.bn0.register_buffer('extra', torch.zeros(1))        # new state_dict key
    assert packs() == 5 and 'bn0.extra' in loads[-1]
    m.load_state_dict(m.state_dict())                      # copy_ into every tensor
    assert packs() == 6 and packs() == 6


def test_python_tuning_constants_match_the_header():
    """The ctypes mirror's knob numbers (sedx/_lib.py) and bench.py's GRU
    kernel table are the values include/sedx.h declares (a drifted number
    would silently A/B the wrong implementation)."""
    import re
    from sedx import _lib
    import bench
    hdr = open(os.path.join(REPO, 'include', 'sedx.h')).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r'\b(SEDX_[A-Z0-9_]+)\s*=\s*(\d+)', hdr)}
    for name in ('GRU_KERNEL', 'GRU_HANDOFF', 'WINO_BLOCK1', 'MEL_MFMA', 'GRU_SPIN', 'WINO_ORDER', 'GAMMA_SPEC'):
        assert getattr(_lib, 'TUNE_' + name) == enum['SEDX_TUNE_' + name], name
    for key, name in (('coop', 'COOP'), ('simple', 'SIMPLE'), ('tag16', 'TAG16'), ('tag8', 'TAG8'),
                      ('coop16', 'COOP16'), ('auto', 'AUTO'), ('ksplit', 'KSPLIT')):
        assert bench.GRU_KERNELS[key] == enum['SEDX_GRU_KERNEL_' + name], key
