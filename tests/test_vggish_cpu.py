"""The three VGGish models without a GPU: the classes and their state_dicts
against the reference's (tests/golden/vggish_meta.json), the checkpoint load
with its ``None`` extension and ``freeze``, the ABI (model ids 15-17, 14 still
unknown), the key sets a handle takes and what finalize names when a key is
missing, the geometry with its refusals from every query, the tests' own
float64 restatement (tests/vggish_refs.py) against the reference's tensors, the
emulations of the kernels' documented orders against torch, and the host side
under ASan + UBSan (tests/native/vggish_driver.cpp: plan, workspace regions,
the packer's round trip, refusals)."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import vggish_refs as V
from sedx import _lib, models, synth

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sound-event-detection_amd')
OK, EINVAL, EKEY = 0, 1, 5
MODEL_IDS = [V.IDS[mt] for mt in V.MODELS]
HOP = 160


def build(mt, ckpt=None, **kw):
    return getattr(models, mt)(*V.ctor_args(ckpt, **kw))


def config(mid, feature=0, classes=25):
    cfg = _lib.SedxConfig()
    cfg.model_type, cfg.feature_type = mid, feature
    cfg.sample_rate, cfg.window_size, cfg.hop_size, cfg.mel_bins = V.P16[:4]
    cfg.fmin, cfg.fmax, cfg.classes_num = float(V.P16[4]), float(V.P16[5]), classes
    return cfg


def create(mid, **kw):
    h = ctypes.c_void_p()
    st = _lib.lib().sedx_create(ctypes.byref(config(mid, **kw)), 0, ctypes.byref(h))
    return st, h


def load(h, key, arr):
    a = np.ascontiguousarray(arr, np.float32)
    shape = (ctypes.c_int64 * a.ndim)(*a.shape)
    return _lib.lib().sedx_load_param(h, key.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim)


@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_class_mirrors_the_reference_state_dict(mt, golden_dir):
    meta = json.load(open(os.path.join(golden_dir, 'vggish_meta.json')))
    m = build(mt)
    sd = m.state_dict()
    got = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in sd.items()]
    assert got == meta[mt]['keys']
    entries, elements = (30, 5975130) if mt == V.AVG else (37, 5988056)
    assert len(sd) == meta[mt]['entries'] == entries
    assert sum(v.numel() for v in sd.values()) == meta[mt]['elements'] == elements
    assert models.MODEL_IDS[mt] == V.MODEL_ID[mt] and mt in models.__all__
    assert [k for k in sd if k.startswith('vggish.')] == ['vggish.0.%d.%s' % (i, s) for i in (0, 3, 6, 8, 11, 13)
                                                          for s in ('weight', 'bias')]
    # 25 outputs whatever classes_num says; feature_type is ignored
    other = getattr(models, mt)(*V.P16, 10, 'gamma', None)
    assert other.classes_num == 25 and other.feature_type == 'logmel'
    assert [tuple(v.shape) for v in other.state_dict().values()] == [tuple(v.shape) for v in sd.values()]
    assert meta['weight_seeds'] == synth.VGGISH_GOLDEN_SEEDS and meta['windowed'][mt]['threshold_margin'] >= 1e-4
    with pytest.raises(TypeError):
        getattr(models, mt)(*V.P16, 25, 'logmel')                    # checkpoint_path is positional, as in the reference


def test_checkpoint_load_the_none_extension_and_freeze(tmp_path):
    """``checkpoint_path`` holds a full ``VGGish().state_dict()``: ``features.*``
    land in ``vggish.0.*``, ``fc.*`` is dropped.  (The container's 290 MB ``fc``
    stack is replaced by small tensors under the same keys: the load reads keys.)"""
    feats = models._vggish_features()
    g = torch.Generator().manual_seed(3)
    ck = {'features.' + k: torch.randn(v.shape, generator=g) for k, v in feats.state_dict().items()}
    assert sorted(ck) == sorted('features.%d.%s' % (i, s) for i in (0, 3, 6, 8, 11, 13) for s in ('weight', 'bias'))
    for i in (0, 2, 4):
        ck['fc.%d.weight' % i], ck['fc.%d.bias' % i] = torch.zeros(2, 2), torch.zeros(2)
    path = str(tmp_path / 'vggish.pth')
    torch.save(ck, path)
    for mt in V.MODELS:
        m = build(mt, path)
        sd = m.state_dict()
        for k, v in ck.items():
            if k.startswith('features.'):
                assert torch.equal(sd['vggish.0.' + k[len('features.'):]], v), k
        assert not any(k.startswith(('vggish.fc', 'vggish.1', 'fc.0')) for k in sd)
        assert m.checkpoint_path == path and m.freeze is False
        assert all(p.requires_grad for p in m.vggish.parameters())
        fz = build(mt, path, freeze=True)
        assert not any(p.requires_grad for p in fz.vggish.parameters())
        assert all(p.requires_grad for n, p in fz.named_parameters()
                   if n.startswith(('gru.', 'att_block.', 'fc.', 'bn0.')))
        assert torch.equal(fz.state_dict()['vggish.0.13.bias'], ck['features.13.bias'])
    # a checkpoint without a trunk key is refused, as VGGish().load_state_dict refuses it
    bad = dict(ck)
    del bad['features.8.bias']
    torch.save(bad, path)
    with pytest.raises(RuntimeError):
        build(V.ATT, path)
    # None: no load (the extension); a missing file raises as torch.load does
    assert build(V.ATT, None).checkpoint_path is None
    with pytest.raises(Exception):
        build(V.ATT, str(tmp_path / 'absent.pth'))


@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_strict_load_of_the_synth_weights_and_refusal_of_a_9_layer_key_set(mt):
    m = build(mt)
    sd = m.state_dict()
    w = synth.make_state_dict(mt, seed=V.SEEDS[mt])
    assert set(sd) - set(w) == {'spectrogram_extractor.stft.conv_real.weight',
                                'spectrogram_extractor.stft.conv_imag.weight', 'logmel_extractor.melW'}
    assert [k for k in sd if k in w] == list(w)                      # the reference's order
    for k, v in w.items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    nine = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict('Cnn_9layers_FrameAtt', seed=0).items()}
    with pytest.raises(RuntimeError):
        m.load_state_dict(nine, strict=True)
    # classes_num does not reach the draws; the three models' trunks differ by seed only
    assert all(np.array_equal(v, synth.make_state_dict(mt, classes_num=7, seed=V.SEEDS[mt])[k]) for k, v in w.items())
    assert float(np.abs(w['vggish.0.0.weight']).max()) <= 1 / 80.0
    assert float(np.abs(w['vggish.0.13.weight']).max()) <= np.sqrt(6.0 / (9 * 512)) + 1e-7


def test_abi_enum_values():
    hdr = open(os.path.join(os.path.dirname(PKG), 'include', 'sedx.h')).read()
    assert '#define SEDX_ABI_VERSION 6' in hdr
    for name, mid in (('SEDX_MODEL_VGGISH_FRAMEATT', 15), ('SEDX_MODEL_VGGISH_GRU_FRAMEATT', 16),
                      ('SEDX_MODEL_VGGISH_FRAMEAVG', 17)):
        assert '%s = %d' % (name, mid) in hdr
    L = _lib.lib()
    assert L.sedx_abi_version() == 6
    cases = [((15,), {}, OK), ((16,), {}, OK), ((17,), {}, OK), ((14,), {}, EINVAL), ((18,), {}, EINVAL),
             ((15,), dict(feature=1), EINVAL), ((16,), dict(feature=1), EINVAL), ((17,), dict(feature=1), EINVAL),
             ((15,), dict(classes=256), OK), ((15,), dict(classes=257), EINVAL)]
    for a, kw, want in cases:
        st, h = create(*a, **kw)
        assert st == want, (a, kw)
        if h:
            L.sedx_destroy(h)


@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_key_sets_and_finalize_names_a_missing_key(mt):
    L = _lib.lib()
    st, h = create(V.MODEL_ID[mt])
    assert st == OK
    try:
        sd = {k: v.numpy() for k, v in build(mt).state_dict().items() if not k.endswith('num_batches_tracked')}
        # gru.* : read by the GRU model (shape checked), accepted and dropped by the other two
        assert load(h, 'gru.weight_ih_l0', sd['gru.weight_ih_l0']) == OK
        assert load(h, 'gru.weight_ih_l0', np.zeros((768, 256))) == (EKEY if mt == V.GRU else OK)
        assert load(h, 'bn0.running_mean', sd['bn0.running_mean']) == OK
        # another family's keys, and a trunk weight of another shape
        for k, shape in (('conv_block1.conv1.weight', (64, 1, 3, 3)), ('conv_block4.bn2.weight', (512,)),
                         ('multihead.fc.weight', (512, 512)), ('fc1.weight', (2048, 2048)),
                         ('encoder.input_layer.0.weight', (144, 512)), ('vggish.0.1.weight', (64,)),
                         ('vggish.fc.0.weight', (4096, 12288)), ('vggish.0.3.weight', (128, 64, 1, 1)),
                         ('fc.weight' if mt != V.AVG else 'att_block.att.weight', (25, 512) if mt != V.AVG else (25, 512, 1))):
            assert load(h, k, np.zeros(shape)) == EKEY, k
            assert k.encode() in L.sedx_last_error(h)
        missing = 'vggish.0.11.bias'
        for k, v in sd.items():
            if k != missing:
                assert load(h, k, v) == OK, k
        assert L.sedx_finalize_weights(h) == EKEY                    # host-side check: no device needed
        assert missing.encode() in L.sedx_last_error(h)
    finally:
        L.sedx_destroy(h)
    if mt == V.GRU:                                                  # the GRU model requires its gru.* keys
        st, h = create(16)
        try:
            for k, v in sd.items():
                if k != 'gru.bias_hh_l0_reverse':
                    assert load(h, k, v) == OK, k
            assert L.sedx_finalize_weights(h) == EKEY and b'gru.bias_hh_l0_reverse' in L.sedx_last_error(h)
        finally:
            L.sedx_destroy(h)


def test_geometry_closed_form():
    for mt in V.MODELS:
        for T in list(range(1, 1400)) + [16015, 16016, 16031, 16032, 20000]:
            t = T
            for _ in range(4):
                t //= 2
            top = 1000 if mt == V.AVG else 83
            assert V.geometry(mt, T) == (None if t < 1 or t > top else (T // 16, 1000 // t if mt == V.AVG else 12)), (mt, T)
    assert V.geometry(V.ATT, 1001) == (62, 12) and V.geometry(V.AVG, 1001) == (62, 16)
    assert V.geometry(V.ATT, 1343) == (83, 12) and V.geometry(V.ATT, 1344) is None and V.geometry(V.AVG, 1344) == (84, 11)
    assert V.geometry(V.AVG, 16015) == (1000, 1) and V.geometry(V.AVG, 16016) is None
    # by the receptive field every input row reaches stage 55: a flooring pool drops conv rows, never input rows
    assert [V.kept_rows(T) for T in (16, 17, 31, 35, 61, 66, 130)] == [16, 17, 31, 35, 61, 66, 130]


# T = 15, 16, 1343, 1344 and seq_len 1000, 1001: (T, refused by the FrameAtt models, refused by FrameAvg, reason)
EDGES = [(15, True, True, b'16'), (16, False, False, None), (1343, False, False, None), (1344, True, False, b'x12'),
         (16015, True, False, b'x12'), (16016, True, True, b'1000')]


@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_every_query_refuses_the_same_shapes_with_a_reason(mt):
    L = _lib.lib()
    st, h = create(V.MODEL_ID[mt])
    assert st == OK
    fr, sl, nb, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t(), ctypes.c_int32()
    crow, grow = (_lib.SedxConvLaunch * 8)(), (_lib.SedxGemmLaunch * 8)()
    try:
        for T, r_att, r_avg, why in EDGES:
            refused = r_avg if mt == V.AVG else r_att
            if mt == V.AVG and T == 16016:
                why = b'1000'
            Ls = (T - 1) * HOP + 7                                   # T = L // hop + 1
            sts = [L.sedx_output_geometry(h, Ls, ctypes.byref(fr), ctypes.byref(sl)),
                   L.sedx_workspace_size(h, 2, Ls, ctypes.byref(nb)),
                   L.sedx_conv_launch_plan(h, 2, Ls, 256, crow, 8, ctypes.byref(n))]
            msgs = [L.sedx_last_error(h)]
            sts.append(L.sedx_gemm_launch_plan(h, 2, Ls, 256, grow, 8, ctypes.byref(n)))
            msgs.append(L.sedx_last_error(h))
            if refused:
                assert sts == [EINVAL] * 4, (T, sts)
                assert all((b'16' if T < 16 else why) in m for m in msgs), (T, msgs)
            else:
                assert sts == [OK] * 4, (T, sts, L.sedx_last_error(h))
                assert (sl.value, fr.value) == (V.geometry(mt, T)[0], 1000) and nb.value > 0
        # the windowed drivers: 14 s windows are 1401 frames, 87 sequence frames
        nw, ws, mf = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        for sd_s, refused in ((10, False), (14, mt != V.AVG)):
            spec = _lib.window_spec(sd_s, 1.0)
            st = L.sedx_window_geometry(h, 16 * 16000, ctypes.byref(spec), ctypes.byref(nw), ctypes.byref(ws), ctypes.byref(mf))
            st2 = L.sedx_window_workspace_size(h, 1, 16 * 16000, ctypes.byref(spec), ctypes.byref(nb))
            assert (st, st2) == ((EINVAL, EINVAL) if refused else (OK, OK)), (sd_s, st, st2)
            if refused:
                assert b'x12' in L.sedx_last_error(h)
        spec = _lib.window_spec(10, 1.0)
        assert L.sedx_window_geometry(h, 12 * 16000, ctypes.byref(spec), ctypes.byref(nw), ctypes.byref(ws), ctypes.byref(mf)) == OK
        assert (nw.value, mf.value) == (3, 1200)
    finally:
        L.sedx_destroy(h)


@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_conv_launch_plan_rows(mt):
    """Five rows, stages 2-6, the exact family in every precision mode, epi 3 / 0 / 3 / 0 / 4; the other
    fields as on the exact launcher's rows (zero)."""
    L = _lib.lib()
    st, h = create(V.MODEL_ID[mt])
    rows, n = (_lib.SedxConvLaunch * 8)(), ctypes.c_int32()
    try:
        for prec in (0, 1, 2):
            assert L.sedx_set_precision(h, prec) == OK
            for knob in (_lib.TUNE_WINO_F43, _lib.TUNE_WINO_BLOCK1):
                assert L.sedx_set_tuning(h, knob, 1) == OK
            assert L.sedx_conv_launch_plan(h, 3, 1000 * HOP, 256, rows, 8, ctypes.byref(n)) == OK and n.value == 5
            got = [(r.stage, r.family, r.T, r.F, r.cin, r.cout, r.epi) for r in rows[:5]]
            assert got == [(2, 0, 500, 32, 64, 128, 3), (3, 0, 250, 16, 128, 256, 0), (4, 0, 250, 16, 256, 256, 3),
                           (5, 0, 125, 8, 256, 512, 0), (6, 0, 125, 8, 512, 512, 4)], (prec, got)
            assert all((r.clips, r.tg, r.nt, r.c4, r.nitems, r.nwg, r.claim, r.order2d, r.clips_per_launch) == (0,) * 9
                       for r in rows[:5])
    finally:
        L.sedx_destroy(h)


def test_cpu_tensors_and_train_mode_raise():
    m = build(V.AVG)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16000))                 # train mode
    m.eval()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16000))                 # a CPU tensor: no fallback


@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_float64_restatement_reproduces_the_references_tensors(mt, golden_dir):
    """vggish_refs' float64 steps on the golden's own stage 53 give its stages 55,
    8, 9 and the three outputs to <= 1e-5: the restatement the GPU tests measure
    against is the reference's arithmetic.  (Stage 53 itself needs the log-mel,
    which is the frontend's: the GPU goldens cover it.)"""
    g = np.load(os.path.join(golden_dir, 'vggish_%s.npz' % mt))
    sd = V.state(mt, torch.float64)
    with torch.no_grad():
        s53 = torch.from_numpy(g['short_stage53']).double()
        s55 = V.step_conv(sd, 5, V.step_conv(sd, 4, s53))
        s8 = V.step_mean(s55)
        s9 = V.step_seq(sd, mt, s8)
        out = V.step_head(sd, mt, s9)
    for what, a, b in (('stage55', s55, g['short_stage55']), ('stage8', s8, g['short_stage8']), ('stage9', s9, g['short_stage9']),
                       ('framewise', out['framewise_output'], g['short_framewise_output']),
                       ('clipwise', out['clipwise_output'], g['short_clipwise_output']),
                       ('embedding', out['embedding'], g['short_embedding'])):
        e = float(np.abs(a.numpy() - b.astype(np.float64)).max())
        print(mt, what, 'max|d| = %.3g' % e)
        assert a.shape == b.shape and e <= 1e-5, what
    # activations stay O(1) on the unnormalised log-mel; spread outputs
    for k in ('short_stage53', 'short_stage55', 'short_stage8'):
        assert 0.5 < float(np.abs(g[k]).max()) < 4.0, k
    for kind, seq in (('short', 4), ('ragged', 3), ('odd', 1), ('clip10s', 62)):
        fw = g[kind + '_framewise_output']
        rep = 1000 // seq if mt == V.AVG else 12
        assert fw.shape[1:] == (1000, 25) and g[kind + '_embedding'].shape[2] == seq
        assert np.array_equal(fw[:, :rep * seq], np.repeat(fw[:, 0:rep * seq:rep], rep, axis=1))
        assert np.array_equal(fw[:, rep * seq:], np.repeat(fw[:, rep * seq - 1:rep * seq], 1000 - rep * seq, axis=1))


def test_emulated_orders_match_torch_in_fp32():
    rng = np.random.default_rng(7)
    sd = V.state(V.ATT, torch.float32)
    x0 = (-40.0 + 20.0 * rng.standard_normal((2, 19, 64))).astype(np.float32)
    with torch.no_grad():
        caps = V.trunk({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, torch.from_numpy(x0).double())
    w, b = V._wb(sd, 0)
    s = V.sample_outputs((2, 9, 32), 12, seed=1)
    assert {(0, 8, 0), (1, 8, 31), (0, 0, 31), (1, 8, 0)} <= set(map(tuple, s.tolist()))     # last pooled row, bin 0, last bin
    e = V.emulate_conv1(w.numpy(), b.numpy(), x0, s)
    ref = caps[50].numpy()[s[:, 0], s[:, 1], s[:, 2]]
    assert float(np.abs(e - ref).max()) <= 16 * 2.0 ** -23 * max(1.0, float(np.abs(ref).max()))
    prev = caps[50].float().numpy()
    for l, stage in ((1, 51), (2, 52)):
        w, b = V._wb(sd, l)
        shape = caps[stage].shape[:3]
        s = V.sample_outputs(shape, 6, seed=l)
        e = V.emulate_conv(w.numpy(), b.numpy(), prev, s, V.EPI_OF[l])
        with torch.no_grad():
            ref = V.step_conv({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, l,
                              torch.from_numpy(prev).double()).numpy()[s[:, 0], s[:, 1], s[:, 2]]
        assert float(np.abs(e - ref).max()) <= 64 * 2.0 ** -23 * max(1.0, float(np.abs(ref).max())), l
        prev = caps[stage].float().numpy()
    # the 4-bin mean's order
    x = rng.standard_normal((1, 4, 8, 4)).astype(np.float32)
    wm = np.zeros((4, 4, 3, 3), np.float32)
    wm[np.arange(4), np.arange(4), 1, 1] = 1.0                       # the identity conv
    got = V.emulate_conv(wm, np.zeros(4, np.float32), x, np.array([[0, 1]]), 'maxpool_fmean')
    p = np.maximum(x, 0)[0, 2:4].reshape(2, 4, 2, 4).max(axis=(0, 2))  # pooled [4 bins, 4 ch]
    want = (((p[0] + p[1]) + p[2]) + p[3]) * np.float32(0.25)
    assert np.array_equal(got[0], want.astype(np.float32))


def test_launch_shape_coverage_of_the_gpu_batches():
    """The batches of the GPU launch-shape test reach every launcher shape at every layer on 256 CUs
    (conv2's 4-wave band is 5 <= B <= 8, hence B = 6 beside the five sizes 1, 3, 9, 20, 32)."""
    seen = [set() for _ in range(5)]
    for B in (1, 3, 6, 9, 20, 32):
        for i, (T, F, cout) in enumerate(V.layer_geometry(1001)):
            seen[i].add(V.exact_launch_shape(B, T, F, cout, 256))
    assert all(s == {'small', '4-wave', '8-wave'} for s in seen), seen
    assert V.exact_launch_shape(8, 500, 32, 128, 256) == '4-wave' and V.exact_launch_shape(9, 500, 32, 128, 256) == '8-wave'
    assert V.exact_launch_shape(20, 125, 8, 512, 256) == '4-wave' and V.exact_launch_shape(32, 125, 8, 512, 256) == '8-wave'


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_side_under_sanitizers():
    r = subprocess.run(['make', '-s', '-C', PKG, 'asan-vggish'], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert 'vggish_driver: clean' in out and 'ERROR: AddressSanitizer' not in out and 'runtime error' not in out, out[-4000:]
