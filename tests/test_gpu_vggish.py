"""HIP path of the three VGGish models: goldens the reference produced
(tools/make_golden_vggish.py) in the three precision modes, the windowed driver
and its events, every conv launch of the trunk in isolation against the tests'
float64 step (tests/vggish_refs.py) on the GPU's own previous capture with the
yardstick of tests/test_gpu_layers.py and its documented summation order bit for
bit, rows dropped by a flooring pool, the launcher's three shapes, the heads'
frame repeat and padding, run / workspace / graph / int16 bit-identity, the
trunk's independence of the precision mode, and the refusals.

Layer yardstick (tests/test_gpu_layers.py unchanged): max|G - R| <=
4 max(e_cpu, e_alg, floor), R the float64 step on the GPU's own previous stage,
e_cpu the fp32 CPU step's distance from R, e_alg that of the CPU fp32 emulation
of the kernel's stated order at the sampled outputs, where the kernel's values
equal the emulation bit for bit.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import test_gpu_layers as TL
import vggish_refs as V
from oracle import sed_oracle as O
from sedx import synth

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the project's bar against the reference (tests/test_gpu_parity.py)
KEYS = V.KEYS
EXACT = ('exact', None)
EINVAL = 1
MODEL_IDS = [V.IDS[mt] for mt in V.MODELS]
PRECS = ['winograd', 'exact', 'x3']
HOP = 160


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


# ---------------------------------------------------------------------------
# models, forwards, captures
# ---------------------------------------------------------------------------
_MODELS, _SD = {}, {}


def build(mt, prec='winograd'):
    from sedx import models
    if mt not in _MODELS:
        m = getattr(models, mt)(*V.ctor_args(None))
        sd = m.state_dict()
        for k, v in synth.make_state_dict(mt, seed=V.SEEDS[mt]).items():
            sd[k] = torch.from_numpy(v)
        m.load_state_dict(sd, strict=True)
        _MODELS[mt] = m.to('cuda').eval()
    return _MODELS[mt].set_precision(prec)


def states(mt):
    if mt not in _SD:
        _SD[mt] = (V.state(mt, torch.float64), V.state(mt, torch.float32))
    return _SD[mt]


def run(m, wave):
    with torch.no_grad():
        out = m(torch.as_tensor(np.asarray(wave)).cuda())
    torch.cuda.synchronize()
    m.check_error()
    assert sorted(out) == sorted(KEYS)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k
    return out


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def forward_features(m, mt, x, ws=None, ws_bytes=0):
    """One forward of features x [B, 64, T] (cuda) through sedx_forward_features; NaN-filled outputs."""
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B, _, T = x.shape
    seq = max(T // 16, 1)
    fw = torch.full((B, 1000, 25), float('nan'), dtype=torch.float32, device=x.device)
    clip = torch.full((B, 25), float('nan'), dtype=torch.float32, device=x.device)
    emb = torch.full((B, 512 if mt == V.AVG else 25, seq), float('nan'), dtype=torch.float32, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(L.sedx_forward_features(nat.h, _p(x), B, T, _p(fw), _p(clip), _p(emb),
                                       _p(ws) if ws is not None else None, ws_bytes, stream), nat.h, 'forward_features')
    return {'framewise_output': fw, 'clipwise_output': clip, 'embedding': emb}


def run_features(m, mt, x, **kw):
    out = forward_features(m, mt, x, **kw)
    torch.cuda.synchronize()
    m.check_error()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k      # every element was written, the pad frames included
    return out


def capture(m, stage, fwd, shape):
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    buf = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(L.sedx_set_capture(nat.h, stage, _p(buf), buf.numel() * 4), nat.h, 'set_capture')
    try:
        fwd()
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'set_capture')
    a = buf.cpu()
    assert torch.isfinite(a).all(), 'stage %d' % stage
    return a


def capture_features(m, mt, stage, x, **kw):
    B, _, T = x.shape
    return capture(m, stage, lambda: forward_features(m, mt, x, **kw), V.capture_shape(stage, B, T))


def feats(B, T):
    return torch.from_numpy(TL.feats(B, T)).cuda()


WAVES = {'short': (2, 10400, 11), 'ragged': (1, 7777, 12), 'odd': (1, 4800, 13)}


def _waves(kind):
    if kind == 'clip10s':
        return synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)[:1]
    b, n, seed = WAVES[kind]
    return synth.make_waveforms(b, seconds=n / 16000., sample_rate=16000, seed=seed)


# ---------------------------------------------------------------------------
# 1. goldens
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['short', 'ragged', 'odd', 'clip10s'])
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_goldens(mt, prec, kind, golden_dir):
    g = np.load(os.path.join(golden_dir, 'vggish_%s.npz' % mt))
    m = build(mt, prec)
    w = _waves(kind)
    out = run(m, w)
    for k in KEYS:
        ref = g['%s_%s' % (kind, k)]
        e = err(out[k], ref)
        print(mt, prec, kind, k, 'max|d| = %.3g' % e)
        assert e <= TOL
    if kind == 'short':
        # stages 53, 55, 8 and 9 within 1e-4 x the stage's scale (test_stage_goldens' rule)
        wc = torch.from_numpy(w).cuda()
        with torch.no_grad():
            for stage in (53, 55, 8, 9):
                a = capture(m, stage, lambda: m(wc), V.capture_shape(stage, 2, 66)).numpy()
                ref = g['short_stage%d' % stage]
                scale = max(1.0, float(np.abs(ref).max()))
                e = err(a, ref)
                print(mt, prec, 'stage', stage, 'max|d| = %.3g (scale %.3g)' % (e, scale))
                assert e <= 1e-4 * scale


# ---------------------------------------------------------------------------
# 2. windowed driver and events
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_windowed_driver_and_events(mt, prec, golden_dir):
    """predict.py driver, 10 s windows at 1 s stride on a 12 s clip: 3 windows of 1000 frames merged to 1200;
    the event lists of both tables."""
    from sedx import inference
    g = np.load(os.path.join(golden_dir, 'vggish_windowed.npz'))['merged_10_1_' + mt]
    ev = json.load(open(os.path.join(golden_dir, 'vggish_events.json')))[mt]
    tables = json.load(open(os.path.join(golden_dir, 'events.json')))
    m = build(mt, prec)
    audio = torch.from_numpy(synth.make_waveforms(1, seconds=12.0, sample_rate=16000, seed=ev['wave_seed'])).cuda()
    merged = inference.predict_windows(m, audio, 10, 1, overlap=True).cpu().numpy()
    assert merged.shape == g.shape == (1, 1200, 25)
    e = err(merged, g)
    print('windowed 10/1', mt, prec, 'max|d| =', e)
    assert e <= TOL
    for which in ('default', 'synthetic'):
        assert inference.events_from_framewise(merged, tables['params_' + which]) == ev[which], which


# ---------------------------------------------------------------------------
# 3. each conv launch in isolation
# ---------------------------------------------------------------------------
LAYER_SHAPES = [(B, T) for T in (16, 17, 31, 35, 61, 66, 130) for B in (1, 3)]


def check_trunk(ck, m, mt, x, tag, n_samples=4):
    """Captures 50-55 and 8 against the float64 step on the GPU's own previous capture; every launch's
    stated order bit for bit at sampled outputs (the last pooled row, bin 0 and the last bin among them)."""
    g64, g32 = states(mt)
    B, _, T = x.shape
    caps = {st: capture_features(m, mt, st, x) for st in V.TRUNK_STAGES}
    assert torch.equal(caps[0], x.cpu().transpose(1, 2))            # the raw log-mel: no bn0
    prev = 0
    for l in range(6):
        stage = V.STAGE_OF[l]
        xin, G = caps[prev], caps[stage]
        with torch.no_grad():
            r64, r32 = V.step_conv(g64, l, xin.double()), V.step_conv(g32, l, xin)
        w, b = V._wb(g32, l)
        s = V.sample_outputs(tuple(G.shape[:3]), n_samples, seed=B + T + l)
        # the last (pooled) row at bin 0 and at the last bin, and the last bin of row 0, are among the samples
        assert {(B - 1, G.shape[1] - 1, 0), (B - 1, G.shape[1] - 1, G.shape[2] - 1), (0, 0, G.shape[2] - 1)} <= \
            set(map(tuple, s.tolist()))
        if l == 0:
            E = V.emulate_conv1(w.numpy(), b.numpy(), xin.numpy(), s)
        else:
            E = V.emulate_conv(w.numpy(), b.numpy(), xin.numpy(), s, 'maxpool' if V.CONVS[l][3] else 'store')
        got = G.numpy()[s[:, 0], s[:, 1], s[:, 2]]
        nd = int((got != E).sum())
        print('  %sstage %d: kernel vs emulated fp32 order on %d outputs x %d channels: %d values differ'
              % (tag, stage, len(s), E.shape[1], nd))
        assert nd == 0, 'stage %d: the kernel no longer sums in the order its header documents' % stage
        e_alg = float(np.abs(E.astype(np.float64) - r64.numpy()[s[:, 0], s[:, 1], s[:, 2]]).max())
        ck.check('%sstage%d' % (tag, stage), G, r64, r32, c=4, e_alg=e_alg)
        prev = stage
    # conv4_2's fused launch: the same pool, then the mean of the 4 pooled bins in the stated order
    G8, x54 = caps[8], caps[54]
    w, b = V._wb(g32, 5)
    with torch.no_grad():
        r64, r32 = V.step_mean(V.step_conv(g64, 5, x54.double())), V.step_mean(V.step_conv(g32, 5, x54))
    s = V.sample_outputs(tuple(G8.shape[:2]), n_samples, seed=B + T)
    E = V.emulate_conv(w.numpy(), b.numpy(), x54.numpy(), s, 'maxpool_fmean')
    assert np.array_equal(G8.numpy()[s[:, 0], s[:, 1]], E), 'stage 8: the fused pool + mean left its documented order'
    p = caps[55].numpy()
    mean = (((p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]) + p[:, :, 3]) * np.float32(0.25)
    assert np.array_equal(G8.numpy(), mean.astype(np.float32)), 'stage 8 is not the ordered mean of stage 55'
    e_alg = float(np.abs(E.astype(np.float64) - r64.numpy()[s[:, 0], s[:, 1]]).max())
    ck.check(tag + 'stage8', G8, r64, r32, c=4, e_alg=e_alg)
    return caps


@pytest.mark.parametrize('B,T', LAYER_SHAPES, ids=['B%d-T%d' % s for s in LAYER_SHAPES])
def test_conv_launches_in_isolation(B, T):
    ck = TL.Checks('vggish', EXACT)
    check_trunk(ck, build(V.ATT), V.ATT, feats(B, T), 'B%d-T%d-' % (B, T))
    ck.done()


# ---------------------------------------------------------------------------
# 4. rows dropped by a flooring pool
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('T', [31, 35])
def test_dropped_rows_never_reach_the_next_layer(T):
    """T = 31 -> 15 -> 7 -> 3 -> 1 and 35 -> 17 -> 8 -> 4 -> 2.  By the receptive field (V.kept_rows, asserted) no
    INPUT row is free at any T: a pool drops the last conv row of a level, and that row's own inputs are
    still the bottom neighbours of the row above it.  So no input row can be overwritten without changing
    stage 55 by conv arithmetic, and the set chosen by the receptive field is empty.  What a dropped row
    could reach the next layer through is the dense buffer: the next layer's bottom halo row is the next
    clip's first row, or whatever lies behind the last clip.  Conv arithmetic says neither can matter, so
    stage 55 of clip 0 must not change when clip 1 is overwritten with large values, and the whole of stage 55
    must not change when the workspace starts as NaN patterns instead of the handle's cache."""
    from sedx import _lib
    assert V.kept_rows(T) == T
    counts = [T, T // 2, T // 4, T // 8]
    assert any(c % 2 for c in counts[:3])                            # a pool floors
    m = build(V.ATT)
    x = feats(2, T)
    base = capture_features(m, V.ATT, 55, x)
    loud = x.clone()
    loud[1] = 1.0e4
    other = capture_features(m, V.ATT, 55, loud)
    assert torch.equal(base[0], other[0]) and not torch.equal(base[1], other[1])
    alone = capture_features(m, V.ATT, 55, x[:1].contiguous())
    assert torch.equal(base[0], alone[0])
    L = _lib.lib()
    nat = m.native(x.device)
    need = ctypes.c_size_t()
    _lib.check(L.sedx_workspace_size(nat.h, 2, (T - 1) * HOP, ctypes.byref(need)), nat.h, 'workspace_size')
    buf = torch.full((need.value + 4096,), 0xFF, dtype=torch.uint8, device='cuda')
    own = capture_features(m, V.ATT, 55, x, ws=buf, ws_bytes=need.value)
    assert torch.equal(base, own)
    assert bool((buf[need.value:] == 0xFF).all())


# ---------------------------------------------------------------------------
# 5. the launcher's shapes
# ---------------------------------------------------------------------------
def test_launch_shapes_on_ten_second_clips():
    """B = 1, 3, 9, 20, 32 (and 6: conv2's 4-wave band is 5 <= B <= 8 on 256 CUs) x 10 s: clips 0-2 are
    bit-identical whatever shape each layer's launch takes; two clips against the fp32 CPU restatement."""
    mt = V.GRU
    m = build(mt)
    x = feats(32, 1001)
    ncu = TL.ncu()
    seen = [set() for _ in range(5)]
    ref = None
    for B in (32, 20, 9, 6, 3, 1):
        for i, (T, F, cout) in enumerate(V.layer_geometry(1001)):
            seen[i].add(V.exact_launch_shape(B, T, F, cout, ncu))
        xb = x[:B].contiguous()
        got = run_features(m, mt, xb)
        got['stage8'] = capture_features(m, mt, 8, xb).numpy()
        if ref is None:
            ref = got
        n = min(B, 3)
        for k in got:
            assert np.array_equal(got[k][:n], ref[k][:n]), (B, k)
    print('launch shapes per layer on %d CUs:' % ncu, seen)
    if ncu == 256:
        assert all(s == {'small', '4-wave', '8-wave'} for s in seen), seen
    g32 = states(mt)[1]
    cpu = V.chain(g32, mt, x[:2].cpu())
    for k in KEYS:
        e = err(ref[k][:2], cpu[k].numpy())
        print('10 s, 2 clips vs the fp32 CPU restatement:', k, 'max|d| = %.3g' % e)
        assert e <= TOL


# ---------------------------------------------------------------------------
# 6. the heads
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', [V.ATT, V.GRU], ids=['att', 'gru'])
def test_att_head_repeats_by_12_and_pads_to_1000(mt):
    ck = TL.Checks('vggish-head', EXACT)
    m = build(mt)
    g64, g32 = states(mt)
    for B, T in ((1, 16), (3, 66), (2, 1001), (1, 1343)):
        seq = T // 16
        x = feats(B, T)
        s8, s9 = capture_features(m, mt, 8, x), capture_features(m, mt, 9, x)
        out = run_features(m, mt, x)
        fw = out['framewise_output']
        assert fw.shape == (B, 1000, 25) and out['embedding'].shape == (B, 25, seq)
        assert np.array_equal(fw[:, :12 * seq], np.repeat(fw[:, 0:12 * seq:12], 12, axis=1))   # frames 12 k .. 12 k + 11
        assert np.array_equal(fw[:, 12 * seq:], np.repeat(fw[:, 12 * seq - 1:12 * seq], 1000 - 12 * seq, axis=1))
        assert np.array_equal(fw[:, 0:12 * seq:12], out['embedding'].transpose(0, 2, 1))
        with torch.no_grad():
            if mt == V.GRU:
                ck.check('B%d-T%d-gru' % (B, T), s9, V.step_seq(g64, mt, s8.double()), V.step_seq(g32, mt, s8), c=4)
            else:
                assert torch.equal(s8, s9)
            rh, fh = V.step_head(g64, mt, s9.double()), V.step_head(g32, mt, s9)
        for k in KEYS:
            ck.check('B%d-T%d-%s' % (B, T, k.split('_')[0]), out[k], rh[k], fh[k], c=4)
    ck.done()


@pytest.mark.parametrize('seq', [1, 3, 4, 62, 84])
def test_frameavg_head_ratio_and_clipwise_mean(seq):
    """ratio = 1000 // seq: 1000, 333 (+1 pad), 250, 16 (+8), 11 (+76); clipwise = the mean over all 1000
    padded frames, against the float64 mean with the yardstick."""
    ck = TL.Checks('vggish-avg', EXACT)
    mt = V.AVG
    m = build(mt)
    g64, g32 = states(mt)
    T = 16 * seq + 9
    B = 2
    x = feats(B, T)
    assert V.geometry(mt, T) == (seq, 1000 // seq)
    rep = 1000 // seq
    s9 = capture_features(m, mt, 9, x)
    assert torch.equal(s9, capture_features(m, mt, 8, x))
    out = run_features(m, mt, x)
    fw = out['framewise_output']
    assert np.array_equal(fw[:, :rep * seq], np.repeat(fw[:, 0:rep * seq:rep], rep, axis=1))
    if rep * seq < 1000:
        assert np.array_equal(fw[:, rep * seq:], np.repeat(fw[:, rep * seq - 1:rep * seq], 1000 - rep * seq, axis=1))
    if seq > 1:
        assert not np.array_equal(fw[:, rep - 1], fw[:, rep])       # the ratio is rep, not more
    assert np.array_equal(out['embedding'], s9.numpy().transpose(0, 2, 1))
    with torch.no_grad():
        rh, fh = V.step_head(g64, mt, s9.double()), V.step_head(g32, mt, s9)
    for k in KEYS:
        ck.check('seq%d-%s' % (seq, k.split('_')[0]), out[k], rh[k], fh[k], c=4)
    # the clipwise output against the float64 mean of the GPU's own 1000 frames
    mean64 = fw.astype(np.float64).mean(axis=1)
    ck.check('seq%d-clipwise-of-frames' % seq, out['clipwise_output'], mean64, fw.mean(axis=1, dtype=np.float32), c=4)
    ck.done()


# ---------------------------------------------------------------------------
# 7. bit-identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_run_workspace_graph_and_int16_identity(mt):
    from sedx import _lib, inference
    m = build(mt)
    x = feats(5, 131)
    a, b = run_features(m, mt, x), run_features(m, mt, x)
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key                   # a second run
    one = run_features(m, mt, x[3:4].contiguous())
    for key in KEYS:
        assert np.array_equal(a[key][3:4], one[key]), key            # alone
    # a caller workspace of exactly sedx_workspace_size bytes, 0xFF-filled inside a larger tensor
    L = _lib.lib()
    nat = m.native(x.device)
    need = ctypes.c_size_t()
    _lib.check(L.sedx_workspace_size(nat.h, 5, 130 * HOP, ctypes.byref(need)), nat.h, 'workspace_size')
    buf = torch.full((need.value + 4096,), 0xFF, dtype=torch.uint8, device='cuda')
    own = run_features(m, mt, x, ws=buf, ws_bytes=need.value)
    for key in KEYS:
        assert np.array_equal(own[key], a[key]), key
    assert bool((buf[need.value:] == 0xFF).all())
    # the HIP-graph path
    w = torch.from_numpy(_waves('short')).cuda()
    with torch.no_grad():
        eager = {k: v.clone() for k, v in m(w).items()}
    out = inference.GraphedForward(m, w)(w)
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(out[key], eager[key]), key
    # sedx_forward_i16 = sedx_forward of the dequantised samples
    q = (np.clip(_waves('short'), -1.0, 1.0) * 32767).astype(np.int16)
    with torch.no_grad():
        o16 = m(torch.from_numpy(q).cuda())
        o32 = m(torch.from_numpy(O.int16_to_float32(q)).cuda())
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(o16[key], o32[key]), key


# ---------------------------------------------------------------------------
# 8. precision: the trunk is fp32 in every mode
# ---------------------------------------------------------------------------
def test_trunk_captures_are_bit_identical_in_every_precision_mode():
    from sedx import _lib
    x = feats(3, 67)
    caps = {}
    for prec in PRECS:
        m = build(V.GRU, prec)
        caps[prec] = {st: capture_features(m, V.GRU, st, x) for st in V.TRUNK_STAGES}
    m = build(V.GRU, 'winograd')
    for knob, value in ((_lib.TUNE_WINO_F43, 0), (_lib.TUNE_WINO_BLOCK1, 0)):
        m.set_tuning(knob, value)
    caps['knobs'] = {st: capture_features(m, V.GRU, st, x) for st in V.TRUNK_STAGES}
    m.set_tuning(_lib.TUNE_WINO_F43, 2).set_tuning(_lib.TUNE_WINO_BLOCK1, 2)
    build(V.GRU, 'winograd')
    for prec in ('winograd', 'x3', 'knobs'):
        for st in V.TRUNK_STAGES:
            assert torch.equal(caps['exact'][st], caps[prec][st]), (prec, st)


# ---------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mt', V.MODELS, ids=MODEL_IDS)
def test_forwards_refuse_what_the_queries_refuse(mt):
    from sedx import _lib
    L = _lib.lib()
    m = build(mt)
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    fr, sl, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_size_t()
    for T in (15, 16, 1343, 1344, 16015, 16016):
        ok = V.geometry(mt, T) is not None
        Ls = (T - 1) * HOP
        assert (L.sedx_output_geometry(nat.h, Ls, ctypes.byref(fr), ctypes.byref(sl)) == 0) == ok, T
        assert (L.sedx_workspace_size(nat.h, 1, Ls, ctypes.byref(nb)) == 0) == ok, T
        if ok:
            assert (fr.value, sl.value) == (1000, T // 16)
            out = run_features(m, mt, feats(1, T))
            assert out['framewise_output'].shape == (1, 1000, 25)
        else:
            assert len(L.sedx_last_error(nat.h)) > 10
            with pytest.raises(RuntimeError):
                forward_features(m, mt, feats(1, T))
            if T < 2000:
                with pytest.raises(RuntimeError):
                    run(m, np.zeros((1, max(Ls, 300)), np.float32))
    torch.cuda.synchronize()
    out = run_features(m, mt, feats(2, 66))                           # and the handle still works
    assert out['framewise_output'].shape == (2, 1000, 25)


def test_a_handle_refuses_another_familys_keys():
    from sedx import models
    m = getattr(models, V.ATT)(*V.ctor_args(None)).to('cuda').eval()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict('Cnn_9layers_FrameAtt', seed=0).items()}
    nat = m.native(torch.device('cuda', torch.cuda.current_device()))
    with pytest.raises(RuntimeError):
        nat.load(sd)
