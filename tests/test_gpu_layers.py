"""Layer-isolated float64 parity of the HIP path over tile, batch, class-count
and sequence-chunk edges.

Every model here takes a [B, 64, T] feature matrix (``sedx_forward_features``),
so T and B are free and no audio frontend is involved (the log-mel front end
alone, waveform -> stage 0: tests/test_gpu_frontend.py); ``sedx_set_capture``
exposes stages 0 and 2-9.  The reference of a step is the oracle's own layer
function in float64 (oracle/layer_refs.py) applied to the GPU's own previous
stage, so one layer's rounding is all that a layer-isolated check measures.

Yardstick (measured against the reference, never against the kernel): for a
step with float64 reference R, e_cpu = max|fp32 oracle step on the same input
- R| and floor = 2^-23 max|R|; the GPU output G must satisfy
max|G - R| <= c max(e_cpu, floor), c = 4 for exact, F(2x2,3x3) and every
non-conv step (fp32 sums of the same length in another order, 1-2 ulp
transcendentals), c = 24 for conv steps under F(4x4,3x3) (that 4 times the
"~6x the direct conv's" of include/sedx.h).  Split-bf16 (x3) conv and linear
steps: max|G - R| <= 2^-15 max(S), S the float64 step on |input|, |folded
weight| and |bias| (products err ~2^-16 relative, include/sedx.h).  Every
check prints ``RATIO`` = max|G - R| / max(e_cpu, floor) before it asserts.

One recorded exception ("Layer yardsticks"): the exact mode's
conv1 steps sum each output as one in-order fp32 fma chain of 9 Cin terms,
the oracle's CPU convolution in blocks, so at Cin = 128 / 256 (blocks 3-4,
stages 5 and 7) e_cpu understates that algorithm's rounding (measured ratios
4.79 and 7.42, spread over every clip, row and column of the channels with
the largest BN scale: first seen at (1, 8) .. (72, 136), stage 7 channels
160 / 235, stage 5 channel 51).  The yardstick of those two steps is
max(e_cpu, e_alg, floor), e_alg the error of a CPU fp32 emulation of that
chain on the same input (``chain_error``), c = 4.  Block 2's conv1 (stage 3,
Cin = 64) keeps max(e_cpu, floor); all three are checked bit for bit
against the emulation at the sampled pixels.

The GRU model is built as the reference's gamma branch (``m(x)`` is
``sedx_forward_features``); the reference's Transformer model has no feature
branch, so its handle is fed through the same C entry point directly.
"""
import ctypes

import numpy as np
import pytest
import torch

import launch_plan as LP
from oracle import layer_refs as R

pytestmark = pytest.mark.gpu

GRU, TRF = R.GRU, R.TRF
SEEDS = {GRU: 0, TRF: 1}
MT_IDS = {GRU: 'gru', TRF: 'trf'}
P16 = (16000, 512, 160, 64, 25, 7000)
P32 = (32000, 1024, 320, 64, 50, 14000)
KEYS = ('framewise_output', 'clipwise_output', 'embedding')
FORMS = [('exact', None), ('x3', None), ('winograd', 0), ('winograd', 1), ('winograd', 2)]
FORM_IDS = ['exact', 'x3', 'wino-f23', 'wino-f43b24', 'wino-f43']
HEAD_FORMS = [('exact', None), ('winograd', 2)]
HEAD_FORM_IDS = ['exact', 'wino-f43']
X3_REL = 2.0 ** -15


def _fid(form):
    return FORM_IDS[FORMS.index(form)]


# ---------------------------------------------------------------------------
# models, forwards, captures
# ---------------------------------------------------------------------------
_MODELS = {}


def _build(mt, form, C):
    from sedx import _lib, models
    if mt == GRU:
        m = models.Cnn_9layers_Gru_FrameAtt(*P32, C, 'gamma')
    else:
        m = models.Cnn_9layers_Transformer_FrameAtt(*P16, C)
    sd = m.state_dict()
    for k, v in R.state(mt, C, SEEDS[mt], torch.float32).items():
        sd[k] = v
    m.load_state_dict(sd, strict=True)
    m = m.to('cuda').eval().set_precision(form[0])
    if form[1] is not None:
        m.set_tuning(_lib.TUNE_WINO_F43, form[1])
    return m


def model(mt, form, C=25):
    if C not in (25, 33):                  # one-off class counts are not kept
        return _build(mt, form, C)
    key = (mt, form, C)
    if key not in _MODELS:
        _MODELS[key] = _build(mt, form, C)
    return _MODELS[key]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def forward(m, mt, x):
    """One forward of features x [B, 64, T] (cuda): the three outputs."""
    if mt == GRU:
        with torch.no_grad():
            return m(x)
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B, _, T = x.shape
    C, T3 = m.classes_num, T // 8
    fw = torch.empty((B, 8 * T3, C), dtype=torch.float32, device=x.device)
    clip = torch.empty((B, C), dtype=torch.float32, device=x.device)
    emb = torch.empty((B, 512, T3), dtype=torch.float32, device=x.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(L.sedx_forward_features(nat.h, _p(x), B, T, _p(fw), _p(clip), _p(emb), None, 0, stream),
               nat.h, 'forward_features')
    return {'framewise_output': fw, 'clipwise_output': clip, 'embedding': emb}


def run(m, mt, x):
    out = forward(m, mt, x)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    m.check_error()
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k
    return out


def capture(m, mt, stage, x):
    from sedx import _lib
    L = _lib.lib()
    nat = m.native(x.device)
    B, _, T = x.shape
    buf = torch.full(R.capture_shape(stage, B, T), float('nan'), dtype=torch.float32, device=x.device)
    _lib.check(L.sedx_set_capture(nat.h, stage, _p(buf), buf.numel() * 4), nat.h, 'set_capture')
    try:
        forward(m, mt, x)
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'set_capture')
    m.check_error()
    a = buf.cpu()
    assert torch.isfinite(a).all(), 'stage %d' % stage
    return R.from_capture(stage, a)


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def feats(B, T):
    return R.features(B, T, seed=1000 + 7 * B + T)


# ---------------------------------------------------------------------------
# references, cached at module scope and shared by the forms
# ---------------------------------------------------------------------------
_BASE, _SD, _TRUNK, _E2E = {}, {}, {}, {}


def sd(mt, C, dtype):
    """State dict of (model, C): the trunk tensors are shared among the class
    counts (synth draws the head last: tests/test_layer_refs_cpu.py)."""
    if (mt, dtype) not in _BASE:
        _BASE[(mt, dtype)] = R.state(mt, 25, SEEDS[mt], dtype)
    if C == 25:
        return _BASE[(mt, dtype)]
    if (mt, C, dtype) not in _SD:
        s = dict(_BASE[(mt, dtype)])
        s.update({k: v for k, v in R.state(mt, C, SEEDS[mt], dtype).items() if k.startswith('att_block.')})
        _SD[(mt, C, dtype)] = s
    return _SD[(mt, C, dtype)]


def trunk(mt, B, T):
    """Stage 9 of the float64 and of the fp32 oracle chain on feats(B, T)."""
    key = (mt, B, T)
    if key not in _TRUNK:
        f = torch.from_numpy(feats(B, T))
        res = []
        with torch.no_grad():
            for dt, xin in ((torch.float64, f.double()), (torch.float32, f)):
                s = sd(mt, 25, dt)
                x = R.step_bn0(s, xin)
                for _, _, fn in R.conv_steps():
                    x = fn(s, x)
                res.append(R.step_seq(s, mt, x))
        _TRUNK[key] = tuple(res)
    return _TRUNK[key]


def e2e_ref(mt, C, B, T):
    """Float64 outputs and the fp32 oracle's own distance from them (the fp32
    chain is O.forward's op sequence: tests/test_layer_refs_cpu.py)."""
    key = (mt, C, B, T)
    if key not in _E2E:
        s64, s32 = trunk(mt, B, T)
        with torch.no_grad():
            r = R.step_head(sd(mt, C, torch.float64), mt, s64)
            f = R.step_head(sd(mt, C, torch.float32), mt, s32)
        _E2E[key] = ({k: r[k].numpy() for k in KEYS}, {k: f[k].numpy() for k in KEYS})
    return _E2E[key]


# ---------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------
def _np(a):
    return np.asarray(a.detach().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


class Checks(object):
    """Collects every comparison of one test, prints each figure, asserts at
    the end (so a failing run still shows every step)."""

    def __init__(self, section, form):
        self.section, self.form, self.bad = section, form, []

    def check(self, step, G, Rf, f32, c=None, abs_bound=None, e_alg=0.0):
        G, Rf, f32 = _np(G), _np(Rf), _np(f32)
        assert G.shape == Rf.shape == f32.shape, (step, G.shape, Rf.shape, f32.shape)
        assert np.isfinite(G).all(), step
        d = np.abs(G - Rf)
        e = float(d.max()) if d.size else 0.0
        e_cpu = float(np.abs(f32 - Rf).max()) if d.size else 0.0
        floor = 2.0 ** -23 * (float(np.abs(Rf).max()) if d.size else 0.0)
        y = max(e_cpu, floor)
        ratio = e / y if y > 0 else (0.0 if e == 0 else float('inf'))
        at = np.unravel_index(int(d.argmax()), d.shape) if d.size else ()
        # a scalar, or one bound per element (the x3 head's per-element S)
        bound = _np(abs_bound) if abs_bound is not None else np.float64(c * max(y, e_alg))
        worst = float((d / bound).max()) if d.size else 0.0
        print('RATIO|%s|%s|%s|%.3f| e=%.3g e_cpu=%.3g floor=%.3g e_alg=%.3g bound=%.3g e/bound=%.3g shape=%s at=%s'
              % (self.section, step, _fid(self.form), ratio, e, e_cpu, floor, e_alg, float(bound.max()), worst,
                 G.shape, tuple(int(i) for i in at)))
        if not (d <= bound).all():
            # where the excess sits: counts over the bound per leading index / last index
            over = np.argwhere(d > bound)
            self.bad.append('%s: max|G-R| %.3g, %.3g of its bound (ratio %.2f) at %s; %d elements over, first %s '
                            'last %s' % (step, e, worst, ratio, at, len(over), over[0].tolist(), over[-1].tolist()))

    def done(self):
        assert not self.bad, '\n'.join(self.bad)


def conv_c(form, nxt):
    """c of the conv step that writes stage ``nxt``: 24 where it runs F(4x4,3x3)."""
    prec, f43 = form
    return 24 if prec == 'winograd' and (f43 == 2 or (f43 == 1 and nxt != 2)) else 4


def e2e_c(form):
    return 24 if form[0] == 'winograd' and form[1] in (1, 2) else 4


def _absbound(s64, nxt, xin):
    if nxt == 2:
        return R.absbound_block1(s64, xin)
    k = {3: 2, 4: 2, 5: 3, 6: 3, 7: 4, 8: 4}[nxt]
    return R.absbound_conv1(s64, k, xin) if nxt % 2 else R.absbound_conv2(s64, k, xin)


def chain_error(s64, nxt, xin, r64, G):
    """The emulated-chain error of an exact-mode conv1 step (stage 3 / 5 / 7;
    e_alg of the yardstick at stages 5 and 7 only): the distance from
    the float64 step of the same convolution summed in fp32 as csrc/conv.hip
    sums it - one in-order fma chain of 9 Cin terms per output
    (R.chain_conv1_fp32), on the same input, at up to 192 sampled pixels and
    every output channel.  The oracle's CPU convolution sums in blocks, so its
    e_cpu is 3-8x below that chain's at Cin = 128 / 256 ("Layer
    yardsticks"); the yardstick of stages 5 and 7 is max(e_cpu, e_alg) with
    the same c = 4.  The bound never looks at the kernel's output; the
    kernel's values at those pixels equal the emulated chain bit for bit."""
    B, _, Tq, Fq = xin.shape
    pix = R.sample_pixels(B, Tq, Fq, 192)
    E = R.chain_conv1_fp32(s64, (nxt + 1) // 2, xin, pix)
    sel = lambda a: a[pix[:, 0], :, pix[:, 1], pix[:, 2]]
    print('  stage %d: kernel vs emulated fp32 chain on %d pixels: max|d| = %.3g, %d of %d values differ'
          % (nxt, len(pix), float((sel(G).double() - E.double()).abs().max()), int((sel(G) != E).sum()),
             E.numel()))
    assert torch.equal(sel(G), E), 'stage %d: the kernel no longer sums as the documented in-order chain' % nxt
    return float((E.double() - sel(r64)).abs().max())


def check_seq_and_head(ck, mt, C, form, s8, s9, outs, tag=''):
    """Stage 8 -> 9 and 9 -> outputs against the float64 steps on the GPU's
    own stage 8 / 9."""
    s64, s32 = sd(mt, C, torch.float64), sd(mt, C, torch.float32)
    x3 = form[0] == 'x3'
    with torch.no_grad():
        r9, f9 = R.step_seq(s64, mt, s8.double()), R.step_seq(s32, mt, s8)
        ck.check(tag + MT_IDS[mt] + '-seq', s9, r9, f9, c=4,
                 abs_bound=X3_REL * R.absbound_seq(s64, mt, s8.double()) if x3 else None)
        rh, fh = R.step_head(s64, mt, s9.double()), R.step_head(s32, mt, s9)
        hb = R.absbound_head(s64, mt, s9.double()) if x3 else None
    for k in KEYS:
        # (the Transformer's embedding is stage 9 transposed: no arithmetic, c = 4 of a zero error)
        ck.check(tag + MT_IDS[mt] + '-head-' + k.split('_')[0], outs[k], rh[k], fh[k], c=4,
                 abs_bound=X3_REL * hb[k] if x3 and hb[k] is not None else None)


# ---------------------------------------------------------------------------
# 3a. the stage chain, layer by layer
# ---------------------------------------------------------------------------
CHAIN_SHAPES = [(1, 8), (3, 37), (2, 135), (2, 527), (8, 64), (16, 136), (72, 136)]


@pytest.mark.parametrize('form', FORMS, ids=FORM_IDS)
@pytest.mark.parametrize('B,T', CHAIN_SHAPES, ids=['B%d-T%d' % s for s in CHAIN_SHAPES])
def test_stage_chain(B, T, form):
    """Stages 0, 2-9 and the outputs, one capture per forward, each step
    against the float64 step on the GPU's own previous stage.  Conv steps on
    the GRU model; the sequence and head steps on both.  (72, 136) runs every
    F(4x4,3x3) launch with item claims."""
    if form == ('winograd', 2) and (B, T) == (72, 136):
        assert [LP.w43_regime(l, B, T, ncu()) for l in range(7)] == ['nt4_claim'] * 7
    ck = Checks('chain', form)
    f = feats(B, T)
    x = torch.from_numpy(f).cuda()
    m = model(GRU, form)
    caps = {st: capture(m, GRU, st, x) for st in R.STAGES}
    outs = run(m, GRU, x)
    s64, s32 = sd(GRU, 25, torch.float64), sd(GRU, 25, torch.float32)
    with torch.no_grad():
        ft = torch.from_numpy(f)
        ck.check('bn0', caps[0], R.step_bn0(s64, ft.double()), R.step_bn0(s32, ft), c=4)
        for prev, nxt, fn in R.conv_steps():
            xin = caps[prev]
            bound, e_alg = None, 0.0
            r64 = fn(s64, xin.double())
            if form[0] == 'x3':
                bound = X3_REL * float(_absbound(s64, nxt, xin.double()).max())
            if form[0] == 'exact' and nxt in (3, 5, 7):
                e_chain = chain_error(s64, nxt, xin, r64, caps[nxt])
                e_alg = e_chain if nxt in (5, 7) else 0.0      # stage 3 meets c = 4 against e_cpu alone
            ck.check('conv-%d' % nxt, caps[nxt], r64, fn(s32, xin), c=conv_c(form, nxt), abs_bound=bound,
                     e_alg=e_alg)
    check_seq_and_head(ck, GRU, 25, form, caps[8], caps[9], outs)
    mt_ = model(TRF, form)
    t8, t9 = capture(mt_, TRF, 8, x), capture(mt_, TRF, 9, x)
    check_seq_and_head(ck, TRF, 25, form, t8, t9, run(mt_, TRF, x))
    ck.done()


# ---------------------------------------------------------------------------
# 3b. exhaustive small-T sweep, end to end
# ---------------------------------------------------------------------------
def _chunks(lst, n):
    return [lst[i:i + n] for i in range(0, len(lst), n)]


def _sweep_groups():
    b3 = lambda ts: [(3, T) for T in ts]
    g = _chunks(b3(range(8, 72)), 8) + _chunks(b3(range(124, 136)), 6) + _chunks(b3(range(252, 264)), 4)
    g += _chunks(b3(range(504, 528)), 3)
    g += _chunks([(1, T) for T in (8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 135, 527)], 6)
    g += _chunks([(B, T) for B in (8, 16) for T in (37, 64, 136, 260)], 2)
    g += [[(72, 64)], [(72, 136)]]
    return g


SWEEP_GROUPS = _sweep_groups()
assert [s for g in SWEEP_GROUPS for s in g] == R.SWEEP_SHAPES
SWEEP_IDS = ['B%d-T%d..B%d-T%d' % (g[0] + g[-1]) for g in SWEEP_GROUPS]


def test_sweep_covers_every_w43_regime():
    """Over the sweep's shapes each of the seven F(4x4,3x3) launches runs in
    every regime it can reach on this device."""
    assert LP.w43_missing(R.SWEEP_SHAPES, ncu()) == []


def test_launch_plan_of_the_device_is_the_plan_of_its_cu_count():
    """sedx_conv_launch_plan asked for the handle's device (ncu 0: the CU
    count the launchers themselves read) answers what it answers for that CU
    count given as a number, the form the CPU tests use; on a 256-CU device
    the three shapes run the regimes tests/test_layer_refs_cpu.py lists."""
    for B, T in ((1, 64), (8, 136), (16, 37)):
        st, rows = LP.conv_launches(B, T, 0)
        assert st == 0 and len(rows) == 7 and all(r['nwg'] > 0 for r in rows)
        assert (st, rows) == LP.conv_launches(B, T, ncu()), (B, T)
    if ncu() == 256:
        assert [LP.w43_regime(l, 1, 64, 0) for l in range(7)] == ['nt1_tg2'] * 3 + ['nt1_tg1'] * 4
        assert LP.w43_regime(3, 8, 136, 0) == 'nt1_tg2' and LP.w43_regime(3, 16, 37, 0) == 'nt1_tg2'


@pytest.mark.parametrize('group', SWEEP_GROUPS, ids=SWEEP_IDS)
@pytest.mark.parametrize('form', FORMS, ids=FORM_IDS)
@pytest.mark.parametrize('mt', [GRU, TRF], ids=['gru', 'trf'])
def test_sweep_end_to_end(mt, form, group):
    """Every T in 8..71, the item-boundary neighbourhoods 124..135, 252..263
    and 504..527, B = 1 / 3 / 8 / 16 / 72: the three outputs against the
    float64 chain, e_cpu from the fp32 oracle forward on the same features
    (x3: the 1e-3 bar)."""
    ck = Checks('sweep', form)
    m = model(mt, form)
    for B, T in group:
        ref, f32 = e2e_ref(mt, 25, B, T)
        outs = run(m, mt, torch.from_numpy(feats(B, T)).cuda())
        for k in KEYS:
            ck.check('%s-%s B%d T%d' % (MT_IDS[mt], k.split('_')[0], B, T), outs[k], ref[k], f32[k],
                     c=e2e_c(form), abs_bound=1e-3 if form[0] == 'x3' else None)
    ck.done()


@pytest.mark.parametrize('mt', [GRU, TRF], ids=['gru', 'trf'])
def test_seven_frames_raise(mt):
    """Fewer than 8 frames leave nothing after the three pools: a loud error."""
    m = model(mt, ('winograd', 2))
    with pytest.raises(RuntimeError):
        forward(m, mt, torch.from_numpy(feats(2, 7)).cuda())
    torch.cuda.synchronize()
    run(m, mt, torch.from_numpy(feats(2, 8)).cuda())      # and the handle still works


# ---------------------------------------------------------------------------
# 3c. class-count and sequence-chunk edges
# ---------------------------------------------------------------------------
def _head_case(mt, form, C, B, T):
    ck = Checks('head', form)
    m = model(mt, form, C)
    x = torch.from_numpy(feats(B, T)).cuda()
    outs = run(m, mt, x)
    T3 = T // 8
    ref, f32 = e2e_ref(mt, C, B, T)
    frames = 8 * T3 if (mt == TRF or 8 * T3 == 1000 or (8 * T3) % 100 == 0) else 8 * T3 + 100 - (8 * T3) % 100
    assert outs['framewise_output'].shape == (B, frames, C) == ref['framewise_output'].shape
    assert outs['clipwise_output'].shape == (B, C)
    assert outs['embedding'].shape == ((B, C, T3) if mt == GRU else (B, 512, T3)) == ref['embedding'].shape
    for k in KEYS:
        ck.check('e2e-%s-%s' % (MT_IDS[mt], k.split('_')[0]), outs[k], ref[k], f32[k], c=4)
    check_seq_and_head(ck, mt, C, form, capture(m, mt, 8, x), capture(m, mt, 9, x), outs)
    ck.done()


@pytest.mark.parametrize('C', [1, 7, 32, 33, 64, 65, 256])
@pytest.mark.parametrize('form', HEAD_FORMS, ids=HEAD_FORM_IDS)
@pytest.mark.parametrize('mt', [GRU, TRF], ids=['gru', 'trf'])
def test_class_counts(mt, form, C):
    """classes_num 1..256: the head projection's 64 -> 128.. rows at C = 33
    and att_head's 32-class slots (c0 > 0), end to end and layer by layer."""
    _head_case(mt, form, C, 3, 8 * 33)


SEQ_LENS = [1, 25, 31, 32, 33, 63, 64, 65, 124, 125, 126, 127, 128, 129, 257]


@pytest.mark.parametrize('n', SEQ_LENS)
@pytest.mark.parametrize('C', [25, 33])
@pytest.mark.parametrize('form', HEAD_FORMS, ids=HEAD_FORM_IDS)
@pytest.mark.parametrize('mt', [GRU, TRF], ids=['gru', 'trf'])
def test_sequence_chunk_edges(mt, form, C, n):
    """Sequence lengths at the MHA's 32-query / 64-key chunks, the GRU model's
    pad-to-100 rule (25: 200 frames, no pad; 125: the 1000-frame exception)
    and att_head's 128-frame staging (127..129, 257)."""
    _head_case(mt, form, C, 2, 8 * n)


# ---------------------------------------------------------------------------
# 3d. the feature-input model at B = 32, T = 994 with item claims
# ---------------------------------------------------------------------------
def test_features_b32_t994_claims():
    """B = 32 x 994 frames on the default Winograd form: blocks 1-3 claim
    their items.  Clips 0, 13, 31 against the float64 chain, and bit for bit
    against the same three clips as a B = 3 batch (static item order)."""
    B, T, form, pick = 32, 994, ('winograd', 2), [0, 13, 31]
    assert [LP.w43_regime(l, B, T, ncu()) for l in range(5)] == ['nt4_claim'] * 5
    assert all(LP.w43_regime(l, 3, T, ncu()) != 'nt4_claim' for l in range(7))
    f = R.features(B, T, seed=994)
    m = model(GRU, form)
    big = run(m, GRU, torch.from_numpy(f).cuda())
    sub = np.ascontiguousarray(f[pick])
    small = run(m, GRU, torch.from_numpy(sub).cuda())
    for k in KEYS:
        assert np.array_equal(big[k][pick], small[k]), k
    ck = Checks('b32t994', form)
    with torch.no_grad():
        ft = torch.from_numpy(sub)
        outs = []
        for dt, xin in ((torch.float64, ft.double()), (torch.float32, ft)):
            s = sd(GRU, 25, dt)
            outs.append(R.chain(s, GRU, R.step_bn0(s, xin)))
    for k in KEYS:
        ck.check('gru-' + k.split('_')[0], big[k][pick], outs[0][k], outs[1][k], c=e2e_c(form))
    ck.done()
