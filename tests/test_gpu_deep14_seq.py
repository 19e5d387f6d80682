"""The sequence layer and head of the two 14-layer models at long sequences
and large batches: the fp32 GEMM launcher's tiled kernel at K = 2048 (and the
switch from the one-wave kernel to it), gru1024's second clip block over many
recurrent steps, the MHA's query / key chunks and att_head's x32 repeat past
its 128-frame staging chunk.

Everything runs ``sedx_forward_features`` on [B, 64, 32 T5] features in the
default precision form (the sequence layer and head are fp32 in every mode).
Each step is compared with its float64 step (tests/deep14_refs.py) on the
GPU's own previous stage, 43 -> 9 and 9 -> outputs, as
tests/test_gpu_deep14.py's ``check_layers`` does; the deep conv emulation is
not repeated here.  Yardstick of tests/test_gpu_layers.py, unchanged:
max|G - R| <= 4 max(e_cpu, 2^-23 max|R|), printed as ``RATIO`` before it is
asserted.  One recorded exception ("Layer yardsticks"): the GRU
model's 43 -> 9 step sums each input-projection output as one in-order
2048-term fp32 chain, the oracle's CPU GEMM in blocks, so e_cpu understates
that order's rounding (ratios 2.7 .. 4.08 from T5 = 7 on, the same hidden units
worst at every length); its yardstick is max(e_cpu, e_alg, floor), e_alg the
error of a CPU fp32 emulation of the documented order on the same input
(``gru_order_error``), c = 4, and the kernel lies within the plain yardstick
of that emulation.  Which kernel a GEMM launch ran is read from
``sedx_gemm_launch_plan`` (tests/launch_plan.py), the plan function the
launcher itself calls.
"""
import numpy as np
import pytest
import torch

import deep14_refs as D
import launch_plan as LP
import test_gpu_deep14 as T14
import test_gpu_layers as TL

pytestmark = pytest.mark.gpu

KEYS = D.KEYS
MT = {D.GRU14: LP.GRU14, D.TRF14: LP.TRF14}          # sedx_model_type of the query's handles

SEQ_LENS = [1, 2, 7, 25, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
RAGGED_LENS = (32, 129)                              # T = 32 T5 + 31 as well
SWITCH_SHAPES = [(2, 128), (1, 257), (3, 128), (3, 129)]
BATCHES = [32, 33, 41]
BATCH_T5 = 32
# every (model, B, T) the tests below run
SHAPES = [(mt, 2, 32 * n) for mt in T14.MODELS for n in SEQ_LENS] + \
         [(mt, 2, 32 * n + 31) for mt in T14.MODELS for n in RAGGED_LENS] + \
         [(D.GRU14, B, 32 * n) for B, n in SWITCH_SHAPES] + [(D.GRU14, 1, 32 * 128)] + \
         [(mt, B, 32 * BATCH_T5) for mt in T14.MODELS for B in BATCHES + [2, 3]]


def kernels(mt, B, T):
    """{launch: kernel} of a forward of [B, 64, T] on this device."""
    return LP.gemm_kernels(MT[mt], B, T, 0)


def forwards(mt, x):
    """Stage 43, stage 9 and the three outputs of features x [B, 64, T]."""
    m = T14.build(mt)
    return T14.capture_features(m, 43, x), T14.capture_features(m, 9, x), T14.run_features(m, x)


ORDER_FRAMES = 16       # frames per direction of the emulated GRU order


def gru_order_error(s64, tag, s43, s9, r9, f9):
    """e_alg of the GRU model's 43 -> 9 step: the distance from the float64 step
    of a CPU fp32 emulation of the order the library sums in (one in-order
    2048-term chain per projection output, four 256-term chains per recurrent
    product: D.emulate_gru14), on the same input, for the middle clip's first
    (forward direction) and last (reverse) ORDER_FRAMES frames.  The oracle's
    CPU GEMM sums in blocks, so its e_cpu understates that order's rounding
    ("Layer yardsticks").  The bound never looks at the kernel's
    output.  The kernel itself must lie within the plain yardstick,
    4 max(e_cpu, floor), of the emulation: what separates the two is the
    device's exp / tanh alone."""
    clip = s43.shape[0] // 2
    fwd, rev = D.emulate_gru14(s64, s43, clip, ORDER_FRAMES)
    n = fwd.shape[0]
    sel = lambda a: torch.cat([a[clip, :n, :1024], a[clip, a.shape[1] - n:, 1024:]]).double()
    E, R = torch.cat([fwd, rev]).double(), sel(r9)
    e_alg = float((E - R).abs().max())
    e_cpu, floor = float((sel(f9) - R).abs().max()), 2.0 ** -23 * float(R.abs().max())
    d = float((sel(s9) - E).abs().max())
    print('ORDER|%s| kernel vs emulated order on %d values: max|d| = %.3g; e_alg = %.3g, e_cpu = %.3g, floor = %.3g '
          'there' % (tag, E.numel(), d, e_alg, e_cpu, floor))
    assert d <= 4 * max(e_cpu, floor), '%s: the kernel is %.3g from its documented order' % (tag, d)
    return e_alg


def check_steps(ck, mt, tag, s43, s9, outs):
    """43 -> 9 and 9 -> outputs against the float64 steps on the GPU's own stage
    43 / 9; the GRU's 43 -> 9 against max(e_cpu, e_alg, floor) (gru_order_error)."""
    s64, s32 = T14.states(mt)
    with torch.no_grad():
        r9, f9 = D.step_seq(s64, mt, s43.double()), D.step_seq(s32, mt, s43)
        e_alg = gru_order_error(s64, tag, s43, s9, r9, f9) if mt == D.GRU14 else 0.0
        ck.check(tag + '-seq', s9, r9, f9, c=4, e_alg=e_alg)
        rh, fh = D.step_head(s64, mt, s9.double()), D.step_head(s32, mt, s9)
    for key in KEYS:
        assert outs[key].shape == tuple(rh[key].shape), (tag, key)
        ck.check(tag + '-head-' + key.split('_')[0], outs[key], rh[key], fh[key], c=4)


def check_shape(ck, mt, B, T):
    """One forward shape: shapes by D.geometry, the pad rows, both steps."""
    T5, frames = D.geometry(T)
    s43, s9, outs = forwards(mt, T14.feats(B, T))
    assert tuple(s43.shape) == (B, 2048, T5) and tuple(s9.shape) == (B, T5, 2048)
    fw = outs['framewise_output']
    assert fw.shape == (B, frames, 25) and outs['clipwise_output'].shape == (B, 25)
    assert outs['embedding'].shape == ((B, 25, T5) if mt == D.GRU14 else (B, 2048, T5))
    # frames past 32 T5 repeat the last real one
    assert frames >= 32 * T5 and np.array_equal(fw[:, 32 * T5:], np.repeat(fw[:, 32 * T5 - 1:32 * T5], frames - 32 * T5, 1))
    check_steps(ck, mt, '%s-B%d-T%d' % (T14.IDS[mt], B, T), s43, s9, outs)
    return s9, outs


# ---------------------------------------------------------------------------
# 1. sequence lengths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', SEQ_LENS)
@pytest.mark.parametrize('mt', T14.MODELS, ids=T14.MODEL_IDS)
def test_sequence_lengths(mt, n):
    """B = 2 at T5 = n: the MHA's 32-query / 64-key chunks (31..33, 63..65,
    127..129, 257), att_head's 128-frame staging chunk on both sides and its
    third chunk (257: 8224 framewise frames by the x32 repeat), up to 256
    recurrent steps of gru1024, and the pad rule (25: 800 frames, no pad; every
    other length pads to the next 100).  T = 32 n + 31 has the same T5 after
    five floor halvings."""
    ck = TL.Checks('deep14-seqlen', T14.WINO)
    assert D.geometry(32 * n)[1] == (800 if n == 25 else 32 * n + 100 - (32 * n) % 100)
    check_shape(ck, mt, 2, 32 * n)
    if n in RAGGED_LENS:
        assert D.geometry(32 * n + 31) == D.geometry(32 * n)
        check_shape(ck, mt, 2, 32 * n + 31)
    ck.done()


# ---------------------------------------------------------------------------
# 2. the switch between the two GEMM kernels at K = 2048, N = 6144
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,n', SWITCH_SHAPES, ids=['B%d-T5_%d' % s for s in SWITCH_SHAPES])
def test_gemm_kernel_switch(B, n):
    """Cnn_14layers_Gru_FrameAtt's input projection at M = 256, 257, 384, 387.
    On 256 CUs: the last M of the one-wave kernel, then the tiled kernel with
    one valid row in its third tile, with three exact tiles, and with a fourth
    tile of three rows.  At (3, 128) every clip equals, bit for bit, the same
    clip alone (M = 128: the one-wave kernel): the two kernels give identical
    bits at K = 2048."""
    mt, T = D.GRU14, 32 * n
    if TL.ncu() == 256:
        st, rows, _ = LP.gemm_launches(LP.GRU14, B, T, 0)
        assert st == 0 and (rows[0]['M'], rows[0]['K'], rows[0]['N']) == (B * n, 2048, 6144)
        assert (rows[0]['kernel'], rows[0]['grid_x']) == {256: ('one_wave', 8), 257: ('tiled', 3), 384: ('tiled', 3),
                                                          387: ('tiled', 4)}[B * n]
    ck = TL.Checks('deep14-switch', T14.WINO)
    s9, outs = check_shape(ck, mt, B, T)
    ck.done()
    if (B, n) == (3, 128):
        if TL.ncu() == 256:
            assert kernels(mt, 1, T)['gru-proj'] == 'one_wave'
        x, m = T14.feats(B, T), T14.build(mt)
        for i in range(B):
            xi = x[i:i + 1].contiguous()
            assert torch.equal(T14.capture_features(m, 9, xi), s9[i:i + 1]), i
            one = T14.run_features(m, xi)
            for key in KEYS:
                assert np.array_equal(one[key], outs[key][i:i + 1]), (i, key)


# ---------------------------------------------------------------------------
# 3. large batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('mt', T14.MODELS, ids=T14.MODEL_IDS)
def test_large_batches(mt, B):
    """T5 = 32 at B = 32, 33, 41 (M = 1024, 1056, 1312).  On 256 CUs the GRU
    projection and the Transformer's fc run the tiled kernel at all three, its
    q|k|v projection only at 41; gru1024 runs a full clip block, a second block
    of one clip and one of nine over 31 recurrent MFMA steps.  Clips 0, 31 and
    B - 1 against float64 (both steps are per clip: the references run on those
    rows of the captured stage 43 / 9), and bit for bit against the same clips
    as one small batch in another order."""
    T = 32 * BATCH_T5
    pick = sorted({0, 31, B - 1})
    if TL.ncu() == 256:
        want = {'gru-proj': 'tiled', 'head': 'ksplit'} if mt == D.GRU14 else \
            {'mha-qkv': 'tiled' if B == 41 else 'one_wave', 'mha-fc': 'tiled', 'head': 'ksplit'}
        assert kernels(mt, B, T) == want
        assert 'tiled' not in kernels(mt, len(pick), T).values()
    x = T14.feats(B, T)
    s43, s9, outs = forwards(mt, x)
    ck = TL.Checks('deep14-batch', T14.WINO)
    check_steps(ck, mt, '%s-B%d' % (T14.IDS[mt], B), s43[pick], s9[pick], {k: outs[k][pick] for k in KEYS})
    ck.done()
    order = pick[::-1]
    _, t9, small = forwards(mt, x[order].contiguous())
    assert torch.equal(t9, s9[order])
    for key in KEYS:
        assert np.array_equal(small[key], outs[key][order]), key


# ---------------------------------------------------------------------------
# 4. what the shapes above cover
# ---------------------------------------------------------------------------
def test_shapes_cover_every_gemm_kernel():
    """Over the shapes of this file every GEMM launch of both models runs in
    every kernel the launcher's rule can give it for some M <= 2048 on this
    device; the query for the handle's device is the query for its CU count."""
    shapes = [(MT[mt], B, T) for mt, B, T in SHAPES]
    for mt, B, T in shapes[::7]:
        assert LP.gemm_launches(mt, B, T, 0) == LP.gemm_launches(mt, B, T, TL.ncu()), (mt, B, T)
    missing = LP.gemm_missing(shapes, TL.ncu())
    assert missing == [], 'no shape runs (model type, launch, kernel): %s' % missing
