"""oracle/layer_refs.py against the oracle it is built from (CPU only): the
float64 step chain agrees with the fp32 ``O.forward``, composes to the
oracle's own straight call bit for bit and its layout helpers round-trip; and
the library's launch plan (tests/launch_plan.py) gives the F(4x4,3x3) regimes
the sweep's shapes are chosen for."""
import numpy as np
import pytest
import torch

import launch_plan as LP
from oracle import layer_refs as R
from oracle import sed_oracle as O

GRU, TRF = R.GRU, R.TRF
SEEDS = {GRU: 0, TRF: 1}


def _err(a, b):
    assert tuple(a.shape) == tuple(b.shape), (a.shape, b.shape)
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize('B,T,C', [(2, 40, 25), (2, 135, 33)])
@pytest.mark.parametrize('mt', [GRU, TRF])
def test_float64_chain_agrees_with_oracle(mt, B, T, C):
    """fp32 vs float64 rounding of the reference arithmetic is 1e-7..2e-6 at
    every stage; 1e-5 leaves 5x and sits 100x inside the 1e-3 bar."""
    feat = R.features(B, T, seed=11)
    sd32 = R.state(mt, C, SEEDS[mt], torch.float32)
    sd32['_hop'] = 320
    ref = O.forward(sd32, mt, features=np.ascontiguousarray(feat.transpose(0, 2, 1))[:, None])
    sd64 = R.state(mt, C, SEEDS[mt], torch.float64)
    with torch.no_grad():
        got = R.chain(sd64, mt, R.step_bn0(sd64, torch.from_numpy(feat).double()))
        f32 = R.chain(sd32, mt, R.step_bn0(sd32, torch.from_numpy(feat)))
    for k in ('framewise_output', 'clipwise_output', 'embedding'):
        assert torch.equal(f32[k], ref[k]), k        # the fp32 chain is O.forward's op sequence
        assert got[k].dtype == torch.float64
        e = _err(got[k], ref[k])
        print(mt, (B, T, C), k, tuple(ref[k].shape), 'max|f64 - f32| = %.3g' % e)
        assert e <= 1e-5, (k, e)


@pytest.mark.parametrize('mt', [GRU, TRF])
def test_steps_compose_bit_for_bit(mt):
    B, T, C = 2, 43, 25
    sd = R.state(mt, C, SEEDS[mt], torch.float64)
    x = torch.from_numpy(R.features(B, T, seed=5)).double()
    with torch.no_grad():
        stages = {}
        got = R.chain(sd, mt, R.step_bn0(sd, x), stages)
        y, acts = O.cnn(sd, x.transpose(1, 2)[:, None])
        assert torch.equal(stages[0], acts['bn0'])
        for st, nm in ((2, 'block1'), (4, 'block2'), (6, 'block3'), (8, 'cnn_out')):
            assert torch.equal(stages[st], acts[nm]), nm
        s = O.gru_bidirectional(sd, y.transpose(1, 2)) if mt == GRU else O.multihead(sd, y.transpose(1, 2))
        assert torch.equal(stages[9], s)
        clip, _, cla = O.att_block(sd, s.transpose(1, 2))
        assert torch.equal(got['clipwise_output'], clip)
        assert torch.equal(got['framewise_output'], O.framewise_from_cla(cla, mt == GRU))
        assert torch.equal(got['embedding'], cla if mt == GRU else s.transpose(1, 2))
    assert got['framewise_output'].shape[1] == (100 if mt == GRU else 40)
    assert [stages[k].shape[1] for k in (3, 5, 7)] == [128, 256, 512]


def test_state_dtypes():
    sd = R.state(GRU, 7, 0, torch.float64)
    assert sd['bn0.num_batches_tracked'].dtype == torch.int64
    assert all(v.dtype == torch.float64 for k, v in sd.items() if not k.endswith('num_batches_tracked'))
    assert sd['att_block.cla.weight'].shape == (7, 512, 1)
    f = R.features(2, 9, 3)
    assert f.dtype == np.float32 and f.shape == (2, 64, 9)
    assert abs(float(f.mean()) + 40) < 3 and 15 < float(f.std()) < 25
    # everything before the head is the same for every class count (the GPU
    # tests share one trunk reference among their class counts)
    for mt in (GRU, TRF):
        a, b = R.state(mt, 25, 3, torch.float32), R.state(mt, 256, 3, torch.float32)
        assert all(torch.equal(a[k], b[k]) for k in a if not k.startswith('att_block.'))


def test_layouts_round_trip():
    B, T = 2, 37
    rng = np.random.default_rng(0)
    for st in R.STAGES:
        a = torch.from_numpy(rng.standard_normal(R.capture_shape(st, B, T)).astype(np.float32))
        x = R.from_capture(st, a)
        assert x.is_contiguous()
        assert torch.equal(R.to_capture(st, x), a)
    # the layouts are the oracle's: a float32 chain's stages land in capture shape
    sd = R.state(GRU, 25, 0, torch.float32)
    stages = {}
    with torch.no_grad():
        R.chain(sd, GRU, R.step_bn0(sd, torch.from_numpy(R.features(B, T, 1))), stages)
    for st in R.STAGES:
        assert tuple(R.to_capture(st, stages[st]).shape) == R.capture_shape(st, B, T), st
    x = stages[4]
    assert float(R.to_capture(4, x)[1, 3, 5, 7]) == float(x[1, 7, 3, 5])


def test_chain_conv1_fp32():
    """The in-order fp32 chain of the exact mode's direct conv is the same
    convolution (float64 distance at fp32 rounding level) at the sampled
    pixels, corners included."""
    B, T = 2, 19
    sd64, sd32 = R.state(GRU, 25, 0, torch.float64), R.state(GRU, 25, 0, torch.float32)
    stages = {}
    with torch.no_grad():
        R.chain(sd32, GRU, R.step_bn0(sd32, torch.from_numpy(R.features(B, T, 2))), stages)
        x = stages[4]                                   # [2, 128, 4, 16]
        pix = R.sample_pixels(B, x.shape[2], x.shape[3], 40)
        assert len(set(map(tuple, pix.tolist()))) == len(pix) >= 40
        assert [0, 0, 0] in pix.tolist() and [B - 1, x.shape[2] - 1, x.shape[3] - 1] in pix.tolist()
        E = R.chain_conv1_fp32(sd64, 3, x, pix)
        ref = R.step_conv1(sd64, 3, x.double())[pix[:, 0], :, pix[:, 1], pix[:, 2]]
    assert E.dtype == torch.float32 and E.shape == (len(pix), 256)
    e = _err(E, ref)
    print('chain vs float64: %.3g (max|ref| %.3g)' % (e, float(ref.abs().max())))
    assert 0 < e <= 2e-5


def test_w43_regimes():
    ncu = 256
    head = [LP.w43_regime(l, 32, 1001, ncu) for l in range(7)]
    assert head == ['nt4_claim'] * 5 + ['nt4_static'] * 2, head      # blocks 1-3 claim, block 4: 512 items
    assert LP.w43_launch(6, 32, 1001, ncu)['nitems'] == 512
    assert all(not LP.w43_launch(l, 4, 1001, ncu)['claim'] for l in range(7))
    assert [LP.w43_regime(l, 32, 994, ncu) for l in range(5)] == ['nt4_claim'] * 5
    # B = 72, T = 136: every launch claims (1224 / 720 / 576 / 576 items against 512)
    assert [LP.w43_launch(l, 72, 136, ncu)['nitems'] for l in range(7)] == [1224, 720, 720, 576, 576, 576, 576]
    assert all(LP.w43_regime(l, 72, 136, ncu) == 'nt4_claim' for l in range(7))
    assert all(LP.w43_launch(l, 72, 136, ncu)['nwg'] == 256 for l in range(7))
    # one clip: 16-channel items, of 16 tiles in the F = 16 / 8 layers
    assert [LP.w43_regime(l, 1, 64, ncu) for l in range(7)] == ['nt1_tg2'] * 3 + ['nt1_tg1'] * 4
    # the 32-tile 16-channel regime of blocks 3-4 needs exactly 16 and 8 tile blocks
    assert LP.w43_regime(3, 16, 37, ncu) == 'nt1_tg2' and LP.w43_regime(3, 8, 136, ncu) == 'nt1_tg2'
    assert LP.w43_regime(5, 8, 64, ncu) == 'nt1_tg2' and LP.w43_regime(5, 16, 64, ncu) == 'nt4_static'
    # below 8 clips the launches get no claim counters, whatever the item count
    assert LP.w43_launch(0, 7, 1001, ncu)['nitems'] > 512 and LP.w43_regime(0, 7, 1001, ncu) == 'nt4_static'


def test_sweep_covers_every_regime():
    """The shape list of the GPU sweep runs each of the seven F(4x4,3x3)
    launches in every regime it can reach (256 CUs)."""
    assert LP.w43_missing(R.SWEEP_SHAPES, 256) == []
    assert len(set(R.SWEEP_SHAPES)) == len(R.SWEEP_SHAPES)
    # and the check can fail: without the B >= 8 shapes nothing claims
    small = [s for s in R.SWEEP_SHAPES if s[0] < 8]
    assert (0, 'nt4_claim') in LP.w43_missing(small, 256)
