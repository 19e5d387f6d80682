"""SEDX_PRECISION_F16 without a GPU: pack_f16 bit for bit against the numpy
emulation of q (a stand-alone host program under ASan + UBSan writes the
packs: tests/native/f16_pack_driver.cpp), the emulation of tests/f16_refs.py
inside the contract derived for it, the forward plan under the mode, and the
kernel's LDS images enumerated per ds_read_b128 lane group."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import f16_refs as H
from oracle import layer_refs as R
from sedx import _lib, models

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'sound-event-detection_amd')
PACK_SHAPES = ((64, 64, 64), (128, 64, 128), (512, 256, 128))


@pytest.fixture(scope='module')
def pack_dir(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('needs g++')
    r = subprocess.run(['make', '-s', '-C', PKG, 'build/f16_pack_driver'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = str(tmp_path_factory.mktemp('f16_pack'))
    r = subprocess.run([os.path.join(PKG, 'build', 'f16_pack_driver'), out], capture_output=True, text=True, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert 'f16_pack_driver: clean' in log and 'ERROR: AddressSanitizer' not in log and 'runtime error' not in log, log[-4000:]
    return out


# ---------------------------------------------------------------------------
# 1. the pack
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N,K,BN', PACK_SHAPES)
def test_pack_bit_for_bit(pack_dir, N, K, BN):
    """Every element of pack_f16's image, un-swizzled by the layout of
    weights.h ([N/BN][K/16][9][BN][2 slots][8]; k half c of channel n in slot
    c ^ ((n >> 3) & 1)), equals q of its weight, bit for bit; the planted edge
    values (the clamp, exact ties, 2^-14 (1 - 2^-12), subnormals, signed
    zeros) are among them."""
    tag = '%d_%d_%d' % (N, K, BN)
    w = np.fromfile(os.path.join(pack_dir, 'w_%s.f32' % tag), dtype=np.float32).reshape(N, K, 9)
    pk = np.fromfile(os.path.join(pack_dir, 'pk_%s.u16' % tag), dtype=np.uint16)
    assert pk.size == N * K * 9
    img = pk.reshape(N // BN, K // 16, 9, BN, 2, 8)
    n = np.arange(BN)
    got = np.empty((N // BN, K // 16, 9, BN, 2, 8), dtype=np.uint16)
    for c in range(2):                       # un-swizzle: logical half c of channel n
        got[:, :, :, n, c, :] = img[:, :, :, n, c ^ ((n >> 3) & 1), :]
    # -> [N][K][9]
    got = got.transpose(0, 3, 1, 4, 5, 2).reshape(N, K, 9)
    want = H.q_numpy(w).view(np.uint16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # the edge cases are there and come out as the contract says
    f = want.view(np.float16).astype(np.float64)
    assert (np.abs(w) > 65504).any() and np.isinf(w).any() and np.abs(f).max() == 65504.0
    assert ((np.abs(w) < H.TINY) & (w != 0)).any() and not ((np.abs(f) < H.TINY) & (f != 0)).any()
    assert not (want == 0x8000).any() and (w.view(np.uint32) == 0x80000000).any()      # -0 -> +0
    edge = np.float32(2.0 ** -14 * (1 - 2.0 ** -12))
    assert (w == edge).any() and (f[w == edge] == 2.0 ** -14).all()                    # rounds up to the smallest normal
    tie = np.float32(1 + 2.0 ** -11)
    assert (w == tie).any() and (f[w == tie] == 1.0).all()                             # a tie goes to even
    assert (f[w == np.float32(1 + 3 * 2.0 ** -11)] == 1 + 2.0 ** -9).all()


# ---------------------------------------------------------------------------
# 2, 3. the emulation against the un-rounded float64 reference
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sd64():
    return R.state(R.GRU, 25, 0, torch.float64)


@pytest.mark.parametrize('B,T', H.SHAPES)
def test_emulation_within_the_derived_contract(sd64, B, T):
    """Per conv step |E - R| <= 2^-10 S element-wise, with and without the
    flush: each operand moves by at most 2^-11 relative (or 2^-14 absolute in
    the flushed range, which 2^-10 S absorbs on these inputs), so a product
    moves by at most (2^-10 + 2^-22) of its magnitude.  A property of the
    reference alone; the inputs are each step's float64 predecessor in fp32."""
    with torch.no_grad():
        x = R.step_bn0(sd64, torch.from_numpy(R.features(B, T, 0)).double())
        for prev, nxt, E, _, Rf, S in H.steps():
            xin = x.float()
            r, s = Rf(sd64, xin), S(sd64, xin)
            for flush in (False, True):
                d = (E(sd64, xin, flush) - r).abs()
                worst = float((d / (2.0 ** -10 * s)).max())
                print('stage %d flush=%d: max|E - R| = %.3g, %.3f of the bound' % (nxt, flush, float(d.max()), worst))
                assert (d <= 2.0 ** -10 * s).all(), (nxt, flush, worst)
            x = r


@pytest.mark.parametrize('B,T', H.SHAPES)
def test_emulation_actually_rounds(B, T):
    e, r, dq = H.outputs(R.GRU, 0, B, T)
    print('d_q at (%d, %d): %s' % (B, T, dq))
    for k in H.KEYS:
        assert dq[k] > 0, k


# ---------------------------------------------------------------------------
# 4. the plan
# ---------------------------------------------------------------------------
def _handle(mid):
    L = _lib.lib()
    for cfg in (_lib.SedxConfig(mid, 0, 16000, 512, 160, 64, 50.0, 7000.0, 25),
                _lib.SedxConfig(mid, 0, 32000, 1024, 320, 64, 50.0, 14000.0, 25)):
        h = ctypes.c_void_p()
        if L.sedx_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0:
            return h, cfg.hop_size
    raise AssertionError('no handle for model id %d' % mid)


def _plan(h, hop, prec, B, T):
    L = _lib.lib()
    assert L.sedx_set_precision(h, _lib.PRECISION[prec]) == 0
    rows, n = (_lib.SedxConvLaunch * 64)(), ctypes.c_int32()
    assert L.sedx_conv_launch_plan(h, B, (T - 1) * hop, 256, rows, 64, ctypes.byref(n)) == 0
    conv = [{f: getattr(r, f) for f, _ in r._fields_} for r in rows[:n.value]]
    grows, gn = (_lib.SedxGemmLaunch * 64)(), ctypes.c_int32()
    assert L.sedx_gemm_launch_plan(h, B, (T - 1) * hop, 256, grows, 64, ctypes.byref(gn)) == 0
    gemm = [{f: getattr(r, f) for f, _ in r._fields_} for r in grows[:gn.value]]
    nb = ctypes.c_size_t()
    assert L.sedx_workspace_size(h, B, (T - 1) * hop, ctypes.byref(nb)) == 0
    return conv, gemm, nb.value


@pytest.mark.parametrize('mt', sorted(models.MODEL_IDS, key=models.MODEL_IDS.get))
def test_plan_under_f16(mt):
    """Family f16 on exactly the conv launches that report x3 under 'x3', the
    exact rows elsewhere; the GEMM rows and the workspace size are the exact
    mode's."""
    L = _lib.lib()
    assert _lib.PRECISION['f16'] == 3 and _lib.CONV_FAMILY['f16'] == 5
    h, hop = _handle(models.MODEL_IDS[mt])
    try:
        assert L.sedx_set_precision(h, 4) != 0 and L.sedx_set_precision(h, 3) == 0
        for B, T in ((1, 65), (3, 101), (32, 1001)):
            cx, _, _ = _plan(h, hop, 'x3', B, T)
            ce, ge, we = _plan(h, hop, 'exact', B, T)
            cf, gf, wf = _plan(h, hop, 'f16', B, T)
            assert len(cf) == len(cx) == len(ce)
            for rf, rx, re_ in zip(cf, cx, ce):
                if rx['family'] == _lib.CONV_FAMILY['x3']:
                    assert rf == dict(rx, family=_lib.CONV_FAMILY['f16']), (rf, rx)
                else:
                    assert rf == re_, (rf, re_)
            assert gf == ge and wf == we, (mt, B, T)
        nine = mt.startswith('Cnn_9layers')
        deep = mt.startswith(('Cnn_14layers', 'Cnn14'))
        assert sum(r['family'] == 5 for r in cf) == (7 if nine else 6 if deep else 0), mt
    finally:
        L.sedx_destroy(h)


def test_version_and_header_name_the_mode():
    hdr = open(os.path.join(os.path.dirname(PKG), 'include', 'sedx.h')).read()
    assert 'SEDX_PRECISION_F16 = 3' in hdr and 'SEDX_CONV_F16 = 5' in hdr
    assert b'fp16' in _lib.lib().sedx_version()
    m = models.Cnn_9layers_Gru_FrameAtt(16000, 512, 160, 64, 50, 7000, 25, 'logmel')
    assert m.set_precision('f16').precision == 'f16'
    with pytest.raises(ValueError):
        m.set_precision('f8')


# ---------------------------------------------------------------------------
# 5. the LDS images
# ---------------------------------------------------------------------------
# ds_read_b128: four groups of 16 lanes, one LDS cycle each when the group's 16-byte slots are distinct mod 16
# (64 banks of 4 bytes) or equal
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]


def test_lds_images_are_conflict_free(pack_dir):
    """Every A and B fragment read of every instantiated (F, BN, epilogue)
    shape, every wave, 32-row tile and tap: no two lanes of a ds_read_b128
    lane group on one bank with different addresses.  The slots come from
    f16_geom.h, which the kernel addresses LDS by."""
    seen, lines = set(), 0
    for line in open(os.path.join(pack_dir, 'lds.txt')):
        p = line.split()
        kind, (F, BN, pool, wave, tile, tap), slots = p[0], map(int, p[1:7]), np.array(p[7:], dtype=np.int64)
        assert slots.size == 64
        for g in B128_GROUPS:
            s = slots[g]
            by_bank = {}
            for a in s:
                by_bank.setdefault(int(a) % 16, set()).add(int(a))
            worst = max(len(v) for v in by_bank.values())
            assert worst == 1, '%s F=%d BN=%d pool=%d wave %d tile %d tap %d: %d-way conflict in group %s: %s' % (
                kind, F, BN, pool, wave, tile, tap, worst, g[:4], s.tolist())
        seen.add((kind, F, BN, pool))
        lines += 1
    shapes = {(64, 64, 1), (32, 128, 0), (32, 128, 1), (16, 128, 0), (16, 128, 1), (8, 128, 0)}
    assert seen == {(k,) + s for k in 'AB' for s in shapes} and lines == 2 * 6 * 8 * 2 * 9
