"""Block 1 of the F(4x4,3x3) chain on the channel-planar conv1 activation
(conv1_planar_kernel + the planar-input conv2, one 16-byte LDS-DMA halo piece
per wave per step; the default) against the chunk-of-4 pair
(SEDX_TUNE_WINO_ORDER 3) and the NHWC two-launch form (SEDX_TUNE_WINO_BLOCK1
1): the arithmetic per output is the same instructions in the same order, so
block 1's output, framewise_output and clipwise_output are compared bit for bit.

Shapes: the smallest at which the new staging can go wrong —
  a  B 1, T 5    less than one item; rows past T in every piece
  b  B 2, T 9    ragged last tile row; item boundary at row 8
  c  B 3, T 37   several items per clip; halo rows shared between items; the
                 t = -1 and t = T zero rows
  d  B 9, T 23   >= 8 clips: the forward passes the claim counters; clip
                 boundaries fall inside a workgroup's item sequence
and d again on memory pre-filled with 0xFF bytes: the zero columns and rows
of the halo image must come from the DMA's range check, not from leftovers.

Two levels.  The launchers themselves (conv1 + conv2 called through the
library's C++ entry points) run all four shapes, with the launcher's item
width (16-channel items at these sizes) and with the 64-channel items the
headline batch runs forced.  The forward runs b, c and d: a forward of T = 5
frames has no output — three 2 x 2 pools leave no frame, and the library
refuses it as the reference fails on it — so case a exists at the launcher
level only."""
import ctypes

import numpy as np
import pytest
import torch

from sedx import synth

pytestmark = pytest.mark.gpu

GRU = 'Cnn_9layers_Gru_FrameAtt'
CASES = {'a': (1, 5), 'b': (2, 9), 'c': (3, 37), 'd': (9, 23)}
EPI_POOL2 = 1

# the library's C++ launchers (csrc/sedx_internal.h), by their Itanium names
_CONV1 = {'nhwc': '_ZN4sedx17launch_conv1_nhwcEPKfiiS1_S1_PfP12ihipStream_t',
          'c4': '_ZN4sedx15launch_conv1_c4EPKfiiS1_S1_PfP12ihipStream_t',
          'planar': '_ZN4sedx19launch_conv1_planarEPKfiiS1_S1_PfP12ihipStream_t'}
_W43 = '_ZN4sedx21launch_conv3x3_wino43EPKfiiiiiS1_S1_PfiS2_P12ihipStream_tibiPib'
_PACK43 = '_ZN4sedx16pack_conv_wino43EPKdiiPf'


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class _Block1:
    """conv1 + block 1's F(4x4,3x3) conv2 through the launchers, on fixed random weights."""

    def __init__(self):
        from sedx import _lib
        L = _lib.lib()
        self.conv1 = {}
        for k, name in _CONV1.items():
            f = getattr(L, name)
            f.restype = None
            f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_void_p]
            self.conv1[k] = f
        self.w43 = getattr(L, _W43)
        self.w43.restype = None
        self.w43.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [
            ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_bool, ctypes.c_int, ctypes.c_void_p,
            ctypes.c_bool]
        pack = getattr(L, _PACK43)
        pack.restype = None
        pack.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        rng = np.random.default_rng(5)
        w = (rng.standard_normal((64, 64, 9)) * np.sqrt(2.0 / 576)).astype(np.float32).astype(np.float64)
        u = np.zeros(2 * 64 * 64 * 36, np.float32)
        pack(w.ctypes.data_as(ctypes.c_void_p), 64, 64, u.ctypes.data_as(ctypes.c_void_p))
        dev = 'cuda'
        self.u = torch.from_numpy(u).to(dev)
        self.w1 = torch.from_numpy((0.3 * rng.standard_normal((64, 9))).astype(np.float32)).to(dev)
        self.b1 = torch.from_numpy((0.1 * rng.standard_normal(64)).astype(np.float32)).to(dev)
        self.bias = torch.from_numpy((0.1 * rng.standard_normal(64)).astype(np.float32)).to(dev)
        self.trash = torch.zeros(64 * 256, dtype=torch.float32, device=dev)
        self.sched = torch.zeros(256, dtype=torch.int32, device=dev)

    def run(self, form, x0, nt_force=0, fill=None):
        """block 1's pooled output [B][T/2][32][64] of X0 [B][T][64] in one of the three forms;
        ``fill``: a byte every activation and output buffer holds before the launches."""
        B, T, _ = x0.shape
        kw = dict(dtype=torch.float32, device=x0.device)
        if fill is None:
            act, out = torch.empty(B * T * 64 * 64, **kw), torch.full((B * (T // 2) * 32 * 64,), float('nan'), **kw)
        else:
            act = torch.full((B * T * 64 * 64 * 4,), fill, dtype=torch.uint8, device=x0.device).view(torch.float32)
            out = torch.full((B * (T // 2) * 32 * 64 * 4,), fill, dtype=torch.uint8, device=x0.device).view(torch.float32)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.conv1[form](_p(x0), B, T, _p(self.w1), _p(self.b1), _p(act), s)
        c4 = form != 'nhwc'
        self.w43(_p(act), B, T, 64, 64, 64, _p(self.u), _p(self.bias), _p(out), EPI_POOL2, _p(self.trash), s, 1, c4,
                 nt_force, _p(self.sched), form == 'planar')
        torch.cuda.synchronize()
        assert int(self.sched.abs().sum()) == 0   # a claiming launch leaves its counters zero
        if c4:   # [B][16][T/2][32][4] -> [B][T/2][32][64]
            out = out.view(B, 16, T // 2, 32, 4).permute(0, 2, 3, 1, 4).reshape(B, T // 2, 32, 64)
        return out.reshape(B, T // 2, 32, 64).cpu().numpy()


@pytest.fixture(scope='module')
def block1():
    return _Block1()


def _x0(B, T):
    g = torch.Generator().manual_seed(100 * B + T)
    return torch.randn(B, T, 64, generator=g).cuda()


@pytest.mark.parametrize('nt_force', [0, 4], ids=['plan', 'nt4'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_planar_pair_launchers_bit_identical(block1, case, nt_force):
    """conv1_planar + the planar-input conv2 against conv1_c4 + the C4 conv2 and conv1_nhwc + the
    NHWC conv2, every pooled output bit for bit — at the plan's item width and with 64-channel items."""
    B, T = CASES[case]
    x0 = _x0(B, T)
    ref = block1.run('c4', x0, nt_force)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    assert np.array_equal(block1.run('nhwc', x0, nt_force), ref), 'C4 and NHWC pairs differ'
    got = block1.run('planar', x0, nt_force)
    bad = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print('case %s nt_force %d: %d of %d outputs differ' % (case, nt_force, bad, ref.size))
    assert bad == 0


@pytest.mark.parametrize('nt_force', [0, 4], ids=['plan', 'nt4'])
def test_planar_pair_launchers_on_dirty_memory(block1, nt_force):
    """Case d with conv1's activation and the output pre-filled with 0xFF bytes (NaN patterns): the halo
    image's zero groups, zero rows and piece tails are written by the DMA."""
    B, T = CASES['d']
    x0 = _x0(B, T)
    ref = block1.run('c4', x0, nt_force)
    got = block1.run('planar', x0, nt_force, fill=0xFF)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _build(tuning=()):
    from sedx import models
    m = getattr(models, GRU)(16000, 512, 160, 64, 25, 7000, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(GRU, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    m = m.to('cuda').eval().set_precision('winograd')
    for knob, v in tuning:
        m.set_tuning(knob, v)
    return m


def _forward(m, wave, T, ws_fill=None):
    """(b1c2's stage capture, framewise, clipwise) of one forward on the handle's workspace, or on a
    caller's workspace of exactly sedx_workspace_size bytes filled with ``ws_fill``."""
    from sedx import _lib
    from sedx.models import _ptr
    L = _lib.lib()
    nat = m.native(wave.device)
    B, length = wave.shape
    cap = torch.full((B, T // 2, 32, 64), float('nan'), dtype=torch.float32, device=wave.device)
    _lib.check(L.sedx_set_capture(nat.h, 2, _p(cap), cap.numel() * 4), nat.h, 'set_capture')
    try:
        if ws_fill is None:
            with torch.no_grad():
                o = m(wave)
            fw, clip = o['framewise_output'], o['clipwise_output']
        else:
            wsz, fr, sl = ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_int64()
            _lib.check(L.sedx_workspace_size(nat.h, B, length, ctypes.byref(wsz)), nat.h, 'workspace_size')
            _lib.check(L.sedx_output_geometry(nat.h, length, ctypes.byref(fr), ctypes.byref(sl)), nat.h, 'geometry')
            ws = torch.full((wsz.value,), ws_fill, dtype=torch.uint8, device=wave.device)
            C = m.classes_num
            fw = torch.full((B, fr.value, C), float('nan'), dtype=torch.float32, device=wave.device)
            clip = torch.full((B, C), float('nan'), dtype=torch.float32, device=wave.device)
            emb = torch.empty((B, C if m._embedding_cla else m._embedding_width, sl.value), dtype=torch.float32,
                              device=wave.device)
            stream = ctypes.c_void_p(torch.cuda.current_stream(wave.device).cuda_stream)
            _lib.check(L.sedx_forward(nat.h, _ptr(wave), B, length, _ptr(fw), _ptr(clip), _ptr(emb), _ptr(ws), wsz.value,
                                      stream), nat.h, 'forward')
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'set_capture')
    return cap.cpu().numpy(), fw.cpu().numpy(), clip.cpu().numpy()


@pytest.fixture(scope='module')
def handles():
    from sedx import _lib
    return {'planar': _build(), 'c4': _build([(_lib.TUNE_WINO_ORDER, 3)]), 'nhwc': _build([(_lib.TUNE_WINO_BLOCK1, 1)])}


def _wave(B, T):
    return torch.from_numpy(synth.make_waveforms(B, seconds=(T - 1) * 160 / 16000.0, sample_rate=16000,
                                                 seed=40 + B)).cuda()


@pytest.mark.parametrize('case', ['b', 'c', 'd'])
def test_planar_forward_bit_identical(handles, case):
    """The default handle (planar pair) against the C4 pair and the NHWC two-launch form: b1c2's stage
    capture, framewise_output and clipwise_output bit for bit."""
    B, T = CASES[case]
    wave = _wave(B, T)
    assert wave.shape[1] // 160 + 1 == T, wave.shape
    got = _forward(handles['planar'], wave, T)
    assert all(np.isfinite(a).all() for a in got)
    for other in ('c4', 'nhwc'):
        ref = _forward(handles[other], wave, T)
        for name, a, b in zip(('b1c2', 'framewise_output', 'clipwise_output'), got, ref):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (other, name)


def test_planar_forward_on_dirty_workspace(handles):
    """Case d on a workspace pre-filled with 0xFF bytes: the same three outputs as on the C4 pair."""
    B, T = CASES['d']
    wave = _wave(B, T)
    ref = _forward(handles['c4'], wave, T)
    got = _forward(handles['planar'], wave, T, ws_fill=0xFF)
    for name, a, b in zip(('b1c2', 'framewise_output', 'clipwise_output'), got, ref):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
