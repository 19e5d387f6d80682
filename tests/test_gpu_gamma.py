"""The gammatone front end (csrc/frontend.hip: gamma_spec_kernel /
gamma_spec_wave_kernel, gamma_erb_kernel, gamma_quant_kernel) stage by stage
against float64 / longdouble references, at the frame counts around the ERB
kernel's 64-frame tile, at batches large enough that the spectrum kernels walk
frames, over input classes that take every quantiser branch, and with a dirty,
shared, banded or handle-owned workspace.

Each stage's reference is applied to the GPU's own previous stage, read from the
workspace through sedx_gamma_workspace_layout (tests/gamma_refs.py holds the
references, the cases and the yardsticks; tests/test_gamma_refs_cpu.py checks
them on the CPU):

  spectrum   audio -> mag   max|G - R| <= 4 max(e_np, 2^-52 max|R|) per sampled
                            frame, R = |DFT(win frame)| in longdouble, e_np the
                            error of numpy's float64 abs(fft(.)); pad bins,
                            unfilled rows and silent clips exactly 0
  ERB + dB   mag -> db      |G - R| <= 4 max(e_np, 2^-52 max|R|) + 4.343 * 7.0e-14
                            dB (the host table's budget), R in longdouble with the
                            reference's weights; g <= 1e-10 gives exactly -100
  quantiser  db -> feats    bit-identical to numpy float64's clamp, scale and
                            truncation on the GPU's db
  end to end                the oracle's int16 codes in every cell that is not
                            within 1e-6 of a rounding boundary (none outside the
                            walk cases), those within one code

Every stage check prints a ``RATIO`` line before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gamma_refs as G
from oracle import sed_oracle as O
from sedx import synth

pytestmark = pytest.mark.gpu

GRU = 'Cnn_9layers_Gru_FrameAtt'
EINVAL = 1
HYGIENE = dict(preset='32k', B=3, T=65)


@functools.lru_cache(maxsize=None)
def _model(preset):
    from sedx import models
    p = O.PRESETS[preset]
    m = getattr(models, GRU)(p['sample_rate'], p['window_size'], p['hop_size'], 64, p['fmin'], p['fmax'], 25, 'gamma')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(GRU, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval()


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _handle(preset, spec):
    from sedx import _lib
    m = _model(preset)
    m.set_tuning(_lib.TUNE_GAMMA_SPEC, spec)
    return m.native(torch.device('cuda', torch.cuda.current_device())).h


def _layout(h, B, L):
    """The layout query, checked against the size query."""
    from sedx import _lib
    lib = _lib.lib()
    lay, wsz = _lib.SedxGammaLayout(), ctypes.c_size_t()
    _lib.check(lib.sedx_gamma_workspace_layout(h, B, L, ctypes.byref(lay)), h, 'gamma_workspace_layout')
    _lib.check(lib.sedx_gamma_workspace_size(h, B, L, ctypes.byref(wsz)), h, 'gamma_workspace_size')
    assert wsz.value == lay.total_bytes
    return lay


def _forward(h, x, ws, ws_bytes, out=None):
    """sedx_gamma_features on the current stream, no synchronisation."""
    from sedx import _lib
    lib = _lib.lib()
    B, L = x.shape
    T = ctypes.c_int64()
    _lib.check(lib.sedx_gamma_features(h, None, B, L, None, ctypes.byref(T), None, 0, None), h, 'gamma geometry')
    if out is None:
        out = torch.empty((B, 64, T.value), dtype=torch.float32, device=x.device)
    _lib.check(lib.sedx_gamma_features(h, _ptr(x), B, L, _ptr(out), ctypes.byref(T), _ptr(ws), ws_bytes, _stream()),
               h, 'gamma_features')
    return out


def _run(preset, spec, audio, fill=None, own=False):
    """-> (features [B, 64, T] on the device, workspace bytes or None, layout)."""
    h = _handle(preset, spec)
    x = torch.from_numpy(np.ascontiguousarray(audio)).cuda()
    lay = _layout(h, *x.shape)
    if own:
        return _forward(h, x, None, 0), None, lay
    ws = torch.empty(lay.total_bytes, dtype=torch.uint8, device='cuda')
    if fill is not None:
        ws.fill_(fill)
    return _forward(h, x, ws, ws.numel()), ws, lay


def _stages(ws, lay, B):
    """(mag [B, T, kp], db [B, 64, T]) float64 views of the workspace."""
    T, kp = lay.T, lay.kp
    mag = ws[lay.mag_offset:lay.mag_offset + B * T * kp * 8].view(torch.float64).view(B, T, kp)
    db = ws[lay.db_offset:lay.db_offset + B * 64 * T * 8].view(torch.float64).view(B, 64, T)
    return mag, db


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------
# the stages, case by case
# ---------------------------------------------------------------------------
def _cases():
    # the walk cases' batch follows the device's CU count: built at run time from this template
    return G.edge_cases() + G.walk_cases(256)


@pytest.mark.parametrize('case', _cases(), ids=G.case_id)
def test_gamma_stages(case):
    c = case
    ncu = _ncu()
    if c.walk:
        c = [w for w in G.walk_cases(ncu) if (w.preset, w.spec) == (c.preset, c.spec)][0]
        # more frames than the largest grid the launcher can choose: the kernels walk
        assert c.B * c.T > 32 * ncu
    tag = G.case_id(c)
    _, nfft, _, hop, _ = G.geom(c.preset)
    nb = nfft // 2 + 1
    audio, orc = G.case_data(c)
    B, L = audio.shape
    feats, ws, lay = _run(c.preset, c.spec, audio)
    torch.cuda.synchronize()
    T, fill = lay.T, lay.T_fill
    assert (T, fill, lay.kp) == (c.T, c.T - 1 if c.r == 0 else c.T, G.kp_of(nfft))
    assert feats.shape == (B, 64, T)
    mag_t, db_t = _stages(ws, lay, B)
    failures = []

    # ---- spectrum: audio -> mag ----
    flat = G.sample_frames(c, ncu)
    filled = np.array([f for f in flat if f % T < fill], dtype=np.int64)
    Gm = mag_t.reshape(B * T, lay.kp)[torch.from_numpy(flat).cuda()].cpu().numpy()
    worst = 0.0
    if filled.size:
        R, N = G.spectrum_ref(G.frames_of(audio, c.preset, filled, T), c.preset)
        bound, e_np = G.spectrum_bound(R, N)
        Gf = Gm[[list(flat).index(f) for f in filled], :nb]
        e = np.max(np.abs(Gf.astype(G.LD) - R), -1).astype(np.float64)
        ok = (e <= bound) | ((bound == 0) & (e == 0))
        ratio = np.where(bound > 0, e / np.where(bound > 0, bound, 1), np.where(e == 0, 0.0, np.inf))
        i = int(np.argmax(ratio))
        worst = float(ratio[i])
        print('RATIO|spectrum|%s|%.3f| frames=%d worst frame=%d e=%.3g e_np=%.3g bound=%.3g max|R|=%.3g'
              % (tag, worst, filled.size, filled[i], e[i], e_np[i], bound[i], float(np.max(R[i]))))
        if not ok.all():
            failures.append('spectrum: e/bound = %.3f at frame %d' % (worst, filled[i]))
    else:
        print('RATIO|spectrum|%s|0.000| no filled frame' % tag)
    pad_max = float(mag_t[:, :, nb:].abs().max()) if lay.kp > nb else 0.0
    unfilled_max = float(mag_t[:, fill:, :].abs().max()) if fill < T else 0.0
    silent = [b for b in range(B) if not audio[b].any()]
    silent_max = float(mag_t[silent].abs().max()) if silent else 0.0
    finite = bool(torch.isfinite(mag_t).all())
    print('ZEROS|spectrum|%s| pad=%g unfilled=%g silent(%d clips)=%g finite=%s'
          % (tag, pad_max, unfilled_max, len(silent), silent_max, finite))
    if pad_max != 0 or unfilled_max != 0 or silent_max != 0 or not finite:
        failures.append('spectrum: pad bins / unfilled rows / silent clips not exactly 0, or not finite')

    # ---- ERB + dB: the GPU's mag -> db ----
    sel = flat if c.walk else np.arange(B * T)
    mag_rows = (Gm if c.walk else mag_t.reshape(B * T, lay.kp).cpu().numpy())[:, :nb]
    db_rows = db_t.permute(0, 2, 1).reshape(B * T, 64)[torch.from_numpy(sel).cuda()].cpu().numpy()
    g, Rdb, Ndb = G.erb_ref(mag_rows, c.preset)
    bound, e_np = G.erb_bound(Rdb, Ndb)
    e = np.abs(db_rows.astype(G.LD) - Rdb).astype(np.float64)
    i = np.unravel_index(int(np.argmax(e)), e.shape)
    below = np.asarray(g <= G.LD(G.AMIN))
    clamp_ok = bool((db_rows[below] == -100.0).all())
    print('RATIO|erb|%s|%.3f| frames=%d e=%.3g at frame %d ch %d, e_np=%.3g bound=%.3g, cells at the clamp %d exact=%s'
          % (tag, e.max() / bound, len(sel), e.max(), sel[i[0]], i[1], e_np, bound, int(below.sum()), clamp_ok))
    if not e.max() <= bound:
        failures.append('erb: e/bound = %.3f' % (e.max() / bound))
    if not clamp_ok:
        failures.append('erb: cells with g <= 1e-10 are not exactly -100')

    # ---- quantiser: the GPU's db -> features, exact ----
    db_all = db_t.cpu().numpy()
    want = np.stack([G.quant_ref(db_all[b]) for b in range(B)])
    got = feats.cpu().numpy()
    dq = got.view(np.int32) != want.view(np.int32)
    nq = int(dq.sum())
    print('RATIO|quant|%s|%d| cells differing in bits, of %d; first %s got %s want %s'
          % (tag, nq, got.size, np.argwhere(dq)[:4].tolist(), got[dq][:4].tolist(), want[dq][:4].tolist()))
    if nq:
        failures.append('quantiser: %d cells differ from numpy float64 on the same db' % nq)

    # ---- end to end: the oracle's codes ----
    q = G.codes_of(got)
    d = q != orc.codes
    hard = d & ~orc.guarded
    far = np.abs(q - orc.codes) > 1
    print('RATIO|codes|%s|%d| cells differing, %d of them unguarded, %d guarded cells of %d; first %s'
          % (tag, int(d.sum()), int(hard.sum()), int(orc.guarded.sum()), d.size, np.argwhere(d)[:4].tolist()))
    if not c.walk and orc.guarded.any():
        failures.append('a guarded cell outside a walk case')
    if orc.guarded.sum() > G.WALK_GUARDED * d.size:
        failures.append('too many guarded cells')
    if hard.any() or far.any():
        failures.append('codes: %d unguarded cells differ, %d by more than one code' % (int(hard.sum()), int(far.sum())))
    assert not failures, (tag, failures)


# ---------------------------------------------------------------------------
# workspace hygiene (B = 3, T = 65, 32 k)
# ---------------------------------------------------------------------------
def _hyg_audio(kind='synth', seed=21, r=2):
    return G.inputs(kind, HYGIENE['preset'], HYGIENE['B'], G.clip_len(HYGIENE['preset'], HYGIENE['T'], r), seed)


@pytest.mark.parametrize('spec', [0, 1])
def test_dirty_workspace_and_band(spec):
    """A workspace full of 0xFF bytes (NaNs, a poisoned max / min pair) gives
    the clean run's bits, and a 4 KiB patterned band after the reported size
    comes back intact."""
    audio = _hyg_audio()
    clean, _, lay = _run('32k', spec, audio, fill=0)
    h = _handle('32k', spec)
    x = torch.from_numpy(audio).cuda()
    band = (torch.arange(4096, device='cuda') % 251).to(torch.uint8)
    ws = torch.empty(lay.total_bytes + 4096, dtype=torch.uint8, device='cuda')
    ws[:lay.total_bytes] = 0xFF
    ws[lay.total_bytes:] = band
    dirty = _forward(h, x, ws, lay.total_bytes)
    torch.cuda.synchronize()
    assert torch.isfinite(dirty).all()
    assert torch.equal(_bits(dirty), _bits(clean))
    assert torch.equal(ws[lay.total_bytes:], band)
    # a byte short of the reported size is refused
    from sedx import _lib
    T = ctypes.c_int64()
    st = _lib.lib().sedx_gamma_features(h, _ptr(x), x.shape[0], x.shape[1], _ptr(dirty), ctypes.byref(T), _ptr(ws),
                                        lay.total_bytes - 1, _stream())
    assert st == EINVAL


@pytest.mark.parametrize('spec', [0, 1])
def test_two_calls_share_a_workspace_without_a_sync(spec):
    """Two calls with different audio on one stream and one workspace, nothing
    in between: gamma_init_kernel re-arms the per-clip max / min, so the
    second result is its stand-alone result (a quiet batch after a loud one: a
    stale max would move every code)."""
    loud, quiet = _hyg_audio('loud64', 22), _hyg_audio('silence', 23)
    alone, _, lay = _run('32k', spec, quiet)
    alone_loud, _, _ = _run('32k', spec, loud)
    h = _handle('32k', spec)
    ws = torch.empty(lay.total_bytes, dtype=torch.uint8, device='cuda')
    xa, xb = torch.from_numpy(loud).cuda(), torch.from_numpy(quiet).cuda()
    first = _forward(h, xa, ws, ws.numel())
    second = _forward(h, xb, ws, ws.numel())
    torch.cuda.synchronize()
    assert torch.equal(_bits(second), _bits(alone))
    assert torch.equal(_bits(first), _bits(alone_loud))
    assert not torch.equal(_bits(first), _bits(second))


def test_handle_owned_workspace_grows_and_is_reused():
    """NULL workspace: the handle's cache serves a small call, grows for a
    walk-sized one and serves the small one again from the larger block; all
    three equal their caller-workspace runs."""
    small = _hyg_audio('noise', 24)
    c = G.walk_cases(_ncu())[0]
    big, _ = G.case_data(c)
    want_small, _, _ = _run('32k', 0, small)
    want_big, _, _ = _run('32k', 0, big)
    for audio, want in ((small, want_small), (big, want_big), (small, want_small)):
        got, _, _ = _run('32k', 0, audio, own=True)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize('spec', [0, 1])
@pytest.mark.parametrize('kind', ['synth', 'silence'])
def test_each_clip_equals_itself_alone(kind, spec):
    """Clip b of a batch (a silent clip beside loud ones in ``silence``)
    equals the same clip at B = 1: the per-clip max / min pair is the clip's."""
    audio = _hyg_audio(kind, 25)
    batch, _, _ = _run('32k', spec, audio)
    for b in range(audio.shape[0]):
        one, _, _ = _run('32k', spec, audio[b:b + 1])
        assert torch.equal(_bits(one[0]), _bits(batch[b])), b


@pytest.mark.parametrize('preset', G.PRESETS)
def test_clip_shorter_than_the_fft_is_refused(preset):
    from sedx import _lib
    lib = _lib.lib()
    h = _handle(preset, 0)
    nfft = G.NFFT[preset]
    wsz, T, lay = ctypes.c_size_t(), ctypes.c_int64(), _lib.SedxGammaLayout()
    assert lib.sedx_gamma_workspace_size(h, 1, nfft - 1, ctypes.byref(wsz)) == EINVAL
    assert lib.sedx_gamma_workspace_layout(h, 1, nfft - 1, ctypes.byref(lay)) == EINVAL
    x = torch.zeros((1, nfft - 1), dtype=torch.float32, device='cuda')
    out = torch.full((1, 64, 1), 7.0, dtype=torch.float32, device='cuda')
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    assert lib.sedx_gamma_features(h, _ptr(x), 1, nfft - 1, _ptr(out), ctypes.byref(T), _ptr(ws), ws.numel(),
                                   _stream()) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all()                          # nothing was launched
    # L = nfft is the shortest clip: one column, never filled
    assert lib.sedx_gamma_workspace_size(h, 1, nfft, ctypes.byref(wsz)) == 0
    assert lib.sedx_gamma_workspace_layout(h, 1, nfft, ctypes.byref(lay)) == 0 and (lay.T, lay.T_fill) == (1, 0)
