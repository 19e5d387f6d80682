"""References and cases of the gammatone front end, stage by stage (test
infrastructure only): the oracle's ``fft_weights`` restated with its
intermediates, a longdouble spectrum / ERB reference, numpy float64's own error
against it (the yardstick), the exact quantiser, the shapes and input classes of
tests/test_gpu_gamma.py and, per case, the oracle's codes, its float64
pre-truncation values (ties) and the quantiser branches the case takes.

CPU only; nothing here imports the library.
"""
import collections
import functools

import numpy as np

from oracle import sed_oracle as O
from sedx import synth

PRESETS = ('8k', '16k', '32k')
NFFT = {'8k': 512, '16k': 1024, '32k': 2048}
LD = np.longdouble
AMIN = 1e-10
TIE_GUARD = 1e-6                # of a code: the project's tie guard (tests/test_frontend_refs_cpu.py)
# The ERB table's error budget.  A relative weight error d moves a dB value by
# at most 10 / ln 10 * d = 4.343 d and a pre-truncation value by at most
# 4.343 * 32767 * d codes (unscaled worst case, maxabs <= 1).  The table may use
# 1 % of the tie guard: 4.343 * 32767 * d <= 1e-8, d <= 7.0e-14.
TABLE_BUDGET = 7.0e-14
DB_PER_REL = 10.0 / np.log(10.0)            # 4.343
assert DB_PER_REL * 32767 * TABLE_BUDGET <= 0.01 * TIE_GUARD < DB_PER_REL * 32767 * 7.1e-14
C_ORDER = 4                     # the project's factor for the same sums in another order


def geom(preset):
    """(sample_rate, nfft, nwin, hop, fmin) as fft_gtgram derives them."""
    p = O.PRESETS[preset]
    return p['sample_rate'], NFFT[preset], p['window_size'], p['hop_size'], p['fmin']


def kp_of(nfft):
    return (nfft // 2 + 1 + 31) // 32 * 32


def clip_len(preset, T, r):
    """L = nfft + hop (T - 1) + r: T columns; r = 0 leaves the last one unfilled."""
    _, nfft, _, hop, _ = geom(preset)
    assert 0 <= r < hop
    return nfft + hop * (T - 1) + r


def layout(B, L, nfft, hop):
    """include/sedx.h sedx_gamma_layout restated: regions of 256-byte granules."""
    al = lambda n: (n + 255) // 256 * 256
    T = 1 + (L - nfft) // hop
    fill = min(len(range(0, L - nfft, hop)), T)
    kp = kp_of(nfft)
    mag = 0
    db = mag + al(B * T * kp * 8)
    mm = db + al(B * 64 * T * 8)
    return dict(T=T, T_fill=fill, nfft=nfft, hop=hop, kp=kp, mag_offset=mag, db_offset=db, mm_offset=mm,
                total_bytes=mm + al(B * 16))


# ---------------------------------------------------------------------------
# host tables: the oracle's fft_weights with its intermediates
# ---------------------------------------------------------------------------
def _ri(z):
    """complex array -> float64 [..., 2] (re, im), the driver's layout."""
    z = np.asarray(z, np.complex128)
    return np.stack([z.real, z.imag], -1)


def weights_steps(preset):
    """``O.gammatone_weights`` statement by statement (the same numpy
    expressions, so ``w`` equals it bit for bit: tests/test_gamma_refs_cpu.py),
    keeping what csrc/gamma_weights.cpp's trace names."""
    fs, nfft, _, _, fmin = geom(preset)
    fs = float(fs)
    T = 1.0 / fs
    cf = O._erb_space(fmin, fs / 2, 64)[::-1]
    ear_q, min_bw = 9.26449, 24.7
    erb = (cf / ear_q + min_bw)
    B = 1.019 * 2 * np.pi * erb
    arg = 2 * cf * np.pi * T
    vec = np.exp(2j * arg)
    rt_pos, rt_neg = np.sqrt(3 + 2 ** 1.5), np.sqrt(3 - 2 ** 1.5)
    common = -T * np.exp(-(B * T))
    k11 = np.cos(arg) + rt_pos * np.sin(arg)
    k12 = np.cos(arg) - rt_pos * np.sin(arg)
    k13 = np.cos(arg) + rt_neg * np.sin(arg)
    k14 = np.cos(arg) - rt_neg * np.sin(arg)
    A11, A12, A13, A14 = common * k11, common * k12, common * k13, common * k14
    gain_arg = np.exp(1j * arg - B * T)
    gain = np.abs((vec - gain_arg * k11) * (vec - gain_arg * k12) * (vec - gain_arg * k13)
                  * (vec - gain_arg * k14)
                  * (T * np.exp(B * T) / (-1 / np.exp(B * T) + 1 + vec * (1 - np.exp(B * T)))) ** 4)
    B2 = np.exp(-2 * B * T)
    ucirc = np.exp(1j * 2 * np.pi * np.arange(0, nfft / 2 + 1) / nfft)[None, :]
    r = np.sqrt(B2)
    theta = 2 * np.pi * cf / fs
    pole = (r * np.exp(1j * theta))[:, None]
    w = (np.abs(ucirc + A11[:, None] * fs) * np.abs(ucirc + A12[:, None] * fs)
         * np.abs(ucirc + A13[:, None] * fs) * np.abs(ucirc + A14[:, None] * fs)
         * np.abs(fs * (pole - ucirc) * (pole.conj() - ucirc)) ** (-4) / gain[:, None])
    return dict(cf=cf, ucirc=_ri(ucirc[0]), erb=erb, B=B, arg=arg, vec=_ri(vec), common=common,
                k1=np.stack([k11, k12, k13, k14], -1), A1=np.stack([A11, A12, A13, A14], -1),
                gain_arg=_ri(gain_arg), gain=gain, B2=B2, r=r, theta=theta, pole=_ri(pole[:, 0]), w=w)


def weights_from(steps, preset):
    """The last statement of fft_weights from given intermediates (a trace of
    the host's, or the oracle's): which inputs carry a difference."""
    fs = float(geom(preset)[0])
    cx = lambda a: a[..., 0] + 1j * a[..., 1]
    ucirc = cx(steps['ucirc'])[None, :]
    pole = cx(steps['pole'])[:, None]
    A = steps['A1']
    return (np.abs(ucirc + A[:, 0, None] * fs) * np.abs(ucirc + A[:, 1, None] * fs)
            * np.abs(ucirc + A[:, 2, None] * fs) * np.abs(ucirc + A[:, 3, None] * fs)
            * np.abs(fs * (pole - ucirc) * (pole.conj() - ucirc)) ** (-4) / steps['gain'][:, None])


@functools.lru_cache(maxsize=None)
def ref_tables(preset):
    """(W [64, nfft/2+1], window [nfft]) of the reference, float64."""
    fs, nfft, nwin, _, fmin = geom(preset)
    return O.gammatone_weights(fs, nfft, 64, fmin, fs / 2), O.gammatone_window(nfft, nwin)


def ulps(a, b):
    """|a - b| in units of the spacing of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def rel_err(a, ref):
    """max |a - ref| / |ref| over |ref| >= 1e-300."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    m = np.abs(ref) >= 1e-300
    return float(np.max(np.abs(a[m] - ref[m]) / np.abs(ref[m]))) if m.any() else 0.0


# ---------------------------------------------------------------------------
# stage references
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twiddle_ld(n):
    """exp(-2 pi i k / n), k < n, longdouble."""
    pi = 4 * np.arctan(LD(1))
    k = np.arange(n)
    ang = (2 * pi / n) * k.astype(LD)
    return (np.cos(ang) - 1j * np.sin(ang)).astype(np.clongdouble)


def fft_ld(x):
    """DFT along the last axis (a power of two) in longdouble: iterative
    radix-2 decimation in time with the longdouble twiddle table."""
    x = np.asarray(x, np.clongdouble)
    n = x.shape[-1]
    assert n & (n - 1) == 0
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, '0%db' % bits)[::-1], 2) for i in range(n)]) if bits else np.zeros(1, int)
    y = x[..., rev].copy()
    tw = _twiddle_ld(n)
    h = 1
    while h < n:
        y = y.reshape(x.shape[:-1] + (n // (2 * h), 2, h))
        a, b = y[..., 0, :], y[..., 1, :] * tw[::n // (2 * h)][:h]
        y = np.concatenate([a + b, a - b], -1).reshape(x.shape[:-1] + (n,))
        h *= 2
    return y


def dft_ld(x, bins):
    """The defining sum at a few bins, longdouble (checks fft_ld)."""
    x = np.asarray(x, np.clongdouble)
    n = x.shape[-1]
    tw = _twiddle_ld(n)
    return np.stack([(x * tw[(k * np.arange(n)) % n]).sum(-1) for k in bins], -1)


def frames_of(audio, preset, flat, T):
    """[n, nfft] float32: the frames with flat index b T + t of audio [B, L]."""
    _, nfft, _, hop, _ = geom(preset)
    flat = np.asarray(flat)
    return np.stack([audio[f // T, (f % T) * hop:(f % T) * hop + nfft] for f in flat])


def spectrum_ref(frames, preset):
    """frames [n, nfft] float32 -> (R [n, nfft/2+1] longdouble |DFT(win frame)|,
    numpy float64's abs(fft(win * frame)) as the reference computes it)."""
    _, nfft, _, _, _ = geom(preset)
    win = ref_tables(preset)[1]
    nb = nfft // 2 + 1
    R = np.abs(fft_ld(win.astype(LD) * frames.astype(LD))[:, :nb])
    N = np.stack([np.abs(np.fft.fft(win * f)[0:nb]) for f in frames])
    return R, N


def spectrum_bound(R, N):
    """Per frame: C_ORDER max(e_np, 2^-52 max|R|) -> (bound [n], e_np [n])."""
    e_np = np.max(np.abs(N.astype(LD) - R), -1).astype(np.float64)
    floor = 2.0 ** -52 * np.max(R, -1).astype(np.float64)
    return C_ORDER * np.maximum(e_np, floor), e_np


def erb_ref(mag, preset):
    """mag [n, nfft/2+1] float64 (rows = frames) -> (g [n, 64] longdouble,
    R = 10 log10(max(1e-10, g)) longdouble, the same in numpy float64), with
    the reference's weights."""
    _, nfft, _, _, _ = geom(preset)
    W = ref_tables(preset)[0]
    g = np.dot(mag.astype(LD), W.T.astype(LD)) / LD(nfft)
    R = 10 * np.log10(np.maximum(LD(AMIN), g))
    gn = (W.dot(np.ascontiguousarray(mag.T)) / nfft).T     # fft_gtgram's own product, its operand layout
    N = 10.0 * np.log10(np.maximum(AMIN, gn))
    return g, R, N


def erb_bound(R, N, table_exact=False):
    e_np = float(np.max(np.abs(N.astype(LD) - R)))
    floor = 2.0 ** -52 * float(np.max(np.abs(R)))
    return C_ORDER * max(e_np, floor) + (0.0 if table_exact else DB_PER_REL * TABLE_BUDGET), e_np


def quant_ref(db):
    """db [64, T] float64 of one clip (before the clamp) -> the float32
    features: power_to_db's top_db clamp, float32_to_int16, int16_to_float32."""
    x = np.maximum(db, db.max() - 80.0)
    return O.int16_to_float32(O.float32_to_int16(x))


def codes_of(feats):
    """int16 codes of dequantised float32 features."""
    return np.round(np.asarray(feats, np.float64) * 32767).astype(np.int32)


# ---------------------------------------------------------------------------
# input classes (all seeded)
# ---------------------------------------------------------------------------
KINDS = ('synth', 'noise', 'tone', 'silence', 'impulse', 'tiny', 'subamin', 'loud64', 'loud1e4')


def inputs(kind, preset, B, L, seed=0):
    """[B, L] float32."""
    sr, nfft, _, _, _ = geom(preset)
    rng = np.random.default_rng(177 + seed)
    n = np.arange(L, dtype=np.float64)
    noise = lambda amp: (amp * rng.standard_normal((B, L))).astype(np.float32)
    if kind == 'synth':
        return np.ascontiguousarray(synth.make_waveforms(B, seconds=(L + 1.0) / sr, sample_rate=sr,
                                                         seed=177 + seed)[:, :L])
    if kind == 'noise':
        return noise(0.3)
    if kind == 'tone':                               # full-scale sines
        f = rng.uniform(0.01, 0.4, B) * sr
        ph = rng.uniform(0, 2 * np.pi, B)
        return np.sin(2 * np.pi * f[:, None] / sr * n[None, :] + ph[:, None]).astype(np.float32)
    if kind == 'silence':                            # all-zero clips at even b
        out = noise(1e-4)
        out[0::2] = 0
        return out
    if kind == 'impulse':                            # one non-zero sample per clip, inside the first frame
        out = np.zeros((B, L), np.float32)
        pos = rng.integers(nfft // 4, 3 * nfft // 4, B)
        out[np.arange(B), pos] = rng.uniform(0.3, 0.9, B).astype(np.float32)
        return out
    if kind == 'tiny':                               # 1e-7 noise: g in about [1.6e-9, 1.5e-7], dB near -80
        return noise(1e-7)
    if kind == 'subamin':                            # 1e-11 noise: every g <= 1.5e-11 < amin, every cell -100 dB
        return noise(1e-11)
    if kind == 'loud64':
        return noise(64 * 0.3)
    if kind == 'loud1e4':
        return noise(1e4 * 0.3)
    if kind == 'unscaled':                           # T = 1 clips whose 64 dB values all lie in [-1, 1]
        assert nfft < L < nfft + geom(preset)[3]
        return np.stack([unscaled_clip(preset, L, 10 * seed + b) for b in range(B)])
    raise ValueError(kind)


def unscaled_clip(preset, L, seed, iters=200):
    """One frame of 64 tones at the channel centres, their amplitudes iterated
    (at most ``iters`` oracle evaluations, over up to 8 draws of the phases)
    until max |dB| <= 1: float32_to_int16 then leaves the values unscaled, the
    one quantiser branch no natural clip takes.  g is linear in the
    amplitudes, so a damped multiplicative update converges in a few steps."""
    sr, nfft, nwin, hop, fmin = geom(preset)
    cf = O._erb_space(fmin, sr / 2, 64)[::-1]
    n = np.arange(L)
    for draw in range(8):
        ph = np.random.default_rng([377 + seed, draw]).uniform(0, 2 * np.pi, 64)
        S = np.sin(2 * np.pi * cf[:, None] / sr * n[None, :] + ph[:, None])
        a = np.ones(64)
        for _ in range(iters // 8):
            x = (a[:, None] * S).sum(0).astype(np.float32)
            db = 10.0 * np.log10(np.maximum(AMIN, O.fft_gtgram(x, sr, nwin / sr, hop / sr, 64, fmin)[:, 0]))
            if np.abs(db).max() <= 1.0:
                return x
            a *= 10.0 ** (-0.5 * db / 10.0)
    raise RuntimeError('no clip with every |dB| <= 1 found for %s in %d evaluations' % (preset, iters))


# ---------------------------------------------------------------------------
# the oracle on a case
# ---------------------------------------------------------------------------
Oracle = collections.namedtuple('Oracle', 'codes x guarded branches')


def branches_of(raw):
    """Which way gamma_quant_kernel's scalars go for a clip's dB values before
    the clamp (csrc/frontend.hip): a set of branch names."""
    mx, mn = float(raw.max()), float(raw.min())
    floor = mx - 80.0
    lo = max(mn, floor)
    maxabs = max(abs(mx), abs(lo))
    out = set()
    if mx == mn:
        out.add('equal')
    elif abs(mx) >= abs(lo):
        out.add('max')
    elif floor > mn:
        out.add('lo_floor')
    else:
        out.add('lo_nofloor')
    if mx > 0:
        out.add('pos')
    out.add('scaled' if maxabs > 1.0 else 'unscaled')
    return out


def oracle(audio, preset):
    """The oracle on audio [B, L]: int16 codes [B, 64, T] (int32), the float64
    pre-truncation values x 32767, the cells within TIE_GUARD of an integer
    (never those holding a scaled clip's max |dB|: +-32767 exactly, by construction)
    and the union of the clips' quantiser branches."""
    sr, _, nwin, hop, fmin = geom(preset)
    codes, xs, guard, br = [], [], [], set()
    for a in audio:
        g = O.fft_gtgram(a, sr, nwin / sr, hop / sr, 64, fmin)
        br |= branches_of(10.0 * np.log10(np.maximum(AMIN, g)))
        db = O.power_to_db(g)
        top = np.max(np.abs(db))
        x = db / top * 32767.0 if top > 1.0 else db * 32767.0
        exact = (np.abs(db) == top) if top > 1.0 else np.zeros(db.shape, bool)
        guard.append((np.abs(x - np.round(x)) < TIE_GUARD) & ~exact)
        xs.append(x)
        codes.append(O.float32_to_int16(db).astype(np.int32))
    return Oracle(np.stack(codes), np.stack(xs), np.stack(guard), br)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'preset spec T r B kind seed walk')
EDGE_T = (1, 2, 63, 64, 65, 127, 128, 129, 193)     # 32 k: around gamma_erb_kernel's 64-frame tile
WALK_T = 257
WALK_GUARDED = 1e-5             # of a walk case's cells (about 2e-6 expected)


def case_id(c):
    return '%s-s%d-T%d-r%d-B%d-%s' % (c.preset, c.spec, c.T, c.r, c.B, c.kind) + ('-walk' if c.walk else '')


def walk_B(ncu):
    """8 workgroups of 256 threads per CU (the wave limit) times the
    launcher's factor 4 is the largest grid launch_gamma_spec can choose:
    B T > 32 ncu frames walk whatever the occupancy is."""
    return -(-(32 * ncu + 1) // WALK_T)


def _seeded(preset, spec, T, r, B, kind, walk=False):
    key = (preset, T, r, B, kind)
    return Case(preset, spec, T, r, B, kind, SEEDS.get(key, 0), walk)


def edge_cases():
    """32 k: every EDGE_T x r in {0, 1, hop - 1} on the Stockham kernel
    (spec 0) and every EDGE_T x r in {0, 2, hop - 2} (even L: float2 loads) on
    the wave kernel (spec 1), plus two odd L with spec 1 (the launcher falls
    back to the Stockham kernel); the input class and B in {1, 3} rotate so
    every class meets both kernels, a full tile, a partial tile and T = 1.
    16 k / 8 k: T in {1, 64, 65, 129}, B = 3."""
    hop = geom('32k')[3]
    out = []
    for spec, rs, shift in ((0, (0, 1, hop - 1), 0), (1, (0, 2, hop - 2), 4)):
        i = 0
        for T in EDGE_T:
            for r in rs:
                kind = KINDS[(i + shift) % len(KINDS)]
                B = 3 if kind == 'silence' or i % 2 else 1
                out.append(_seeded('32k', spec, T, r, B, kind))
                i += 1
    out.append(_seeded('32k', 1, 1, 1, 3, 'synth'))
    out.append(_seeded('32k', 1, 65, 1, 3, 'silence'))
    # the unscaled branch (max |dB| <= 1): one frame, both kernels at 32 k (even L for the wave kernel)
    out.append(_seeded('32k', 0, 1, 1, 3, 'unscaled'))
    out.append(_seeded('32k', 1, 1, 2, 3, 'unscaled'))
    out.append(_seeded('16k', 0, 1, 1, 3, 'unscaled'))
    out.append(_seeded('8k', 0, 1, 1, 3, 'unscaled'))
    for preset, kinds in (('16k', ('synth', 'silence', 'impulse', 'loud64')), ('8k', ('noise', 'subamin', 'tiny', 'loud1e4'))):
        h = geom(preset)[3]
        for T, r, kind in zip((1, 64, 65, 129), (0, 1, 0, h - 1), kinds):
            out.append(_seeded(preset, 0, T, r, 3, kind))
    return out


def walk_cases(ncu=256):
    """One per preset and spectrum kernel: T = 257, r = 0 (every clip's last
    column unfilled, so the walk meets the zero rows too, and L is even)."""
    B = walk_B(ncu)
    return [_seeded(p, s, WALK_T, 0, B, 'synth', walk=True) for p, s in (('32k', 0), ('32k', 1), ('16k', 0), ('8k', 0))]


@functools.lru_cache(maxsize=64)
def _case_data(preset, T, r, B, kind, seed):
    audio = inputs(kind, preset, B, clip_len(preset, T, r), seed)
    return audio, oracle(audio, preset)


def case_data(c):
    """(audio [B, L] float32, Oracle), cached: the spec 0 / 1 twins share it."""
    return _case_data(c.preset, c.T, c.r, c.B, c.kind, c.seed)


def sample_frames(c, ncu, n=24):
    """Up to n flat frame indices b T + t: first, last, last filled, the ERB
    tile edges of the first and last clip and, in a walk case, both sides of
    every grid size launch_gamma_spec can choose (4 ncu per_cu, per_cu <= 8)."""
    T, total = c.T, c.B * c.T
    fill = T - 1 if c.r == 0 else T
    pick = [0, total - 1, (c.B - 1) * T + max(fill - 1, 0), fill - 1 if fill else 0]
    if c.walk:
        for p in range(1, 9):
            pick += [4 * ncu * p - 1, 4 * ncu * p]
    for t in (63, 64, 65, 127, 128, 129, 191, 192, 1, T // 2):
        pick += [t, (c.B - 1) * T + t] if t < T else []
    seen = []
    for f in pick:
        if 0 <= f < total and f not in seen:
            seen.append(f)
    return np.array(seen[:n])


# seeds under which no cell of the case is guarded (tests/test_gamma_refs_cpu.py
# asserts it); a case not listed uses seed 0.  Key: (preset, T, r, B, kind).
SEEDS = {('32k', 65, 318, 1, 'synth'): 1}
