"""Record what a libsedx.so answers about shapes, per model type, into
tests/golden/model_shapes.json (tests/test_host_cpu.py holds a later library to
it).  The queries need no GPU.

    python tools/make_golden_model_shapes.py [path/to/libsedx.so]

Run it on the library of the commit whose answers are the baseline (a build of
that commit in a scratch copy), not on the one under test.

Per model, at 16 kHz / hop 160 with L = (T - 1) * 160 samples:
  points   every T of 1 .. 1400 (B = 1 for the size, 2 for the GEMM query), then LARGE's (B, T)
  columns  run-length encoded over the points, [[value, count], ...]:
           geom / size / gemm   status of sedx_output_geometry / sedx_workspace_size / sedx_gemm_launch_plan
           frames, seq          sedx_output_geometry's answers (-1 where it refuses)
           gemm_rows            sedx_gemm_launch_plan's row count (256 CUs)
           geom_msg / size_msg / gemm_msg   sedx_last_error of a refusal ('' where the call succeeds)
  gemm     the rows themselves at GEMM_POINTS, in the default mode and in x3
  windows  sedx_window_geometry for WINDOWS: [status, message, windows, window samples, merged frames]"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'sound-event-detection_amd'))
from sedx import _lib  # noqa: E402

MODELS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 13, 15, 16, 17, 19]
T_RANGE = 1400           # covers lcm(32, 100) = 800 and the VGGish 83-frame limit at T = 1344
# both sides of: 1000 VGGish sequence frames, 1000 and 5000 Conformer sequence frames, the 32-bit batch limit
LARGE = [(1, 16015), (1, 16016), (1, 32031), (1, 32032), (1, 40007), (1, 40008),
         (530, 63309), (530, 63310), (530, 63311)]
GEMM_POINTS = [(2, 65), (3, 1001)]
NCU = 256
# (driver, sample_duration, overlap_value, clip samples): six 5 s windows; main_strong's ever shorter windows past
# the padded 10 s, down to 6 frames; one 14 s window (87 VGGish sequence frames); one 420 s window (5250 / 2625 / 1312 sequence frames)
WINDOWS = [('predict', 5, 1.0, 160000), ('main_strong', 5, 0.05, 239360), ('predict', 14, 1.0, 320000),
           ('predict', 420, 1.0, 420 * 16000)]
COLUMNS = ('geom', 'frames', 'seq', 'size', 'gemm', 'gemm_rows', 'geom_msg', 'size_msg', 'gemm_msg')


def create(L, model_type):
    cfg = _lib.SedxConfig(model_type, 0, 16000, 512, 160, 64, 50.0, 7000.0, 25)
    h = ctypes.c_void_p()
    assert L.sedx_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    return h


def points():
    return [(1, T) for T in range(1, T_RANGE + 1)] + LARGE


def gemm_rows(L, h, B, T):
    """(status, row count, rows as lists) of sedx_gemm_launch_plan for B clips of T frames."""
    rows, n = (_lib.SedxGemmLaunch * 64)(), ctypes.c_int32()
    st = L.sedx_gemm_launch_plan(h, B, (T - 1) * 160, NCU, rows, 64, ctypes.byref(n))
    return st, n.value, [[getattr(r, f) for f, _ in r._fields_] for r in rows[:n.value]]


def point(L, h, B, T):
    """One point's values in COLUMNS order."""
    msg = lambda st: L.sedx_last_error(h).decode() if st else ''
    n = (T - 1) * 160
    fr, sl, wsz = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_size_t()
    g = L.sedx_output_geometry(h, n, ctypes.byref(fr), ctypes.byref(sl))
    g_msg = msg(g)
    w = L.sedx_workspace_size(h, B, n, ctypes.byref(wsz))
    w_msg = msg(w)
    m, rows, _ = gemm_rows(L, h, B if B > 1 else 2, T)
    return [g, fr.value if g == 0 else -1, sl.value if g == 0 else -1, w, m, rows, g_msg, w_msg, msg(m)]


def rle(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return out


def unrle(runs):
    return [v for v, n in runs for _ in range(n)]


def window(L, h, driver, sd, ov, samples):
    spec = _lib.window_spec(sd, ov, driver=driver)
    nw, ws, mf = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    st = L.sedx_window_geometry(h, samples, ctypes.byref(spec), ctypes.byref(nw), ctypes.byref(ws), ctypes.byref(mf))
    return [st, L.sedx_last_error(h).decode() if st else '', nw.value, ws.value, mf.value]


def gemm_section(L, h):
    out = []
    for prec in ('winograd', 'x3'):
        assert L.sedx_set_precision(h, _lib.PRECISION[prec]) == 0
        for B, T in GEMM_POINTS:
            st, _, rows = gemm_rows(L, h, B, T)
            out.append([prec, B, T, st, rows])
    assert L.sedx_set_precision(h, _lib.PRECISION['winograd']) == 0
    return out


def walk(L):
    models = {}
    for mt in MODELS:
        h = create(L, mt)
        cols = list(zip(*[point(L, h, B, T) for B, T in points()]))
        models[str(mt)] = {'columns': {name: rle(col) for name, col in zip(COLUMNS, cols)},
                           'gemm': gemm_section(L, h),
                           'windows': [window(L, h, *w) for w in WINDOWS]}
        L.sedx_destroy(h)
    return models


if __name__ == '__main__':
    if len(sys.argv) > 1:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    models = walk(_lib.lib())
    out = os.path.join(REPO, 'tests', 'golden', 'model_shapes.json')
    with open(out, 'w') as f:
        f.write('{"t_range": %d, "large": %s, "gemm_points": %s, "ncu": %d,\n "windows": %s,\n "models": {\n'
                % (T_RANGE, json.dumps(LARGE), json.dumps(GEMM_POINTS), NCU, json.dumps(WINDOWS)))
        f.write(',\n'.join('  "%s": %s' % (mt, json.dumps(m, separators=(',', ':'))) for mt, m in models.items()))
        f.write('\n }}\n')
    print('%d models x %d points -> %s (%d bytes)' % (len(models), len(points()), out, os.path.getsize(out)))
