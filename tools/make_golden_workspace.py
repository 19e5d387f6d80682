"""Record the byte counts and geometries a libsedx.so answers into
tests/golden/workspace_sizes.json (tests/test_host_cpu.py compares a later
library against them).  The queries need no GPU.

    python tools/make_golden_workspace.py [path/to/libsedx.so]

Run it on the library of the commit whose sizes are the baseline (a build of
that commit in a scratch copy), not on the one under test."""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'sound-event-detection_amd'))
from sedx import _lib  # noqa: E402

PAIRS = [(1, 1280), (1, 5280), (5, 5280), (3, 117280), (32, 160000)]   # (clips, samples)
WINDOW = dict(sample_duration=5, overlap_value=1.0, n_clips=2, samples=160000)
TUNE_WINO_BLOCK1, TUNE_WINO_F43 = 2, 7
MODELS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 13, 15, 16, 17, 19]   # every sedx_model_type (include/sedx.h)


def create(L, model_type):
    cfg = _lib.SedxConfig(model_type, 0, 16000, 512, 160, 64, 50.0, 7000.0, 25)
    h = ctypes.c_void_p()
    assert L.sedx_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    return h


def sizes(L, h, B, samples):
    """[workspace bytes, output frames, sequence frames] of B clips of ``samples`` samples; where the model
    refuses the pair, the two queries' statuses instead: ['refused', size status, geometry status]."""
    wsz, fr, sl = ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_int64()
    st = [L.sedx_workspace_size(h, B, samples, ctypes.byref(wsz)),
          L.sedx_output_geometry(h, samples, ctypes.byref(fr), ctypes.byref(sl))]
    return [wsz.value, fr.value, sl.value] if st == [0, 0] else ['refused'] + st


def window_size(L, h):
    spec = _lib.window_spec(WINDOW['sample_duration'], WINDOW['overlap_value'])
    wsz = ctypes.c_size_t()
    assert L.sedx_window_workspace_size(h, WINDOW['n_clips'], WINDOW['samples'], ctypes.byref(spec),
                                        ctypes.byref(wsz)) == 0
    return wsz.value


def walk(L):
    """rows [model, precision, wino_block1, wino_f43, clips, samples, bytes, frames, seq] and
    the window workspace bytes per model of MODELS (default tuning)."""
    rows, windows = [], []
    for model_type in MODELS:
        h = create(L, model_type)
        windows.append(window_size(L, h))
        for precision in range(3):
            assert L.sedx_set_precision(h, precision) == 0
            for b1 in range(3):
                assert L.sedx_set_tuning(h, TUNE_WINO_BLOCK1, b1) == 0
                for f43 in range(3):
                    assert L.sedx_set_tuning(h, TUNE_WINO_F43, f43) == 0
                    for B, n in PAIRS:
                        rows.append([model_type, precision, b1, f43, B, n] + sizes(L, h, B, n))
        L.sedx_destroy(h)
    return rows, windows


if __name__ == '__main__':
    if len(sys.argv) > 1:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    rows, windows = walk(_lib.lib())
    out = os.path.join(REPO, 'tests', 'golden', 'workspace_sizes.json')
    with open(out, 'w') as f:
        f.write('{"models": %s,\n "window": %s,\n "window_bytes": %s,\n "rows": [\n  '
                % (json.dumps(MODELS), json.dumps(WINDOW), json.dumps(windows)))
        f.write(',\n  '.join(json.dumps(r) for r in rows))
        f.write('\n ]}\n')
    print('%d rows, %d window sizes -> %s' % (len(rows), len(windows), out))
