"""Record what the Winograd conv launchers of the baseline commit decide into
tests/golden/conv_launches.json (tests/test_host_cpu.py holds
``sedx_conv_launch_plan`` of later libraries to it, row by row).

    python tools/make_golden_conv_launches.py path/to/instrumented/libsedx.so

This runs against an INSTRUMENTED build of the baseline commit (5e2239f, the
last one whose launchers decide inside conv_wino.hip / conv_wino43.hip), made
in a scratch copy and never committed:
  * ``launch_wino_w``, ``launch_block1_w`` and ``launch_w43_g`` print one line
    per launch: the stage, the family, their inputs, TG, NT (F(4x4): 1 for
    16-channel items, else 4), c4, tb_per_clip, ngroups, nitems, nwg, claim,
    order2d and the entry point's ``bmax``;
  * the CU count they query is overridden by a global;
  * an extra entry ``sedx_dbg_conv(handle, B, T, ncu, path)`` runs
    ``plan_forward`` and the conv loop of ``run_body`` (copied verbatim) with
    null buffers, appending those lines to ``path``.
No GPU is needed: without a device the launchers still compute every decision
and ``launch_info`` then refuses the launch.  The library under test is never
the source of this file."""
import ctypes
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'sound-event-detection_amd'))
sys.path.insert(0, REPO)
from sedx import _lib  # noqa: E402
from oracle.layer_refs import SWEEP_SHAPES  # noqa: E402

COLUMNS = ['stage', 'family', 'clips', 'T', 'F', 'cin', 'cout', 'epi', 'tg', 'nt', 'c4', 'tb_per_clip', 'ngroups',
           'nitems', 'nwg', 'claim', 'order2d', 'clips_per_launch']
DEFAULT = (2, 2, 1)   # SEDX_TUNE_WINO_BLOCK1, SEDX_TUNE_WINO_F43, SEDX_TUNE_WINO_ORDER
# (200, 1001) and (600, 1001) split stage 2 under F(4x4)'s byte and F(2x2)'s element limit
EXTRA = [(32, 1001), (32, 994), (72, 136), (4, 1001), (7, 1001), (1, 1001), (64, 1001), (200, 1001), (600, 1001)]
FORMS = [s for s in SWEEP_SHAPES if s[0] == 1] + [(8, 136), (16, 37), (32, 1001), (72, 136)]


def cases():
    """(block1, f43, order, ncu, B, T) in file order."""
    out = [DEFAULT + (256, B, T) for (B, T) in list(SWEEP_SHAPES) + EXTRA]
    out += [(b1, f43, order, 256, B, T) for f43 in range(3) for b1 in range(3) for order in range(3)
            for (B, T) in FORMS]
    out += [DEFAULT + (ncu, B, T) for ncu in (64, 304) for (B, T) in FORMS]
    return out


def record(L, path):
    cfg = _lib.SedxConfig(0, 0, 16000, 512, 160, 64, 50.0, 7000.0, 25)
    h = ctypes.c_void_p()
    assert L.sedx_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    L.sedx_dbg_conv.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_char_p]
    for (b1, f43, order, ncu, B, T) in cases():
        for knob, v in ((_lib.TUNE_WINO_BLOCK1, b1), (_lib.TUNE_WINO_F43, f43), (_lib.TUNE_WINO_ORDER, order)):
            assert L.sedx_set_tuning(h, knob, v) == 0
        assert L.sedx_dbg_conv(h, B, T, ncu, path.encode()) == 0
    L.sedx_destroy(h)


def parse(path):
    """The log -> one list of launch rows (COLUMNS order) per 'Q' line."""
    per_case = []
    for line in open(path):
        f = line.split()
        if f[0] == 'Q':
            per_case.append((tuple(int(x) for x in f[1:]), []))
            continue
        stage, fam, bs, T, F, cin, cout, epi, _order, tg, nt, c4, tb, ngroups, nitems, nwg, claim, o2d, bmax = (
            int(x) for x in f[1:])
        per_case[-1][1].append([stage, fam, bs, T, F, cin, cout, epi, tg, nt, c4, tb, ngroups, nitems, nwg, claim, o2d,
                                bmax])
    return per_case


if __name__ == '__main__':
    # not _lib.lib(): the baseline library has none of the later entry points
    L = ctypes.CDLL(os.path.abspath(sys.argv[1]))
    L.sedx_create.argtypes = [ctypes.POINTER(_lib.SedxConfig), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.sedx_set_tuning.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    L.sedx_destroy.argtypes = [ctypes.c_void_p]
    log = os.path.join(tempfile.mkdtemp(), 'launches.log')
    record(L, log)
    per_case = parse(log)
    want = cases()
    assert len(per_case) == len(want)
    pool, out_cases = {}, []
    for (b1, f43, order, ncu, B, T), (q, rows) in zip(want, per_case):
        assert q == (2, b1, f43, order, B, T, ncu), (q, b1, f43, order, B, T, ncu)
        ids = [pool.setdefault(tuple(r), len(pool)) for r in rows]
        out_cases.append([b1, f43, order, ncu, B, T, ids])
    out = os.path.join(REPO, 'tests', 'golden', 'conv_launches.json')
    with open(out, 'w') as f:
        f.write('{"columns": %s,\n "case_columns": ["wino_block1", "wino_f43", "wino_order", "ncu", "B", "T", "rows"],\n'
                % json.dumps(COLUMNS))
        f.write(' "rows": [\n  ' + ',\n  '.join(json.dumps(list(r)) for r in pool) + '\n ],\n')
        f.write(' "cases": [\n  ' + ',\n  '.join(json.dumps(c) for c in out_cases) + '\n ]}\n')
    print('%d cases, %d distinct launch rows -> %s (%d bytes)' % (len(out_cases), len(pool), out, os.path.getsize(out)))
