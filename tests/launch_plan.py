"""What the conv launchers decide, read from ``sedx_conv_launch_plan`` (the plan
function the launchers call, asked for a CU count: no GPU needed), and the names
of the four F(4x4,3x3) launch regimes.  One handle, default tuning: the CNN
trunk is the same for all nine models."""
import ctypes

W43_REGIMES = ('nt4_static', 'nt4_claim', 'nt1_tg2', 'nt1_tg1')
_handle = None


def _h():
    global _handle
    from sedx import _lib
    if _handle is None:
        cfg = _lib.SedxConfig(0, 0, 16000, 512, 160, 64, 50.0, 7000.0, 25)
        _handle = ctypes.c_void_p()
        assert _lib.lib().sedx_create(ctypes.byref(cfg), 0, ctypes.byref(_handle)) == 0
    return _handle


def conv_launches(B, T, ncu, tuning=(), capacity=64):
    """(status, one dict per conv launch of stages 2-8) of a forward of [B, 64, T];
    ``tuning``: (knob, value) pairs for this call, the default restored after it."""
    from sedx import _lib
    L, h = _lib.lib(), _h()
    default = {_lib.TUNE_WINO_BLOCK1: 2, _lib.TUNE_WINO_F43: 2, _lib.TUNE_WINO_ORDER: 1}
    rows, n = (_lib.SedxConvLaunch * capacity)(), ctypes.c_int32()
    try:
        for knob, v in tuning:
            assert knob in default and L.sedx_set_tuning(h, knob, v) == 0
        st = L.sedx_conv_launch_plan(h, B, (T - 1) * 160, ncu, rows, capacity, ctypes.byref(n))   # hop 160
    finally:
        for knob, v in default.items():
            assert L.sedx_set_tuning(h, knob, v) == 0
    return st, [{f: getattr(r, f) for f, _ in r._fields_} for r in rows[:min(n.value, capacity)]]


def w43_launch(layer, B, T, ncu):
    """Launch ``layer`` (0..6) of a default forward (all F(4x4,3x3), unsplit) with its regime."""
    st, rows = conv_launches(B, T, ncu)
    assert st == 0 and len(rows) == 7 and all(r['family'] == 4 for r in rows), (st, rows)
    r = rows[layer]
    r['regime'] = 'nt1_tg1' if r['tg'] == 1 else 'nt1_tg2' if r['nt'] == 1 else 'nt4_claim' if r['claim'] else 'nt4_static'
    return r


def w43_regime(layer, B, T, ncu):
    return w43_launch(layer, B, T, ncu)['regime']


def w43_reachable(layer):
    """Regimes launch ``layer`` can run in: 16-tile items exist for F = 16 / 8."""
    return set(W43_REGIMES) if w43_launch(layer, 1, 64, 256)['F'] in (16, 8) else set(W43_REGIMES) - {'nt1_tg1'}


def w43_missing(shapes, ncu):
    """(layer, regime) pairs a launch can reach and no (B, T) of ``shapes`` runs."""
    seen = {(l, w43_regime(l, B, T, ncu)) for (B, T) in shapes for l in range(7)}
    return sorted((l, r) for l in range(7) for r in w43_reachable(l) if (l, r) not in seen)
