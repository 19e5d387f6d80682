"""What the conv launchers decide, read from ``sedx_conv_launch_plan`` (the plan
function the launchers call, asked for a CU count: no GPU needed), and the names
of the four F(4x4,3x3) launch regimes.  One handle, default tuning: the CNN
trunk is the same for all nine models.  And what the fp32 GEMM launcher of the
sequence layer and head decides, read from ``sedx_gemm_launch_plan``: one
handle per model type."""
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


# ---------------------------------------------------------------------------
# the GEMM launches of the sequence layer and the head
# ---------------------------------------------------------------------------
GRU9, GRU14, TRF14 = 0, 10, 11          # sedx_model_type (include/sedx.h)
GEMM_KERNELS = ('tiled', 'one_wave', 'ksplit', 'x3', 'conformer')
# the launches by name, in launch order
GEMM_NAMES = {GRU14: ('gru-proj', 'head'), TRF14: ('mha-qkv', 'mha-fc', 'head'), GRU9: ('gru-proj', 'head')}
_gemm_handles = {}


def gemm_handle(model_type):
    from sedx import _lib
    if model_type not in _gemm_handles:
        cfg = _lib.SedxConfig(model_type, 0, 16000, 512, 160, 64, 50.0, 7000.0, 25)
        h = ctypes.c_void_p()
        assert _lib.lib().sedx_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
        _gemm_handles[model_type] = h
    return _gemm_handles[model_type]


def gemm_launches(model_type, B, T, ncu, capacity=64, precision=None):
    """(status, one dict per GEMM launch of the sequence layer and head) of a
    forward of [B, 64, T]; ``kernel`` is the name in GEMM_KERNELS.  ``precision``
    ('x3', ...) for this call, the default restored after it."""
    from sedx import _lib
    L, h = _lib.lib(), gemm_handle(model_type)
    rows, n = (_lib.SedxGemmLaunch * max(capacity, 1))(), ctypes.c_int32()
    try:
        if precision is not None:
            assert L.sedx_set_precision(h, _lib.PRECISION[precision]) == 0
        st = L.sedx_gemm_launch_plan(h, B, (T - 1) * 160, ncu, rows if capacity else None, capacity, ctypes.byref(n))
    finally:
        assert L.sedx_set_precision(h, _lib.PRECISION['winograd']) == 0
    out = [{f: getattr(r, f) for f, _ in r._fields_} for r in rows[:min(n.value, capacity)]]
    for r in out:
        r['kernel'] = GEMM_KERNELS[r['kernel']]
    return st, out, n.value


def gemm_kernels(model_type, B, T, ncu):
    """{launch name: kernel name} of a forward of [B, 64, T] on ``ncu`` CUs."""
    st, rows, _ = gemm_launches(model_type, B, T, ncu)
    assert st == 0 and len(rows) == len(GEMM_NAMES[model_type]), (st, rows)
    return {name: r['kernel'] for name, r in zip(GEMM_NAMES[model_type], rows)}


def gemm_reachable(model_type, ncu, max_m=2048):
    """(launch, kernel) pairs the rule gives a 14-layer model for some M <= max_m
    (M = B clips of 32 frames: one sequence frame each)."""
    return {(name, k) for M in range(1, max_m + 1) for name, k in gemm_kernels(model_type, M, 32, ncu).items()}


def gemm_missing(shapes, ncu):
    """(model, launch, kernel) triples a 14-layer model's GEMM launch can reach
    and no (model, B, T) of ``shapes`` runs."""
    seen = {(mt, name, k) for mt, B, T in shapes for name, k in gemm_kernels(mt, B, T, ncu).items()}
    want = {(mt, name, k) for mt in (GRU14, TRF14) for name, k in gemm_reachable(mt, ncu)}
    return sorted(want - seen)
