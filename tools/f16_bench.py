"""Speed and accuracy of the fp16 conv stack (SEDX_PRECISION_F16) against the
two fastest existing precision modes, in one process.

Workload: Cnn_9layers_Gru_FrameAtt, 16 kHz, B = 32 x 10 s.  'winograd', 'x3'
and 'f16' alternate round by round on one handle; per round and mode a warm-up,
then the mean of --forwards forwards (HIP events) and, from sedx_stage_times,
the conv stack alone (stages b1c1 .. b4c2).  Reported: the median over the
rounds and the spread (min, max) per mode.  Before timing, the end-to-end bound
of tests/test_gpu_f16.py is checked on the timed batch's first --check-clips
clips: max|G - E_out| <= d_q per output key, E_out the chained emulation of
tests/f16_refs.py on the GPU's own stage 0.

The bar: 'f16' beats the faster of 'winograd' and 'x3' by more than the
recorded spread (the larger of the two modes' max - min), for the forward and
for the conv stack.  The verdict is recorded, not asserted.

Accuracy, recorded and not asserted (synthetic weights: the event margins are
arbitrary): on the golden 10 s clips, max|framewise('f16') - fp32 oracle| and
the number of events that differ from the events of the oracle's framewise.

    python tools/f16_bench.py [--rounds 7] [--forwards 10] [--out profiles/f16_bench_mi355x.json]
    python tools/f16_bench.py --only f16 --forwards 20      (a plain run of one mode, for a profiler)
    python tools/f16_bench.py --attach kernel_stats_f16=FILE sq_summary=FILE ...
        (no GPU: embeds profiler outputs, rocprofv3's kernel stats and tools/sq_summary.py's table, as text under
        "traces" of the existing --out file)
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, 'sound-event-detection_amd'), os.path.join(REPO, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import f16_refs as H  # noqa: E402
from oracle import layer_refs as R  # noqa: E402
from sedx import _lib, inference, models, synth  # noqa: E402

GRU, TRF = R.GRU, R.TRF
SEEDS = {GRU: 0, TRF: 1}
P16 = (16000, 512, 160, 64, 25, 7000)
MODES = ('winograd', 'x3', 'f16')
CONV = slice(1, 9)      # b1c1 .. b4c2 of _lib.STAGES


def build(mt):
    m = getattr(models, mt)(*P16, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, seed=SEEDS[mt]).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval()


def forward_ms(m, wave, forwards):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        for _ in range(2):
            m(wave)
        torch.cuda.synchronize()
        a.record()
        for _ in range(forwards):
            m(wave)
        b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / forwards


def conv_ms(m, wave, forwards):
    nat, L, n_st = m.native(wave.device), _lib.lib(), len(_lib.STAGES)
    _lib.check(L.sedx_set_profiling(nat.h, 1), nat.h, 'set_profiling')
    acc = np.zeros(n_st)
    try:
        for _ in range(forwards):
            with torch.no_grad():
                m(wave)
            ms, n = (ctypes.c_float * n_st)(), ctypes.c_int32()
            _lib.check(L.sedx_stage_times(nat.h, ms, n_st, ctypes.byref(n)), nat.h, 'stage_times')
            acc += np.array(ms[:])
    finally:
        _lib.check(L.sedx_set_profiling(nat.h, 0), nat.h, 'set_profiling')
    return float(acc[CONV].sum() / forwards), [round(float(v / forwards), 4) for v in acc]


def check_bound(m, wave, clips):
    """max|G - E_out| <= d_q on the first clips of the timed batch."""
    w = wave[:clips].contiguous()
    nat, L = m.native(w.device), _lib.lib()
    T = w.shape[1] // 160 + 1
    buf = torch.empty((clips, T, 64), dtype=torch.float32, device=w.device)
    m.set_precision('f16')
    _lib.check(L.sedx_set_capture(nat.h, 0, ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4), nat.h, 'capture')
    try:
        with torch.no_grad():
            G = {k: v.cpu().numpy().astype(np.float64) for k, v in m(w).items()}
        torch.cuda.synchronize()
    finally:
        _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'capture')
    x0 = buf.cpu()[:, None].double()
    sd = R.state(GRU, 25, SEEDS[GRU], torch.float64)
    with torch.no_grad():
        e, r = H.chain(sd, GRU, x0), R.chain(sd, GRU, x0)
    out = {}
    for k in H.KEYS:
        dq = float((e[k] - r[k]).abs().max())
        d = float(np.abs(G[k] - e[k].numpy()).max())
        out[k] = {'max_abs_G_minus_E': d, 'd_q': dq, 'ratio': d / dq, 'within': bool(d <= dq)}
    return out


def accuracy():
    """'f16' on the golden 10 s clips against the fp32 oracle's recorded outputs."""
    tables = json.load(open(os.path.join(REPO, 'tests', 'golden', 'events.json')))
    wave = torch.from_numpy(synth.make_waveforms(2, seconds=10.0, sample_rate=16000, seed=1234)).cuda()
    out = {}
    for mt in (GRU, TRF):
        g = np.load(os.path.join(REPO, 'tests', 'golden', 'clip10s_%s.npz' % mt))['framewise_output']
        m = build(mt)
        rec = {}
        for mode in ('exact', 'f16'):
            with torch.no_grad():
                fw = m.set_precision(mode)(wave)['framewise_output'].cpu().numpy()
            ev = [json.dumps(e, sort_keys=True) for e in inference.events_from_framewise(fw.copy(), tables['params_default'])]
            ref = [json.dumps(e, sort_keys=True) for e in inference.events_from_framewise(g.copy(), tables['params_default'])]
            rec[mode] = {'max_abs_framewise_vs_oracle': float(np.abs(fw.astype(np.float64) - g).max()),
                         'events': len(ev), 'oracle_events': len(ref),
                         'events_differing': len(set(ev) ^ set(ref))}
        out[mt] = rec
        del m
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--forwards', type=int, default=10)
    ap.add_argument('--check-clips', type=int, default=2)
    ap.add_argument('--only', default=None, help='run --forwards forwards of one mode and exit (profiler runs)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'f16_bench_mi355x.json'))
    ap.add_argument('--attach', nargs='+', default=None, metavar='NAME=FILE')
    args = ap.parse_args()
    if args.attach:
        res = json.load(open(args.out))
        res.setdefault('traces', {})
        for item in args.attach:
            name, path = item.split('=', 1)
            res['traces'][name] = open(path).read().splitlines()
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')
        return
    wave = torch.from_numpy(synth.make_waveforms(32, seconds=10.0, sample_rate=16000, seed=4321)).cuda()
    m = build(GRU)
    if args.only:
        print(json.dumps({'mode': args.only, 'forward_ms': forward_ms(m.set_precision(args.only), wave, args.forwards)}))
        return
    res = {'device': torch.cuda.get_device_name(0), 'model': GRU, 'batch': 32, 'seconds': 10.0,
           'rounds': args.rounds, 'forwards': args.forwards, 'stages': list(_lib.STAGES),
           'bound_check': check_bound(m, wave, args.check_clips)}
    fwd = {k: [] for k in MODES}
    conv = {k: [] for k in MODES}
    stages = {}
    for _ in range(args.rounds):
        for mode in MODES:
            m.set_precision(mode)
            fwd[mode].append(forward_ms(m, wave, args.forwards))
            c, st = conv_ms(m, wave, max(3, args.forwards // 2))
            conv[mode].append(c)
            stages[mode] = st
    summ = lambda v: {'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4),  # noqa: E731
                      'rounds': [round(x, 4) for x in v]}
    res['forward_ms'] = {k: summ(v) for k, v in fwd.items()}
    res['conv_stack_ms'] = {k: summ(v) for k, v in conv.items()}
    res['stage_ms_last_round'] = stages
    res['bar'] = {}
    for name, t in (('forward', res['forward_ms']), ('conv_stack', res['conv_stack_ms'])):
        best = min(('winograd', 'x3'), key=lambda k: t[k]['median'])
        spread = max(t['f16']['max'] - t['f16']['min'], t[best]['max'] - t[best]['min'])
        margin = t[best]['median'] - t['f16']['median']
        res['bar'][name] = {'best_other': best, 'margin_ms': round(margin, 4), 'spread_ms': round(spread, 4),
                            'speedup': round(t[best]['median'] / t['f16']['median'], 4), 'met': bool(margin > spread)}
    del m
    torch.cuda.empty_cache()
    res['accuracy_golden_clips'] = accuracy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps({'bar': res['bar'], 'forward_ms': {k: v['median'] for k, v in res['forward_ms'].items()},
                      'conv_stack_ms': {k: v['median'] for k, v in res['conv_stack_ms'].items()},
                      'bound_check': res['bound_check']}))


if __name__ == '__main__':
    main()
