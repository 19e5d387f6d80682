"""Windowed inference over recordings of different lengths: one predict_windows
call per file (the only way before the ragged driver) against ONE
predict_windows_ragged call over all of them.

N synthetic recordings (sedx.synth.make_waveforms) with durations drawn
uniformly from 5 .. 60 s by a fixed seed, Cnn_9layers_Gru_FrameAtt with seeded
weights at 16 kHz, the default precision, predict.py's arguments (5 s windows,
1 s stride, overlap_value 1).  Both sides end in a device synchronise (the
drivers sync and check the handle before they return), so a host clock around
the calls measures completed work.  Per repeat the two sides alternate, and
every call takes the recordings in another (rotated) order than the call before: the handle keeps
the last ragged plan, which one inference asks for three times, and a list
never seen before is the directory loop's real case.  The
medians, the spread (min, max) and their ratio go to the JSON, with the
device's name and the clocks rocm-smi reports after the run.  The outputs of
the two sides are compared bit for bit before anything is timed.

    python tools/ragged_bench.py --n 8 32 --chunks 64 256 0 --out profiles/ragged_bench_mi355x.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'sound-event-detection_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from sedx import inference, models, synth   # noqa: E402

MT = 'Cnn_9layers_Gru_FrameAtt'
SR = 16000


def build():
    m = getattr(models, MT)(SR, 512, 160, 64, 25, 7000, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(MT, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval()


def recordings(n, seed):
    rng = np.random.default_rng(seed)
    seconds = rng.uniform(5.0, 60.0, n)
    lengths = [int(s * SR) for s in seconds]
    return [torch.from_numpy(synth.make_waveforms(1, seconds=L / float(SR), sample_rate=SR, seed=seed + 1 + i)[0]).cuda()
            for i, L in enumerate(lengths)]


def per_file(m, clips):
    return [inference.predict_windows(m, c[None], 5, 1.0)[0] for c in clips]


def ragged(m, clips, k):
    return inference.predict_windows_ragged(m, (torch.cat(clips), [int(c.shape[0]) for c in clips]),
                                            max_windows_per_forward=k or None)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks', '--json'], capture_output=True, text=True, timeout=60)
        d = json.loads(r.stdout)
        card = sorted(d)[0]
        return {k: v for k, v in d[card].items() if 'sclk' in k or 'mclk' in k}
    except Exception as e:   # the tool is optional: the timings stand without it
        return {'unavailable': repr(e)}


def summary(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--chunks', type=int, nargs='+', default=[64, 256, 0], help='max windows per forward; 0: all at once')
    ap.add_argument('--seed', type=int, default=2024)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ragged_bench_mi355x.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ragged_bench needs a HIP device: a timing taken elsewhere says nothing')
    m = build()
    result = {'command': 'python tools/ragged_bench.py ' + ' '.join(sys.argv[1:]), 'model': MT, 'sample_rate': SR,
              'device': torch.cuda.get_device_name(0), 'warmup': a.warmup, 'repeats': a.repeats, 'seed': a.seed,
              'timing': 'host clock around calls that end in a device synchronise; the sides alternate per repeat, every '
                        'call on another rotation of the list than the call before',
              'cases': []}
    with torch.no_grad():
        for n in a.n:
            clips = recordings(n, a.seed)
            lengths = [int(c.shape[0]) for c in clips]
            nw = inference.ragged_window_geometry(m, lengths)[0]
            # every side takes the list of the repeat (the concatenation is part of the ragged side's time)
            sides = {'per_file': lambda cl: per_file(m, cl)}
            for k in a.chunks:
                sides['ragged_%s' % (k or 'all')] = (lambda cl, k=k: ragged(m, cl, k))
            ref = sides['per_file'](clips)
            identical = {name: all(torch.equal(x, y) for x, y in zip(fn(clips), ref)) for name, fn in sides.items()}
            for _ in range(a.warmup):
                for fn in sides.values():
                    fn(clips)
            ms = {name: [] for name in sides}
            calls = 0
            for _ in range(a.repeats):
                for name, fn in sides.items():
                    calls += 1                      # no two calls in a row on the same list
                    k = 1 + calls % (n - 1) if n > 2 else 0
                    order = clips[k:] + clips[:k]
                    ms[name].append(timed(lambda: fn(order))[0])
            case = {'n_files': n, 'seconds_total': sum(lengths) / float(SR), 'windows': int(sum(nw)),
                    'windows_per_file': {'min': min(nw), 'max': max(nw)}, 'bit_identical_to_per_file': identical,
                    'ms': {name: summary(v) for name, v in ms.items()}}
            base = case['ms']['per_file']['median_ms']
            case['per_file_over_ragged'] = {name: base / v['median_ms'] for name, v in case['ms'].items()
                                            if name != 'per_file'}
            result['cases'].append(case)
            print(json.dumps(case))
    result['clocks_after'] = clocks()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
