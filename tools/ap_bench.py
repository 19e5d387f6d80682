"""Device time of the average-precision ranking (sedx.evaluate.average_precision,
csrc/rank.hip) against sklearn.metrics.average_precision_score on the host CPU
of the same machine, on the same arrays.  Not part of bench.py.

Two shapes: [488 000, 25] (the testing set's framewise size: 488 clips x 1000
frames, scores repeated x8 along the frames as the models' interpolation
produces) and [20 000, 527] (an AudioSet-sized clipwise set).

  device_ms    HIP events around `reps` back-to-back calls of the device entry
               on one stream (inputs resident, workspace allocated, after
               warm-up), divided by reps: the ranking's device time
  call_ms      host clock around evaluate.average_precision on a HIP tensor,
               read-back of ap / info included (ends in a synchronise)
  sklearn_ms   host clock around average_precision_score(average=None)
  max_abs_diff the largest |ap - sklearn| over the classes, at the timed size

Needs a HIP device: there is no fallback.  Prints one JSON line per shape.

Usage:  python tools/ap_bench.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(REPO, 'sound-event-detection_amd')]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.metrics import average_precision_score  # noqa: E402

from sedx import _lib, evaluate  # noqa: E402

SHAPES = [('framewise_488x1000x25', 488000, 25, 8), ('clipwise_20000x527', 20000, 527, 1)]


def make(M, C, repeat, seed):
    rng = np.random.RandomState(seed)
    s = np.repeat(rng.rand((M + repeat - 1) // repeat, C).astype(np.float32), repeat, axis=0)[:M]
    t = (rng.rand(M, C) < 0.1).astype(np.uint8)
    t[0, :] = 1
    return np.ascontiguousarray(t), np.ascontiguousarray(s)


def device_ms(t, s, reps, warmup):
    L = _lib.lib()
    M, C = s.shape
    dt, ds = torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda()
    wsz = ctypes.c_size_t()
    _lib.check(L.sedx_average_precision_workspace_size(M, C, ctypes.byref(wsz)), None, 'workspace_size')
    ws = torch.empty(wsz.value, dtype=torch.uint8, device='cuda')
    out = torch.empty(4 * C, dtype=torch.int64, device='cuda')
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    null = ctypes.c_void_p(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(L.sedx_average_precision_device(p(ds), p(dt), M, C, p(out), p(out[C:]), null, null, null, p(ws),
                                                   ws.numel(), stream), None, 'average_precision_device')
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, wsz.value, ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ap_bench: no HIP device (there is no fallback)')
    rows = []
    for name, M, C, repeat in SHAPES:
        t, s = make(M, C, repeat, 7)
        dev_ms, ws_bytes, ds = device_ms(t, s, args.reps, args.warmup)
        calls = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = evaluate.average_precision(t, ds)
            calls.append((time.perf_counter() - t0) * 1e3)
        sk_ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            sk = average_precision_score(t, s, average=None)
            sk_ms.append((time.perf_counter() - t0) * 1e3)
        row = {'shape': name, 'M': M, 'C': C, 'device_ms': round(dev_ms, 4), 'call_ms': round(min(calls), 3),
               'sklearn_ms': round(min(sk_ms), 1), 'sklearn_over_device': round(min(sk_ms) / dev_ms, 1),
               'sklearn_over_call': round(min(sk_ms) / min(calls), 1), 'workspace_MiB': round(ws_bytes / 2.0 ** 20, 1),
               'max_abs_diff': float(np.max(np.abs(got - sk))), 'reps': args.reps,
               'host_threads': int(os.environ.get('OMP_NUM_THREADS', 0)) or None,
               'device': torch.cuda.get_device_name(0)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
