"""Stage times of the three VGGish models against a torch eager baseline.

At B = 32 x 10 s and B = 1 x 10 s (16 kHz preset): every stage of
``sedx_stage_times`` (profiling mode 1: the last forward's HIP events) averaged
over ``--forwards`` forwards, ``--repeats`` times, and the whole forward
(waveform in, outputs out) timed with device events over the same forwards.
Stage 1 is conv1 with its pool (csrc/conv_vgg.hip), stages 2-6 the launches of
conv2, conv3_1, conv3_2, conv4_1 and conv4_2 on the exact fp32 kernel, 7 and 8
are empty, 9 is the GRU, 10 the head.

Baseline, same session and device: the fp32 torch restatement of
tests/vggish_refs.py (``F.conv2d`` + ReLU + ``F.max_pool2d``, the mean, an
``nn.GRU`` with the same weights, the head and the framewise expansion) run
eagerly on the GPU from the log-mel the library computed (so the baseline does
not pay for a frontend); device events after warm-up.

Per conv launch: the FLOPs it executes (2 x 9 Cin Cout per output pixel of the
T x F image, whatever the epilogue keeps) over its stage time, as a fraction of
the 157.3 TFLOP/s fp32 matrix peak, beside the exact launch of the same
(F, Cin, Cout) triple in the 9-layer GRU model under ``set_precision('exact')``
(stages 3 and 5-8 there: b2c1, b3c1, b3c2, b4c1, b4c2), timed the same way.  The first layer: bytes
written by its one launch against the 9-layer ``conv1_c4_kernel``'s
full-resolution activation, and the write rate stage 1 reaches.

Prints one JSON line (kept as profiles/vggish_stage_times.json).

Usage:  python tools/vggish_stage_times.py [--forwards 30] [--repeats 3]
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, 'sound-event-detection_amd'), os.path.join(REPO, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vggish_refs as V  # noqa: E402
from deep14_stage_times import stage_times, timed  # noqa: E402
from sedx import _lib, models, synth  # noqa: E402

PEAK_TFLOPS = 157.3
# conv l of the VGGish trunk -> the 9-layer model's stage with the same (F, Cin, Cout): b2c1, b3c1, b3c2, b4c1, b4c2
# (b2c2, stage 4, is 128 -> 128 at F = 32: no VGGish layer has that triple)
EXACT9_STAGE = {1: 3, 2: 5, 3: 6, 4: 7, 5: 8}
T10 = 1001


def build(mt):
    m = getattr(models, mt)(*V.ctor_args(None))
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, seed=V.SEEDS[mt]).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval()


def build_gru9():
    mt = 'Cnn_9layers_Gru_FrameAtt'
    m = getattr(models, mt)(*V.P16, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval().set_precision('exact')


def stage0(m, wave):
    """The library's log-mel [B, T, 64]: the baseline's input."""
    nat, L = m.native(wave.device), _lib.lib()
    T = wave.shape[1] // 160 + 1
    buf = torch.empty((wave.shape[0], T, 64), dtype=torch.float32, device=wave.device)
    _lib.check(L.sedx_set_capture(nat.h, 0, ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4), nat.h, 'capture')
    with torch.no_grad():
        m(wave)
    torch.cuda.synchronize()
    _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'capture')
    return buf


def eager_model(mt, dev):
    """x0 [B, T, 64] -> the three outputs: vggish_refs' steps in fp32 on the device."""
    sd = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in V.state(mt, torch.float32).items()}
    gru = None
    if mt == V.GRU:
        gru = torch.nn.GRU(512, 256, num_layers=1, bias=True, batch_first=True, bidirectional=True).to(dev).eval()
        gru.load_state_dict({k[len('gru.'):]: v for k, v in sd.items() if k.startswith('gru.')})

    def fwd(x0):
        s8 = V.trunk(sd, x0)[8]
        s9 = gru(s8)[0] if gru is not None else s8
        return V.step_head(sd, mt, s9)
    return fwd


def conv_gflop(B):
    """GFLOP each of the six conv launches executes on B 10 s clips."""
    T1, T2, T3 = T10 // 2, T10 // 4, T10 // 8
    px = [T10 * 64, T1 * 32, T2 * 16, T2 * 16, T3 * 8, T3 * 8]
    return [2.0 * 9 * cin * cout * p * B / 1e9 for (_, cin, cout, _), p in zip(V.CONVS, px)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--forwards', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    res = {'forwards': args.forwards, 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0),
           'stages': ['frontend', 'conv1', 'conv2', 'conv3_1', 'conv3_2', 'conv4_1', 'conv4_2', '-', '-', 'seq', 'head',
                      'pipeline_wait'], 'peak_tflops_fp32_matrix': PEAK_TFLOPS}
    waves = {B: torch.from_numpy(synth.make_waveforms(B, seconds=10.0, sample_rate=16000, seed=1234)).cuda() for B in (32, 1)}
    # the existing exact launches of the same (F, Cin, Cout) triples: the 9-layer GRU model's stages 3-8
    g9 = build_gru9()
    exact9 = {B: np.median(np.array(stage_times(g9, waves[B], args.forwards, args.repeats)), axis=0) for B in (32, 1)}
    del g9
    for mt in V.MODELS:
        m = build(mt)
        base = eager_model(mt, torch.device('cuda'))
        for B in (32, 1):
            wave = waves[B]
            st = stage_times(m, wave, args.forwards, args.repeats)
            x0 = stage0(m, wave)
            with torch.no_grad():
                ref = base(x0)
                got = m(wave)
                for _ in range(2):
                    base(x0)
            torch.cuda.synchronize()
            med = np.median(np.array(st), axis=0)
            gf = conv_gflop(B)
            launches = {}
            for l, name in enumerate(('conv1', 'conv2', 'conv3_1', 'conv3_2', 'conv4_1', 'conv4_2')):
                ms = float(med[1 + l])
                row = {'gflop': round(gf[l], 3), 'ms': round(ms, 4),
                       'fraction_of_peak': round(gf[l] / ms / PEAK_TFLOPS, 4) if ms > 0 else None}
                if l >= 1:   # the 9-layer model's exact launch of the same triple (same pixels, same FLOPs)
                    ms9 = float(exact9[B][EXACT9_STAGE[l]])
                    row['exact9_ms'] = round(ms9, 4)
                    row['exact9_fraction_of_peak'] = round(gf[l] / ms9 / PEAK_TFLOPS, 4) if ms9 > 0 else None
                launches[name] = row
            wrote = B * (T10 // 2) * 32 * 64 * 4
            res['%s/B%d' % (mt, B)] = {
                'stage_ms': st,
                'forward_ms': timed(lambda: m(wave), args.forwards, args.repeats),
                'torch_eager_ms': timed(lambda: base(x0), args.forwards, args.repeats),
                'max_abs_framewise_vs_eager': float((got['framewise_output'] - ref['framewise_output']).abs().max()),
                'conv_launches': launches,
                'conv1_bytes_written': wrote,
                'conv1_c4_kernel_bytes_written': B * T10 * 64 * 64 * 4,
                'conv1_write_GBps': round(wrote / (float(med[1]) * 1e-3) / 1e9, 1) if med[1] > 0 else None,
            }
        del m, base
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
