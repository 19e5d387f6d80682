"""Stage times of the two 14-layer models against a torch eager baseline.

For Cnn_14layers_Gru_FrameAtt and Cnn_14layers_Transformer_FrameAtt at
B = 32 x 10 s and B = 1 x 10 s: every stage of ``sedx_stage_times`` (profiling
mode 1: the last forward's HIP events) averaged over ``--forwards`` forwards,
``--repeats`` times, and the whole forward (waveform in, outputs out) timed
with device events over the same forwards.  On a 14-layer handle stage 8 spans
block 4's conv2 and the four launches of blocks 5-6 (csrc/conv_deep.hip: 18.8
GFLOP per 10 s clip) and stage 9 is the sequence layer alone (GRU: the input
projection + 31 recurrence launches).

Baseline, same session and device: the fp32 torch restatement of
tests/deep14_refs.py (bn0, the 12 convolutions with their BatchNorms and
pools, the sequence layer, AttBlock) run eagerly on the GPU from the log-mel
features the library computed (so the baseline does not pay for a frontend),
with ``torch.nn.GRU`` as the recurrence; device events after warm-up.

Prints one JSON line.

Usage:  python tools/deep14_stage_times.py [--forwards 30] [--repeats 3]
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

import deep14_refs as D  # noqa: E402
from sedx import _lib, models, synth  # noqa: E402

P16 = (16000, 512, 160, 64, 25, 7000)
# direct-conv FLOP of stage 8's five launches per 10 s clip (T3 = 125, T4 = 62, T5 = 31)
DEEP_GFLOP = 2e-9 * 9 * (125 * 8 * 512 * 512 + 62 * 4 * (512 * 1024 + 1024 * 1024) + 31 * 2 * (1024 * 2048 + 2048 * 2048))


def build(mt):
    m = getattr(models, mt)(*P16, 25, 'logmel')
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, seed=D.SEEDS[mt]).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval()


def timed(fn, forwards, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.no_grad():
            for _ in range(forwards):
                fn()
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b) / forwards, 4))
    return out


def stage_times(m, wave, forwards, repeats):
    """Per repeat: the per-stage means in ms."""
    nat, L = m.native(wave.device), _lib.lib()
    n_st = len(_lib.STAGES)
    with torch.no_grad():
        for _ in range(3):
            m(wave)
    torch.cuda.synchronize()
    _lib.check(L.sedx_set_profiling(nat.h, 1), nat.h, 'set_profiling')
    out = []
    for _ in range(repeats):
        acc = np.zeros(n_st)
        for _ in range(forwards):
            with torch.no_grad():
                m(wave)
            ms, n = (ctypes.c_float * n_st)(), ctypes.c_int32()
            _lib.check(L.sedx_stage_times(nat.h, ms, n_st, ctypes.byref(n)), nat.h, 'stage_times')
            acc += np.array(ms[:])
        out.append([round(float(v / forwards), 4) for v in acc])
    _lib.check(L.sedx_set_profiling(nat.h, 0), nat.h, 'set_profiling')
    return out


def stage0(m, wave):
    """The library's bn0 output [B, T, 64] -> the features [B, 64, T] it stands for are not
    needed: the baseline starts from stage 0 itself, [B, 1, T, 64]."""
    nat, L = m.native(wave.device), _lib.lib()
    T = wave.shape[1] // 160 + 1
    buf = torch.empty((wave.shape[0], T, 64), dtype=torch.float32, device=wave.device)
    _lib.check(L.sedx_set_capture(nat.h, 0, ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4), nat.h, 'capture')
    with torch.no_grad():
        m(wave)
    torch.cuda.synchronize()
    _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'capture')
    return buf[:, None].contiguous()


def eager_model(mt, dev):
    """x0 [B, 1, T, 64] -> the three outputs: deep14_refs' steps in fp32 on the device."""
    sd = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in D.state(mt, torch.float32).items()}
    gru = None
    if mt == D.GRU14:
        gru = torch.nn.GRU(2048, 1024, num_layers=1, bias=True, batch_first=True, bidirectional=True).to(dev).eval()
        gru.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith('gru.')}, strict=True)
    steps = [fn for _, _, _, fn in D.conv_steps()]

    def fwd(x):
        for fn in steps:
            x = fn(sd, x)
        x = gru(x.transpose(1, 2))[0] if gru is not None else D.step_seq(sd, mt, x)
        return D.step_head(sd, mt, x)
    return fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--forwards', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    res = {'forwards': args.forwards, 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0),
           'stages': list(_lib.STAGES), 'deep_gflop_per_clip': round(DEEP_GFLOP, 3)}
    for mt in (D.GRU14, D.TRF14):
        m = build(mt)
        base = eager_model(mt, torch.device('cuda'))
        for B in (32, 1):
            wave = torch.from_numpy(synth.make_waveforms(B, seconds=10.0, sample_rate=16000, seed=1234)).cuda()
            st = stage_times(m, wave, args.forwards, args.repeats)
            x0 = stage0(m, wave)
            with torch.no_grad():
                ref = base(x0)
                got = m(wave)
                for _ in range(2):
                    base(x0)
            torch.cuda.synchronize()
            res['%s/B%d' % (mt, B)] = {
                'stage_ms': st,
                'deep_tflops': [round(B * DEEP_GFLOP / s[8], 2) for s in st],
                'forward_ms': timed(lambda: m(wave), args.forwards, args.repeats),
                'torch_eager_ms': timed(lambda: base(x0), args.forwards, args.repeats),
                'max_abs_framewise_vs_eager': float((got['framewise_output'] - ref['framewise_output']).abs().max()),
            }
        del m, base
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
