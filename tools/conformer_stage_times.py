"""Sequence-layer and head time of the four kinds of model, one batch at a time.

For Cnn_9layers_Gru_FrameAtt, Cnn_9layers_Transformer_FrameAtt and the two
Conformer models: stage 9 (GRU / MultiHead / the whole Conformer encoder) and
stage 10 (head) of ``sedx_stage_times`` (profiling mode 1: the last forward's
HIP events), averaged over ``--forwards`` forwards, ``--repeats`` times, at
B = 32 x 10 s and B = 1.  Then the baseline of the Conformer encoder: the fp32
torch restatement of tests/conformer_refs.py run eagerly on the same device on
the stage-8 tensor the library captured, timed with HIP events over the same
number of forwards.  Prints one JSON line.

Usage:  python tools/conformer_stage_times.py [--forwards 30] [--repeats 3]
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

import conformer_refs as CR  # noqa: E402
from sedx import _lib, models, synth  # noqa: E402

GRU, TRF = 'Cnn_9layers_Gru_FrameAtt', 'Cnn_9layers_Transformer_FrameAtt'
P16 = (16000, 512, 160, 64, 25, 7000)


def build(mt):
    args = P16 + ((25, 'logmel') if mt in (GRU, TRF) else (25,))
    m = getattr(models, mt)(*args)
    sd = m.state_dict()
    for k, v in synth.make_state_dict(mt, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval()


def stage_times(m, wave, forwards, repeats):
    """[(stage 9 ms, stage 10 ms)] per repeat."""
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
        out.append((round(float(acc[9] / forwards), 4), round(float(acc[10] / forwards), 4)))
    _lib.check(L.sedx_set_profiling(nat.h, 0), nat.h, 'set_profiling')
    return out


def stage8(m, wave):
    nat, L = m.native(wave.device), _lib.lib()
    fr, sl = m.output_geometry(wave.shape[1])
    buf = torch.empty((wave.shape[0], sl, 512), dtype=torch.float32, device=wave.device)
    _lib.check(L.sedx_set_capture(nat.h, 8, ctypes.c_void_p(buf.data_ptr()), buf.numel() * 4), nat.h, 'capture')
    with torch.no_grad():
        m(wave)
    torch.cuda.synchronize()
    _lib.check(L.sedx_set_capture(nat.h, -1, None, 0), nat.h, 'capture')
    return buf


def eager_encoder(mt, s8, forwards, repeats):
    """ms per forward of the fp32 torch restatement of the encoder, eager, on the device."""
    sd = {k: (v.to(s8.device) if isinstance(v, torch.Tensor) else v) for k, v in CR.state(mt, seed=0).items()}
    with torch.no_grad():
        for _ in range(3):
            CR.encoder(sd, s8)
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.no_grad():
            for _ in range(forwards):
                CR.encoder(sd, s8)
        b.record()
        torch.cuda.synchronize()
        out.append(round(a.elapsed_time(b) / forwards, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--forwards', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    res = {'forwards': args.forwards, 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0)}
    for B in (32, 1):
        wave = torch.from_numpy(synth.make_waveforms(B, seconds=10.0, sample_rate=16000, seed=1234)).cuda()
        for mt in (GRU, TRF, CR.CATT, CR.CAVG):
            m = build(mt)
            key = '%s/B%d' % (mt, B)
            res[key] = {'stage9_10_ms': stage_times(m, wave, args.forwards, args.repeats)}
            if mt in CR.MODELS:
                res[key]['torch_eager_encoder_ms'] = eager_encoder(mt, stage8(m, wave), args.forwards, args.repeats)
            del m
    print(json.dumps(res))


if __name__ == '__main__':
    main()
