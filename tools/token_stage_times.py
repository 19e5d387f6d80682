"""Stage times of Cnn_9layers_Conformer against a torch eager baseline, and the
A/B of its two attention kernels, on the pattern of
``tools/conformer14_stage_times.py`` (``tools/deep14_stage_times.py``'s helpers).

Default mode.  At B = 32 x 10 s and B = 1 x 10 s (1001 tokens per clip), under
SEDX_TUNE_CF_ATTN 0 (four lanes per query) and 1 (the fp32 matrix pipe): every
stage of ``sedx_stage_times`` averaged over ``--forwards`` forwards, ``--repeats``
times, and the whole forward timed with device events.  Stage 8 is block 4's
conv2 plus the token kernel, 9 the encoder, 10 the classifier and the split.
Baseline (context only), same session and device: the fp32 torch restatement
(``oracle/layer_refs.py``'s conv steps, ``tests/token_refs.py``) run eagerly on the
GPU from the library's bn0 output.  Prints one JSON line.

``--profile-run KNOB``: ``--forwards`` forwards of B = 32 x 10 s under that knob
after two warm-up forwards and nothing else -- the program a
``rocprofv3 --kernel-trace --stats`` run of its own wraps.
``--summarise DIR...``: reads the ``*kernel_stats.csv`` of such runs (directory
names ``k<KNOB>_r<REPEAT>``) and prints, per knob and repeat, the summed device
time per forward of the attention launches, of the encoder's GEMMs
(cf_gemm_kernel), of the conv stack and of everything else.

Usage:  python tools/token_stage_times.py [--forwards 20] [--repeats 3]
"""
import argparse
import csv
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, 'sound-event-detection_amd'), os.path.join(REPO, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

WARMUP = 2


def build(knob):
    import torch
    import token_refs as TR
    from sedx import _lib, models, synth
    m = models.Cnn_9layers_Conformer(*TR.P16, 25)
    sd = m.state_dict()
    for k, v in synth.make_state_dict(TR.TOKEN, seed=TR.SEEDS[TR.TOKEN]).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=True)
    return m.to('cuda').eval().set_tuning(_lib.TUNE_CF_ATTN, knob)


def eager_model(dev):
    """x0 [B, 1, T, 64] -> the two outputs, every step in fp32 on the device."""
    import torch
    import token_refs as TR
    from oracle import layer_refs as R
    sd = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in TR.state(torch.float32).items()}
    steps = [fn for _, dst, fn in R.conv_steps() if dst <= 7]

    def fwd(x):
        for fn in steps:
            x = fn(sd, x)
        x = x.permute(0, 2, 3, 1)                  # capture 7's layout [B, T3, 8, 512]
        for src, _ in TR.STEPS:
            x = TR.step(sd, src, x)
        return TR.head(sd, x)
    return fwd


def waves(B):
    import torch
    from sedx import synth
    return torch.from_numpy(synth.make_waveforms(B, seconds=10.0, sample_rate=16000, seed=1234)).cuda()


def measure(args):
    import torch
    import deep14_stage_times as S
    from sedx import _lib
    res = {'forwards': args.forwards, 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0),
           'stages': list(_lib.STAGES), 'model': 'Cnn_9layers_Conformer', 'tokens': 1001}
    base = eager_model(torch.device('cuda'))
    for B in (32, 1):
        wave = waves(B)
        row = {}
        for knob in (0, 1):
            m = build(knob)
            st = S.stage_times(m, wave, args.forwards, args.repeats)
            row['attn%d' % knob] = {'stage_ms': st, 'stage_8_9_10_ms': [[s[8], s[9], s[10]] for s in st],
                                    'forward_ms': S.timed(lambda: m(wave), args.forwards, args.repeats)}
        x0 = S.stage0(m, wave)
        with torch.no_grad():
            ref, got = base(x0), m(wave)
            base(x0)
        torch.cuda.synchronize()
        row['torch_eager_ms'] = S.timed(lambda: base(x0), max(2, args.forwards // 4), args.repeats)
        row['max_abs_framewise_vs_eager'] = float((got['framewise_output'] - ref['framewise_output']).abs().max())
        res['B%d' % B] = row
    print(json.dumps(res))


def profile_run(args):
    import torch
    m, wave = build(args.profile_run), waves(32)
    with torch.no_grad():
        for _ in range(WARMUP + args.forwards):
            m(wave)
    torch.cuda.synchronize()


def summarise(args):
    out = {}
    for d in args.summarise:
        tag = os.path.basename(os.path.normpath(d))
        files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not files:
            continue
        groups = {'attention': 0.0, 'cf_gemm': 0.0, 'conv': 0.0, 'rest': 0.0}
        calls = 0
        for r in csv.DictReader(open(files[0])):
            name, ns = r['Name'], float(r['TotalDurationNs'])
            if 'cf_relattn' in name:
                groups['attention'] += ns
                calls += int(r['Calls'])
            elif 'cf_gemm_kernel' in name:
                groups['cf_gemm'] += ns
            elif 'conv' in name and 'glu_dwconv' not in name:
                groups['conv'] += ns
            else:
                groups['rest'] += ns
        n = calls / 3.0                              # forwards in the trace, warm-up included: three launches each
        out[tag] = {k + '_ms_per_forward': round(v / n / 1e6, 4) for k, v in groups.items()}
        out[tag]['forwards'] = n
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--forwards', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--profile-run', type=int, default=None)
    ap.add_argument('--summarise', nargs='+', default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args)
    if args.profile_run is not None:
        return profile_run(args)
    measure(args)


if __name__ == '__main__':
    main()
