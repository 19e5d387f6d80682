"""Save a fixed forward's outputs (B=1 and B=32 of every chosen model and
precision) for bit-exactness checks between two builds of the package:
    python tools/ab_outputs.py out.npz --ab-package <pkg dir>
        [--models all | Name,Name,...] [--precisions winograd,exact,x3] [--gamma]
    python tools/ab_outputs.py --compare a.npz b.npz
The default is the two FrameAtt models at exact and x3; --gamma adds
Cnn_9layers_Gru_FrameAtt on gammatone features (32 kHz).  Keys are
<model>[_gamma]_<precision>_B<n>_<framewise|clipwise>: a file saved before the
keys carried the full model name and the output's name does not compare with
a new one (--compare walks the first file's keys)."""
import os
import sys

if sys.argv[1] == '--compare':
    import numpy as np
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = 0
    for k in a.files:
        eq = np.array_equal(a[k], b[k])
        d = float(np.max(np.abs(a[k].astype(np.float64) - b[k]))) if a[k].shape == b[k].shape else float('nan')
        print('%-40s %s  max|d| %.3g' % (k, 'IDENTICAL' if eq else 'DIFFERENT', d))
        bad += not eq
    sys.exit(1 if bad else 0)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import bench  # noqa: E402  (honours --ab-package in sys.argv)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sedx import _lib, inference, models, synth  # noqa: E402


def _list(flag, default):
    if flag not in sys.argv:
        return default
    return tuple(sys.argv[sys.argv.index(flag) + 1].split(','))


names = _list('--models', ('Cnn_9layers_Gru_FrameAtt', 'Cnn_9layers_Transformer_FrameAtt'))
if names == ('all',):
    names = tuple(synth.MODEL_PARTS)
precisions = _list('--precisions', ('exact', 'x3'))
runs = [(n, (16000, 512, 160, 64, 25, 7000), 'logmel', 16000) for n in names]
if '--gamma' in sys.argv:
    runs.append(('Cnn_9layers_Gru_FrameAtt', (32000, 1024, 320, 64, 50, 14000), 'gamma', 32000))


def build(name, preset, feature):
    """bench.build_model's steps, for the models without a sequence layer too
    (their constructors take no feature argument, which build_model passes)"""
    args = preset + (25,) + ((feature,) if synth.MODEL_PARTS[name][0] else ())
    m = getattr(models, name)(*args)
    sd = m.state_dict()
    for k, v in synth.make_state_dict(name, seed=0).items():
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd)
    m.set_tuning(_lib.TUNE_WINO_BLOCK1, int(bench.WINO_BLOCK1))
    m.set_tuning(_lib.TUNE_WINO_F43, int(bench.WINO_F43))
    return m.to(dev).eval()


dev = torch.device('cuda:0')
out = {}
for name, preset, feature, sr in runs:
    m = build(name, preset, feature)
    for prec in precisions:
        m.set_precision(prec)
        for B in (1, 32):
            w = torch.from_numpy(synth.make_waveforms(B, seconds=10.0, sample_rate=sr, seed=77)).to(dev)
            with torch.no_grad():
                o = m(inference.gamma_features(m, w) if feature == 'gamma' else w)
            tag = name + ('_gamma' if feature == 'gamma' else '')
            for k in ('framewise_output', 'clipwise_output'):
                out['%s_%s_B%d_%s' % (tag, prec, B, k.split('_')[0])] = o[k].cpu().numpy()
np.savez(sys.argv[1], **out)
print('saved', sys.argv[1], len(out))
