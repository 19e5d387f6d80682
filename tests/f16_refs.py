"""CPU references of SEDX_PRECISION_F16 (include/sedx.h), built from the
oracle's layer functions alone (oracle/layer_refs.py): the operand rounding
``q``, and per conv step of ``layer_refs.conv_steps()``

  E    the float64 step on q(input) and q(fp32(BN-folded weight)), with the
       fp32-rounded folded bias: what the f16 conv layer computes, up to its
       fp32 accumulation;
  S16  the same step on their absolute values without the ReLU (as
       ``layer_refs.absbound_conv1/2``): the magnitude sum an accumulation
       error is measured against;
  R,S  the un-rounded float64 step and its magnitude sum (layer_refs' own).

Block 1's step is conv1 in float64, cast to fp32 (the library's conv1 is
fp32), then q, then conv2.  ``chain`` runs every step on the previous E and
the sequence layer and head in float64: the end-to-end outputs E_out.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import layer_refs as R
from oracle import sed_oracle as O

TINY = 2.0 ** -14
KEYS = ('framewise_output', 'clipwise_output', 'embedding')
SHAPES = ((1, 8), (3, 37), (2, 135))


def q(x, flush=True):
    """q(v) of fp32 values, as float64: clamp to +-65504, nearest-even fp16
    with gradual underflow, then |q| < 2^-14 -> +0."""
    h = torch.as_tensor(x).float().clamp(-65504.0, 65504.0).half().double()
    if flush:
        h = torch.where(h.abs() < TINY, torch.zeros_like(h), h)
    return h


def q_numpy(x, flush=True):
    """The same with numpy alone (tests/test_f16_cpu.py compares pack_f16 with it), as fp16."""
    with np.errstate(over='ignore'):
        h = np.clip(np.asarray(x, dtype=np.float32), np.float32(-65504.0), np.float32(65504.0)).astype(np.float16)
    if flush:
        h = np.where(np.abs(h.astype(np.float64)) < TINY, np.float16(0.0), h)
    return h


def folded(sd, k, j):
    """BN-folded weight and bias of block k's conv j in float64 (csrc/weights.cpp: bn_fold, prepare_weights)."""
    p, bn = 'conv_block%d' % k, '.bn%d' % j
    s = O._t(sd[p + bn + '.weight']) / torch.sqrt(O._t(sd[p + bn + '.running_var']) + R.BN_EPS)
    w = O._t(sd[p + '.conv%d.weight' % j]) * s[:, None, None, None]
    b = O._t(sd[p + bn + '.bias']) - O._t(sd[p + bn + '.running_mean']) * s
    return w, b


def _finish(y, k, j, relu):
    if relu:
        y = F.relu(y)
    if j == 2:
        y = F.avg_pool2d(y, kernel_size=R.POOLS[k])
        if k == 4:
            y = torch.mean(y, dim=3)
    return y


def conv_E(sd, k, j, x, flush=True):
    """E of block k's conv j on the fp32 activation x (oracle layout)."""
    w, b = folded(sd, k, j)
    y = F.conv2d(q(x, flush), q(w.float(), flush), padding=1) + b.float().double()[None, :, None, None]
    return _finish(y, k, j, True)


def conv_S16(sd, k, j, x):
    w, b = folded(sd, k, j)
    y = F.conv2d(q(x).abs(), q(w.float()).abs(), padding=1) + b.float().double().abs()[None, :, None, None]
    return _finish(y, k, j, False)


def _conv1_fp32(sd, x):
    """Block 1's conv1 + bn1 + ReLU in float64, cast to fp32."""
    return R.step_conv1(sd, 1, x.double()).float()


# (previous stage, next stage, E, S16, R, S): each a function of (float64 state dict, previous stage)
def steps():
    out = [(0, 2,
            lambda sd, x, flush=True: conv_E(sd, 1, 2, _conv1_fp32(sd, x), flush),
            lambda sd, x: conv_S16(sd, 1, 2, _conv1_fp32(sd, x)),
            lambda sd, x: R.step_block1(sd, x.double()),
            lambda sd, x: R.absbound_block1(sd, x.double()))]
    for prev, nxt, _ in R.conv_steps()[1:]:
        k, j = (nxt + 1) // 2, 1 if nxt % 2 else 2
        out.append((prev, nxt,
                    lambda sd, x, flush=True, k=k, j=j: conv_E(sd, k, j, x, flush),
                    lambda sd, x, k=k, j=j: conv_S16(sd, k, j, x),
                    (lambda sd, x, k=k: R.step_conv1(sd, k, x.double())) if j == 1
                    else (lambda sd, x, k=k: R.step_conv2(sd, k, x.double())),
                    (lambda sd, x, k=k: R.absbound_conv1(sd, k, x.double())) if j == 1
                    else (lambda sd, x, k=k: R.absbound_conv2(sd, k, x.double()))))
    return out


def chain(sd, mt, x0, stages=None, flush=True):
    """The chained emulation from stage 0 (oracle layout, float64 or fp32):
    every conv step's E on the previous E cast to fp32 (activations are fp32
    in memory), the sequence layer and the head in float64."""
    with torch.no_grad():
        x = torch.as_tensor(x0)
        if stages is not None:
            stages[0] = x
        for _, nxt, E, _, _, _ in steps():
            x = E(sd, x.float(), flush)
            if stages is not None:
                stages[nxt] = x
        x = R.step_seq(sd, mt, x.float().double())
        if stages is not None:
            stages[9] = x
        return R.step_head(sd, mt, x)


_CACHE = {}


def outputs(mt, seed, B, T, feat=None, tag=None):
    """(E_out, R_out, d_q) of model mt on layer_refs.features(B, T, seed=0)
    (or ``feat``, cached under ``tag``): numpy float64 per output key, and
    d_q[key] = max|E_out - R_out|.  Computed once per key."""
    key = (mt, seed, B, T, tag)
    if key not in _CACHE:
        sd = R.state(mt, 25, seed, torch.float64)
        f = torch.from_numpy(R.features(B, T, 0) if feat is None else feat).double()
        with torch.no_grad():
            x0 = R.step_bn0(sd, f)
            e = chain(sd, mt, x0)
            r = R.chain(sd, mt, x0)
        e = {k: e[k].numpy() for k in KEYS}
        r = {k: r[k].numpy() for k in KEYS}
        _CACHE[key] = (e, r, {k: float(np.abs(e[k] - r[k]).max()) for k in KEYS})
    return _CACHE[key]
