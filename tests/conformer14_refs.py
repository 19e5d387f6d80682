"""Layer references of ``Cnn_14layers_Conformer_FrameAtt`` (test infrastructure
only): the float64 / float32 restatement of pytorch/models.py:1780-1794 on the
steps of ``tests/conformer_refs.py`` (the encoder is the 9-layer models' with a
2048-wide input Linear) and ``oracle/sed_oracle.py``'s AttBlock, plus fp32 CPU
emulations of the two documented summation orders this model adds:

  * the input layer's GEMM at K = 2048 (csrc/conformer.hip, cf_gemm_kernel):
    four in-order fma chains over the K quarters of 512, summed
    ((q0 + q1) + q2) + q3, + bias;
  * the head (csrc/att_head_rep.hip header): a_t by the spelled-out
    exponential, tot and clipwise as 8 lane partials (t = l mod 8, ascending)
    combined ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)).

CPU only; nothing here imports the library.
"""
import numpy as np
import torch

import conformer_refs as CR
import deep14_refs as D14
from oracle import sed_oracle as O
from sedx import synth

CF14 = 'Cnn_14layers_Conformer_FrameAtt'
SEED = synth.CONFORMER14_GOLDEN_SEEDS[CF14]
KEYS = CR.KEYS
P16 = CR.P16
ACT_IDS = CR.ACT_IDS                       # 20 .. 32, all [B, T5, 144]
STEPS = [(43, 20)] + [(i, i + 1) for i in range(20, 32)]
LOGITS = 44                                # capture id of the head's logits [B * T5, 64]
f32 = np.float32


def state(dtype, classes_num=25):
    """synth weights of the golden seed plus the constructor's constant buffers."""
    return CR.state(CF14, classes_num, SEED, dtype)


def geometry(T):
    """T input frames -> (T5, ratio, framewise frames) (models.py:1791-1794)."""
    T5 = T // 32
    ratio = 1000 // T5
    n = ratio * T5
    return T5, ratio, n if n == 1000 else O.roundup(n)


def step(sd, src, x):
    """The step from capture id ``src`` to the next one; 43: x [B, T5, 2048]."""
    return CR.input_layer(sd, x) if src == 43 else CR.step(sd, src, x)


def head(sd, x):
    """x [B, T5, 144] (the encoder output) -> the three outputs."""
    emb = x.transpose(1, 2)
    clipwise, _, cla = O.att_block(sd, emb)
    _, ratio, _ = geometry(32 * x.shape[1])
    return {'framewise_output': CR.interpolate_pad(cla.transpose(1, 2), ratio), 'clipwise_output': clipwise,
            'embedding': emb}


# ---------------------------------------------------------------------------
# the input layer's GEMM in the kernel's order
# ---------------------------------------------------------------------------
def emulate_input_gemm(sd, x):
    """x [B, T5, 2048] fp32 -> A W^T + b [B, T5, 144] fp32 the way cf_gemm_kernel
    sums K = 2048 (``sd`` float64: the weights are rounded to fp32 here)."""
    w = sd['encoder.input_layer.0.weight'].numpy().astype(f32)          # [144, 2048]
    b = sd['encoder.input_layer.0.bias'].numpy().astype(f32)
    a = np.asarray(x, f32).reshape(-1, 2048)
    aq = np.ascontiguousarray(a.reshape(-1, 4, 512).transpose(1, 0, 2))   # [4, M, 512]
    wq = np.ascontiguousarray(w.reshape(144, 4, 512).transpose(1, 0, 2))  # [4, 144, 512]
    p = D14._fma_chains(aq, wq)                                         # [4, M, 144]
    y = (((p[0] + p[1]) + p[2]) + p[3]) + b[None, :]
    return torch.from_numpy(y.astype(f32).reshape(tuple(x.shape[:2]) + (144,)))


def emulate_input_layer(sd64, sd32, x):
    """Capture 20 from capture 43 with the GEMM in the kernel's order and the
    rest (LayerNorm, ReLU, x 12, + pe) as the fp32 restatement does it."""
    import math
    import torch.nn.functional as F
    y = emulate_input_gemm(sd64, x)
    y = F.relu(CR._ln(sd32, 'encoder.input_layer.1', y))
    return y * math.sqrt(CR.D) + sd32['encoder.input_layer.4.pe'][:, :x.shape[1]]


# ---------------------------------------------------------------------------
# the head in the kernel's order (csrc/att_head_rep.hip)
# ---------------------------------------------------------------------------
def _fma(a, b, c):
    """One fused multiply-add in fp32, exactly: a b + c rounded ONCE to fp32.
    The product of two fp32 values is exact in float64; the float64 sum s = p + c
    may round, with the exact remainder e from the error-free two-sum.  Rounding
    s to fp32 is the rounding of p + c unless s sits exactly half way between two
    fp32 neighbours while e != 0 (the float64 rounding is monotonic and the
    midpoint is a float64 number, so s and s + e lie on one side of it otherwise):
    there the tie is broken by the sign of e instead of to-even."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                      # two-sum: p + c = s + e exactly
    r = s.astype(f32)
    d = s - r.astype(np.float64)                       # exact
    fix = (e != 0) & (d != 0)
    if fix.any():
        other = np.nextafter(r, np.where(d > 0, f32(np.inf), f32(-np.inf)).astype(f32))
        mid = 0.5 * (r.astype(np.float64) + other.astype(np.float64))
        tie = fix & (mid == s)
        up = tie & (np.sign(e) == np.sign(d))          # the exact value lies beyond the midpoint: the other neighbour
        r = np.where(up, other, r).astype(f32)
    return r


def rep_exp(x):
    """rep_exp_ of the kernel, operation by operation, on fp32 x in [-10, 10]."""
    x = np.asarray(x, f32)
    n = np.rint(x * f32(1.44269504088896341)).astype(f32)
    r = _fma(n, f32(-0.693359375), x)
    r = _fma(n, f32(2.12194440e-4), r)
    p = np.full_like(x, f32(1.9875691500e-4))
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = _fma(p, r, f32(c))
    y = _fma(p, r * r, r) + f32(1.0)
    return np.ldexp(y, n.astype(np.int32)).astype(f32)


def _tree8(p):
    """[8, ...] lane partials -> ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))."""
    return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))


def emulate_clipwise(att, s):
    """att [B, T, C] fp32 logits, s [B, T, C] fp32 framewise values sigmoid(cla)
    -> (tot, clipwise) [B, C] fp32 in the kernel's stated order."""
    att, s = np.asarray(att, f32), np.asarray(s, f32)
    B, T, C = att.shape
    a = rep_exp(np.minimum(np.maximum(att, f32(-10.0)), f32(10.0))) + f32(1e-6)
    p = np.zeros((8, B, C), f32)
    for t in range(T):
        p[t % 8] = p[t % 8] + a[:, t]
    tot = _tree8(p)
    inv = (f32(1.0) / tot).astype(f32)
    q = np.zeros((8, B, C), f32)
    for t in range(T):
        q[t % 8] = _fma(a[:, t] * inv, s[:, t], q[t % 8])
    return tot, _tree8(q)


def sigmoid32(x):
    x = np.asarray(x, f32)
    return (f32(1.0) / (f32(1.0) + np.exp(-x, dtype=f32))).astype(f32)
