"""Layer references of ``Cnn14_DecisionLevelAtt`` (test infrastructure only):
float64 / float32 restatements of the steps pytorch/models.py:2763-2781 adds
to the 14-layer trunk -- the pooled sum over three sequence frames, ``fc1`` +
ReLU, the AttBlock's framewise expansion to ``T - 1`` frames -- and a CPU fp32
emulation of csrc/decision.hip's documented summation order.  Everything that
already exists is imported: the trunk's steps from ``deep14_refs``, the
AttBlock from ``oracle/sed_oracle.py``, the state helper from
``oracle/layer_refs.py``.

CPU only; nothing here imports the library.
"""
import numpy as np
import torch
import torch.nn.functional as F

import deep14_refs as D
from oracle import layer_refs as R
from oracle import sed_oracle as O
from sedx import synth

CNN14 = 'Cnn14_DecisionLevelAtt'
SEED = synth.CNN14_GOLDEN_SEEDS[CNN14]
RATIO = D.RATIO
KEYS = ('framewise_output', 'clipwise_output')
P16 = (16000, 512, 160, 64, 25, 7000)
P32 = (32000, 1024, 320, 64, 50, 14000)
MAX_CLASSES = 527


def state(dtype, classes_num=25):
    return R.state(CNN14, classes_num, SEED, dtype)


def geometry(T):
    """T frames -> (T5, out_frames) = (T // 32, T - 1), or None where the
    reference raises: fewer than 32 frames (its fifth pool has no output) and
    every multiple of 32 (pad_framewise_output is asked for -1 frames)."""
    if T < 32 or T % 32 == 0:
        return None
    return T // 32, T - 1


def step_pool(x):
    """[B, 2048, T5] -> max_pool1d(3, 1, 1) + avg_pool1d(3, 1, 1) (models.py:2765-2767):
    -inf padding for the max, zero padding and always / 3 for the mean."""
    return F.max_pool1d(x, kernel_size=3, stride=1, padding=1) + F.avg_pool1d(x, kernel_size=3, stride=1, padding=1)


def step_decision(sd, x):
    """stage 43 [B, 2048, T5] -> stage 9 [B, T5, 2048] = relu(fc1(pooled)) (models.py:2765-2770)."""
    p = step_pool(x).transpose(1, 2)
    return F.relu(torch.matmul(p, O._t(sd['fc1.weight']).t()) + O._t(sd['fc1.bias']))


def step_fc1(sd, p):
    """fc1's input [B, T5, 2048] -> relu(fc1)."""
    return F.relu(torch.matmul(p, O._t(sd['fc1.weight']).t()) + O._t(sd['fc1.bias']))


def step_head(sd, x, frames):
    """stage 9 [B, T5, 2048] -> the two outputs (models.py:2773-2781): every
    sequence frame x32, then the last frame repeated up to ``frames``."""
    clipwise, _, cla = O.att_block(sd, x.transpose(1, 2))
    fw = cla.transpose(1, 2)
    B, T, C = fw.shape
    fw = fw[:, :, None, :].repeat(1, 1, RATIO, 1).reshape(B, T * RATIO, C)
    assert frames >= fw.shape[1]
    fw = torch.cat([fw, fw[:, -1:, :].repeat(1, frames - fw.shape[1], 1)], dim=1)
    return {'framewise_output': fw, 'clipwise_output': clipwise}


def trunk(sd, x0):
    """bn0 output [B, 1, T, 64] -> stage 43 [B, 2048, T5]: deep14_refs' eleven conv steps."""
    for _, _, _, fn in D.conv_steps():
        x0 = fn(sd, x0)
    return x0


def chain(sd, feat):
    """features [B, 64, T] -> the two outputs, every step in sd's dtype."""
    with torch.no_grad():
        x = trunk(sd, R.step_bn0(sd, feat))
        return step_head(sd, step_decision(sd, x), geometry(feat.shape[2])[1])


# ---------------------------------------------------------------------------
# csrc/decision.hip's arithmetic, emulated in fp32 on the CPU
# ---------------------------------------------------------------------------
def pooled_fp32(S):
    """S fp32 [B, T5, 2048] -> P fp32 as the kernel rounds it (its header):
    max over the in-clip frames + ((lo + S) + hi) / 3.0f, lo / hi = 0.0f outside the clip."""
    S = np.asarray(S, np.float32)
    lo, hi = np.zeros_like(S), np.zeros_like(S)
    lo[:, 1:], hi[:, :-1] = S[:, :-1], S[:, 1:]
    mx = S.copy()
    mx[:, 1:] = np.maximum(mx[:, 1:], S[:, :-1])
    mx[:, :-1] = np.maximum(mx[:, :-1], S[:, 1:])
    avg = ((lo + S).astype(np.float32) + hi).astype(np.float32) / np.float32(3.0)
    return (mx + avg.astype(np.float32)).astype(np.float32)


def kernel_k_order():
    """The k of the 2048 fma steps of one K quarter q = 0: g, c, j -> 16 g + 4 j + c."""
    return np.array([16 * g + 4 * j + c for g in range(32) for c in range(4) for j in range(4)])


def emulate_decision(w1, b1, S, rows, cols):
    """The kernel's H at rows (b, t) x output columns ``cols``: P rounded as
    above; per K quarter one in-order fma chain from zero in the header's k
    order (an fma = a float64 product, exact for fp32 operands, and sum, rounded
    to fp32 once); ((a0 + a1) + a2) + a3, + bias, ReLU.  w1 [2048, 2048], b1
    [2048] fp32; returns fp32 [len(rows), len(cols)]."""
    P = pooled_fp32(S)
    rows = np.asarray(rows)
    a = P[rows[:, 0], rows[:, 1]].astype(np.float64)                 # [R, 2048]
    w = np.asarray(w1, np.float32)[np.asarray(cols)].astype(np.float64)   # [C, 2048]
    order = kernel_k_order()
    parts = []
    for q in range(4):
        acc64 = np.zeros((len(rows), len(cols)), np.float64)
        acc32 = np.zeros((len(rows), len(cols)), np.float32)
        for k in 512 * q + order:
            acc64 += a[:, k][:, None] * w[:, k][None, :]
            acc32[...] = acc64                                      # one rounding per fma
            acc64[...] = acc32
        parts.append(acc32.copy())
    v = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    v = v + np.asarray(b1, np.float32)[np.asarray(cols)][None, :]
    return np.maximum(v, np.float32(0.0)).astype(np.float32)


def sample_rows(B, T5, n, seed=0):
    """Up to n distinct (b, t), every clip's first and last frame of the first
    and last clip and the rows on both sides of each 32-row tile edge among them."""
    rng = np.random.default_rng(seed)
    M = B * T5
    idx = set(rng.choice(M, size=min(n, M), replace=False).tolist())
    idx |= {0, T5 - 1, M - T5, M - 1}
    idx |= {m for e in range(32, M, 32) for m in (e - 1, e)}
    idx = np.array(sorted(i for i in idx if 0 <= i < M))
    return np.stack([idx // T5, idx % T5], axis=1)
