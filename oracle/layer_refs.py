"""ORACLE (test infrastructure only): layer-by-layer references for the stage
captures of libsedx (``sedx_set_capture``, include/sedx.h) in any dtype.

The oracle's layer functions (``oracle.sed_oracle.bn0 / conv_block /
gru_bidirectional / multihead / att_block``) take whatever dtype their state
dict and input carry, so a state dict cast to float64 gives a high-precision
reference of every capturable step, and the same functions in float32 give
the reference arithmetic's own rounding for that step and that input (the
yardstick of tests/test_gpu_layers.py).  One function per step; each takes
the previous stage and returns the next in the oracle's own layout (NCHW
activations, [B, 512, T/8] after the CNN, [B, T/8, 512] after the GRU / MHA).
``from_capture`` / ``to_capture`` convert to and from the library's
channels-last capture layouts.

CPU only.  Nothing here imports the library; ``sedx.synth`` is plain numpy.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import sed_oracle as O
from sedx import synth

GRU, TRF = 'Cnn_9layers_Gru_FrameAtt', 'Cnn_9layers_Transformer_FrameAtt'
POOLS = {1: (2, 2), 2: (2, 2), 3: (2, 2), 4: (1, 1)}
BN_EPS = 1e-5


# ---------------------------------------------------------------------------
# weights and inputs
# ---------------------------------------------------------------------------
def state(mt, classes_num, seed, dtype):
    """``synth.make_state_dict`` as torch tensors of ``dtype`` (weights and BN
    statistics cast; the int64 ``num_batches_tracked`` entries left alone)."""
    sd = {}
    for k, v in synth.make_state_dict(mt, classes_num=classes_num, seed=seed).items():
        t = torch.from_numpy(np.asarray(v))
        sd[k] = t.to(dtype) if t.is_floating_point() else t
    return sd


def features(B, T, seed):
    """float32 [B, 64, T] = -40 + 20 N(0,1): with synth's bn0 statistics
    (mean -45..-35, var 300..500) the bn0 output is near N(0,1), so the conv
    stack sees a full-range image."""
    rng = np.random.default_rng(seed)
    return (-40.0 + 20.0 * rng.standard_normal((B, 64, T))).astype(np.float32)


# ---------------------------------------------------------------------------
# layouts: the library's captures (include/sedx.h, sedx_set_capture) <-> oracle
# ---------------------------------------------------------------------------
STAGES = (0, 2, 3, 4, 5, 6, 7, 8, 9)


def capture_shape(stage, B, T):
    """Shape of the capture of ``stage`` for a [B, 64, T] input."""
    T1, T2, T3 = T // 2, T // 4, T // 8
    return {0: (B, T, 64), 2: (B, T1, 32, 64), 3: (B, T1, 32, 128), 4: (B, T2, 16, 128),
            5: (B, T2, 16, 256), 6: (B, T3, 8, 256), 7: (B, T3, 8, 512), 8: (B, T3, 512),
            9: (B, T3, 512)}[stage]


def from_capture(stage, a):
    """Capture layout -> the oracle's layout, as a contiguous torch tensor."""
    a = torch.as_tensor(a)
    if stage == 0:                      # [B][T][64] -> [B, 1, T, 64]
        return a[:, None].contiguous()
    if 2 <= stage <= 7:                 # [B][T'][F'][C] -> [B, C, T', F']
        return a.permute(0, 3, 1, 2).contiguous()
    if stage == 8:                      # [B][T/8][512] -> [B, 512, T/8]
        return a.transpose(1, 2).contiguous()
    if stage == 9:                      # [B][T/8][512] as the oracle's seq_out
        return a.contiguous()
    raise ValueError('stage %r cannot be captured' % (stage,))


def to_capture(stage, x):
    """The oracle's layout -> capture layout (inverse of ``from_capture``)."""
    x = torch.as_tensor(x)
    if stage == 0:
        return x[:, 0].contiguous()
    if 2 <= stage <= 7:
        return x.permute(0, 2, 3, 1).contiguous()
    if stage == 8:
        return x.transpose(1, 2).contiguous()
    if stage == 9:
        return x.contiguous()
    raise ValueError('stage %r cannot be captured' % (stage,))


# ---------------------------------------------------------------------------
# one function per capturable step (previous stage -> next stage)
# ---------------------------------------------------------------------------
def step_bn0(sd, feat):
    """features [B, 64, T] -> stage 0 [B, 1, T, 64] (models.py:636-644)."""
    x = torch.as_tensor(feat).transpose(1, 2)[:, None]
    return O.bn0(sd, x).contiguous()


def step_block1(sd, x):
    """stage 0 -> stage 2: conv1 + conv2 + 2x2 pool of block 1."""
    return O.conv_block(sd, 1, x, POOLS[1])


def step_conv1(sd, k, x):
    """stage 2 / 4 / 6 -> 3 / 5 / 7: conv1 + bn1 + relu of block k
    (ConvBlock.forward, models.py:125-141, first half)."""
    p = 'conv_block%d' % k
    return F.relu(O._bn(sd, p + '.bn1', F.conv2d(x, O._t(sd[p + '.conv1.weight']), padding=1)))


def step_conv2(sd, k, x):
    """stage 3 / 5 / 7 -> 4 / 6 / 8: conv2 + bn2 + relu + pool of block k;
    k = 4 includes the (1, 1) pool and the frequency mean (models.py:666-668),
    giving [B, 512, T/8]."""
    p = 'conv_block%d' % k
    x = F.relu(O._bn(sd, p + '.bn2', F.conv2d(x, O._t(sd[p + '.conv2.weight']), padding=1)))
    x = F.avg_pool2d(x, kernel_size=POOLS[k])
    return torch.mean(x, dim=3) if k == 4 else x


def step_seq(sd, mt, x):
    """stage 8 [B, 512, T/8] -> stage 9 [B, T/8, 512]: GRU or MHA."""
    x = x.transpose(1, 2)
    return O.gru_bidirectional(sd, x) if mt == GRU else O.multihead(sd, x)


def step_head(sd, mt, x):
    """stage 9 [B, T/8, 512] -> the three outputs, as ``O.forward`` builds
    them (x8 repeat, the GRU model's pad-to-100 rule, the embedding)."""
    x = x.transpose(1, 2)
    clipwise, _, cla = O.att_block(sd, x)
    fw = O.framewise_from_cla(cla, mt == GRU)
    return {'framewise_output': fw, 'clipwise_output': clipwise, 'embedding': cla if mt == GRU else x}


# (previous stage, next stage, step) in capture order
def conv_steps():
    return [(0, 2, step_block1),
            (2, 3, lambda sd, x: step_conv1(sd, 2, x)), (3, 4, lambda sd, x: step_conv2(sd, 2, x)),
            (4, 5, lambda sd, x: step_conv1(sd, 3, x)), (5, 6, lambda sd, x: step_conv2(sd, 3, x)),
            (6, 7, lambda sd, x: step_conv1(sd, 4, x)), (7, 8, lambda sd, x: step_conv2(sd, 4, x))]


def chain(sd, mt, x0, stages=None):
    """Every step from stage 0 (oracle layout) on: returns the outputs and,
    in ``stages`` (a dict, optional), each stage in the oracle's layout."""
    with torch.no_grad():
        x = x0
        if stages is not None:
            stages[0] = x
        for _, nxt, fn in conv_steps():
            x = fn(sd, x)
            if stages is not None:
                stages[nxt] = x
        x = step_seq(sd, mt, x)
        if stages is not None:
            stages[9] = x
        return step_head(sd, mt, x)


# ---------------------------------------------------------------------------
# magnitude bounds for the split-bf16 (x3) mode: the same step with |input|,
# |BN-folded weight| and |bias| (include/sedx.h: products err ~2^-16 relative)
# ---------------------------------------------------------------------------
def _folded_abs(sd, p, conv, bn):
    s = O._t(sd[p + bn + '.weight']) / torch.sqrt(O._t(sd[p + bn + '.running_var']) + BN_EPS)
    w = (O._t(sd[p + conv + '.weight']) * s[:, None, None, None]).abs()
    b = (O._t(sd[p + bn + '.bias']) - O._t(sd[p + bn + '.running_mean']) * s).abs()
    return w, b


def absbound_conv1(sd, k, x):
    w, b = _folded_abs(sd, 'conv_block%d' % k, '.conv1', '.bn1')
    return F.conv2d(x.abs(), w, padding=1) + b[None, :, None, None]


def absbound_conv2(sd, k, x):
    w, b = _folded_abs(sd, 'conv_block%d' % k, '.conv2', '.bn2')
    s = F.avg_pool2d(F.conv2d(x.abs(), w, padding=1) + b[None, :, None, None], kernel_size=POOLS[k])
    return torch.mean(s, dim=3) if k == 4 else s


def absbound_block1(sd, x):
    """Block 1 in x3 mode: conv1 (one input channel) is fp32, conv2 split-bf16
    on conv1's activation."""
    return absbound_conv2(sd, 1, step_conv1(sd, 1, x))


def absbound_linear(x, w, b):
    return F.linear(x.abs(), O._t(w).abs(), O._t(b).abs())


def absbound_seq(sd, mt, x):
    """Largest pre-activation magnitude sum of the step's projections: GRU
    |x||W_ih| + |b_ih| + |W_hh| 1 + |b_hh| (|h| <= 1); MHA the q/k/v
    projections and fc on |attention output|.  The gates, softmax averages and
    the relu are 1-Lipschitz or contractions of those pre-activations."""
    x = x.transpose(1, 2)
    if mt == GRU:
        m = 0.0
        for sfx in ('', '_reverse'):
            gi = absbound_linear(x, sd['gru.weight_ih_l0' + sfx], sd['gru.bias_ih_l0' + sfx])
            gh = O._t(sd['gru.weight_hh_l0' + sfx]).abs().sum(dim=1) + O._t(sd['gru.bias_hh_l0' + sfx]).abs()
            m = max(m, float((gi + gh).max()))
        return m
    m = 0.0
    v = None
    for nm in ('w_qs', 'w_ks', 'w_vs'):
        v = absbound_linear(x, sd['multihead.%s.weight' % nm], sd['multihead.%s.bias' % nm])
        m = max(m, float(v.max()))
    # the attention output is a convex combination of value rows: |o| <= max_t |v|
    o = v.max(dim=1, keepdim=True).values.expand_as(v)
    return max(m, float(absbound_linear(o, sd['multihead.fc.weight'], sd['multihead.fc.bias']).max()))


def absbound_head(sd, mt, x):
    """Per-element magnitude sums S of the head's att | cla projections of
    stage 9 ``x`` [B, T/8, 512], laid out as the three outputs: framewise and
    the GRU model's embedding carry the cla logit's S of their own (class,
    frame) (the sigmoid is 1/4-Lipschitz); clipwise the largest att or cla S
    over the frames of its (clip, class) (the normalised attention is a
    relative perturbation of the att logits, the sum a convex combination)."""
    x = x.transpose(1, 2)
    a = F.conv1d(x.abs(), O._t(sd['att_block.att.weight']).abs(), O._t(sd['att_block.att.bias']).abs())
    c = F.conv1d(x.abs(), O._t(sd['att_block.cla.weight']).abs(), O._t(sd['att_block.cla.bias']).abs())
    return {'framewise_output': O.framewise_from_cla(c, mt == GRU),
            'clipwise_output': torch.maximum(a, c).amax(dim=2),
            'embedding': c if mt == GRU else None}


# ---------------------------------------------------------------------------
# the exact mode's direct convolution as its kernel sums it
# ---------------------------------------------------------------------------
def chain_conv1_fp32(sd, k, x, pixels):
    """conv1 + bn1 + relu of block k at ``pixels`` (rows of (b, t, f)) in fp32
    the way csrc/conv.hip's conv3x3_kernel accumulates it: BN folded into the
    weights in float64 and rounded once (csrc/weights.cpp: bn_fold's scale,
    prepare_weights' bias and wf, pack_conv_exact), one in-order fma
    chain per output over K = 9 Cin from zero - chunks of 4 input channels,
    the 9 taps of a chunk, its 4 channels (conv.hip header comment :13-23 and the wave-shape comment
    :73-83) - then
    + bias and ReLU.  ``sd`` float64, ``x`` fp32 [B, Cin, T, F]; returns fp32
    [len(pixels), Cout].  An fma is emulated as a float64 product (exact for
    fp32 operands) and sum rounded to fp32."""
    p = 'conv_block%d' % k
    s = O._t(sd[p + '.bn1.weight']) / torch.sqrt(O._t(sd[p + '.bn1.running_var']) + BN_EPS)
    w = (O._t(sd[p + '.conv1.weight']) * s[:, None, None, None]).float().double()   # [Cout, Cin, 3, 3]
    b = (O._t(sd[p + '.bn1.bias']) - O._t(sd[p + '.bn1.running_mean']) * s).float()
    xp = F.pad(x.double(), (1, 1, 1, 1))
    pix = torch.as_tensor(pixels, dtype=torch.long)
    pb, pt, pf = pix[:, 0], pix[:, 1], pix[:, 2]
    cin = x.shape[1]
    acc = torch.zeros(len(pix), w.shape[0], dtype=torch.float32)
    for chunk in range(cin // 4):
        for tap in range(9):
            a = xp[pb, :, pt + tap // 3, pf + tap % 3]                  # [N, Cin]
            for i in range(4 * chunk, 4 * chunk + 4):
                acc = (acc.double() + a[:, i, None] * w[None, :, i, tap // 3, tap % 3]).float()
    return F.relu(acc + b[None, :])


def sample_pixels(B, T, Fq, n, seed=0):
    """Up to n distinct (b, t, f) of a [B, C, T, Fq] activation, the corners
    of the first and last clip among them."""
    rng = np.random.default_rng(seed)
    total = B * T * Fq
    idx = set(rng.choice(total, size=min(n, total), replace=False).tolist())
    idx |= {0, Fq - 1, (T - 1) * Fq, total - 1}
    idx = np.array(sorted(idx))
    return np.stack([idx // (T * Fq), idx // Fq % T, idx % Fq], axis=1)


# ---------------------------------------------------------------------------
# the shapes of the end-to-end sweep (tests/test_gpu_layers.py, section 3b),
# shared with tests/test_layer_refs_cpu.py's coverage check
# ---------------------------------------------------------------------------
SWEEP_T_ALL = (list(range(8, 72)) + list(range(124, 136)) + list(range(252, 264))
               + list(range(504, 528)))
SWEEP_SHAPES = ([(3, T) for T in SWEEP_T_ALL]
                + [(1, T) for T in (8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 135, 527)]
                + [(B, T) for B in (8, 16) for T in (37, 64, 136, 260)]
                + [(72, T) for T in (64, 136)])
