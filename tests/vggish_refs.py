"""Layer references of the three VGGish models (test infrastructure only): the
tests' own float64 / float32 torch restatement of every step of
pytorch/models.py:2219-2592 -- the six convs with bias and ReLU, the four
flooring 2x2 max pools, the mean over the 4 remaining bins, the bi-GRU, the two
heads with their frame repeat and padding to 1000 frames -- and CPU fp32
emulations of the summation orders that csrc/conv_vgg.hip and csrc/conv.hip
document.  The GRU recurrence and the AttBlock come from ``oracle/sed_oracle.py``.

Activations are channels-last, as ``sedx_set_capture`` returns them:
stage 0 [B, T, 64]; 50 [B, T/2, 32, 64]; 51 [B, T/4, 16, 128]; 52 [B, T/4, 16, 256];
53 [B, T/8, 8, 256]; 54 [B, T/8, 8, 512]; 55 [B, T/16, 4, 512]; 8 and 9 [B, T/16, 512].

CPU only; nothing here imports the library.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import layer_refs as R
from oracle import sed_oracle as O
from sedx import synth

ATT, GRU, AVG = 'VGGish_FrameAtt', 'VGGish_Gru_FrameAtt', 'VGGish_FrameAvg'
MODELS = (ATT, GRU, AVG)
IDS = {ATT: 'att', GRU: 'gru', AVG: 'avg'}
MODEL_ID = {ATT: 15, GRU: 16, AVG: 17}
SEEDS = synth.VGGISH_GOLDEN_SEEDS
KEYS = ('framewise_output', 'clipwise_output', 'embedding')
P16 = (16000, 512, 160, 64, 25, 7000)
OUT_FRAMES = 1000
# conv l: (nn.Sequential index, cin, cout, pooled); the capture each conv launch writes and the one it reads
CONVS = [(0, 1, 64, True), (3, 64, 128, True), (6, 128, 256, False), (8, 256, 256, True), (11, 256, 512, False),
         (13, 512, 512, True)]
STAGE_OF = {0: 50, 1: 51, 2: 52, 3: 53, 4: 54, 5: 55}
TRUNK_STAGES = (0, 50, 51, 52, 53, 54, 55, 8)


def ctor_args(ckpt=None, classes=25, freeze=False):
    return P16 + (classes, 'logmel', ckpt, freeze)


def state(mt, dtype):
    return R.state(mt, 25, SEEDS[mt], dtype)


def geometry(mt, T):
    """T frames -> (seq_len, repeat), or None where no forward runs: fewer than
    16 frames (the fourth pool has no output), more than 83 sequence frames on
    the FrameAtt models (x12 passes 1000: the reference's pad count is negative),
    more than 1000 on VGGish_FrameAvg (the reference returns an empty tensor)."""
    seq = T // 2 // 2 // 2 // 2
    if seq < 1 or seq > (1000 if mt == AVG else 83):
        return None
    return seq, (1000 // seq if mt == AVG else 12)


def capture_shape(stage, B, T):
    T1, T2, T3, T4 = T // 2, T // 4, T // 8, T // 16
    return {0: (B, T, 64), 50: (B, T1, 32, 64), 51: (B, T2, 16, 128), 52: (B, T2, 16, 256), 53: (B, T3, 8, 256),
            54: (B, T3, 8, 512), 55: (B, T4, 4, 512), 8: (B, T4, 512), 9: (B, T4, 512)}[stage]


# ---------------------------------------------------------------------------
# the steps, in the dtype of sd
# ---------------------------------------------------------------------------
def _wb(sd, l):
    p = 'vggish.0.%d' % CONVS[l][0]
    return O._t(sd[p + '.weight']), O._t(sd[p + '.bias'])


def step_conv(sd, l, x):
    """Conv l on the previous capture x (channels-last; l = 0: the log-mel [B, T, 64]):
    Conv2d(3x3, padding 1) + bias + ReLU, then MaxPool2d(2, 2) (flooring) where the layer has one."""
    w, b = _wb(sd, l)
    xin = x[:, None] if l == 0 else x.permute(0, 3, 1, 2)
    y = F.relu(F.conv2d(xin, w, b, padding=1))
    if CONVS[l][3]:
        y = F.max_pool2d(y, kernel_size=2, stride=2)
    return y.permute(0, 2, 3, 1).contiguous()


def step_mean(x55):
    """[B, T/16, 4, 512] -> torch.mean over the 4 bins (models.py:2365)."""
    return torch.mean(x55, dim=2)


def step_seq(sd, mt, x8):
    return O.gru_bidirectional(sd, x8) if mt == GRU else x8


def _expand(fw, ratio):
    B, T, C = fw.shape
    fw = fw[:, :, None, :].repeat(1, 1, ratio, 1).reshape(B, T * ratio, C)
    assert fw.shape[1] <= OUT_FRAMES
    return torch.cat([fw, fw[:, -1:, :].repeat(1, OUT_FRAMES - fw.shape[1], 1)], dim=1)


def step_head(sd, mt, x9):
    """stage 9 [B, seq, 512] -> the three outputs (models.py:2370-2383, :2573-2592)."""
    if mt == AVG:
        p = torch.sigmoid(F.linear(x9, O._t(sd['fc.weight']), O._t(sd['fc.bias'])))
        fw = _expand(p, OUT_FRAMES // p.shape[1])
        return {'framewise_output': fw, 'clipwise_output': torch.mean(fw, dim=1), 'embedding': x9.transpose(1, 2)}
    clipwise, _, cla = O.att_block(sd, x9.transpose(1, 2))
    return {'framewise_output': _expand(cla.transpose(1, 2), 12), 'clipwise_output': clipwise, 'embedding': cla}


def trunk(sd, x0):
    """log-mel [B, T, 64] -> {stage: capture} of 50..55 and 8."""
    caps, x = {}, x0
    for l in range(6):
        x = step_conv(sd, l, x)
        caps[STAGE_OF[l]] = x
    caps[8] = step_mean(x)
    return caps


def chain(sd, mt, feat):
    """features [B, 64, T] -> the three outputs, every step in sd's dtype."""
    with torch.no_grad():
        s8 = trunk(sd, feat.transpose(1, 2).contiguous())[8]
        return step_head(sd, mt, step_seq(sd, mt, s8))


# ---------------------------------------------------------------------------
# the kernels' documented orders, emulated in fp32 on the CPU.  An fma is a
# float64 product (exact for fp32 operands) and sum, rounded to fp32 once.
# ---------------------------------------------------------------------------
def _fma(acc32, a64, b64):
    return (acc32.astype(np.float64) + a64 * b64).astype(np.float32)


def emulate_conv1(w, b, x, samples):
    """conv_vgg.hip's header: per conv output taps 0..8 in row-major order, one
    fma chain from zero, + bias, ReLU; the pooled value = the maximum of the 2x2
    window.  w [64, 1, 3, 3], b [64] fp32, x [B, T, 64] fp32, samples rows of
    (b, to, fo) -> fp32 [len(samples), 64]."""
    w = np.asarray(w, np.float32).reshape(64, 9).astype(np.float64)
    b = np.asarray(b, np.float32)
    xp = np.pad(np.asarray(x, np.float32), ((0, 0), (1, 1), (1, 1))).astype(np.float64)
    s = np.asarray(samples)
    out = np.zeros((len(s), 64), np.float32)
    for dt in range(2):
        for df in range(2):
            acc = np.zeros((len(s), 64), np.float32)
            for k in range(9):
                xv = xp[s[:, 0], 2 * s[:, 1] + dt + k // 3, 2 * s[:, 2] + df + k % 3]
                acc = _fma(acc, w[None, :, k], xv[:, None])
            out = np.maximum(out, np.maximum(acc + b[None, :], np.float32(0.0)))
    return out


def emulate_conv_pixels(w, b, x, pix):
    """conv.hip's header: chunks of 4 input channels ascending, the 9 taps of a
    chunk, its 4 channels ascending, one fma chain from zero, + bias, ReLU.
    w [Cout, Cin, 3, 3], b [Cout] fp32, x channels-last fp32 [B, T, F, Cin], pix
    rows of (b, t, f) -> fp32 [len(pix), Cout]."""
    w = np.asarray(w, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32)
    xp = np.pad(np.asarray(x, np.float32), ((0, 0), (1, 1), (1, 1), (0, 0))).astype(np.float64)
    pix = np.asarray(pix)
    cin = x.shape[3]
    acc = np.zeros((len(pix), w.shape[0]), np.float32)
    for chunk in range(cin // 4):
        for tap in range(9):
            a = xp[pix[:, 0], pix[:, 1] + tap // 3, pix[:, 2] + tap % 3]          # [N, Cin]
            for i in range(4 * chunk, 4 * chunk + 4):
                acc = _fma(acc, a[:, i, None], w[None, :, i, tap // 3, tap % 3])
    return np.maximum(acc + b[None, :], np.float32(0.0))


def emulate_conv(w, b, x, samples, epi):
    """A conv launch at sampled outputs.  epi 'store': samples (b, t, f); 'maxpool':
    samples (b, to, fo), the maximum of the window's four outputs; 'maxpool_fmean':
    samples (b, to), the four pooled bins p0..p3 and (((p0 + p1) + p2) + p3) * 0.25f."""
    s = np.asarray(samples)
    if epi == 'store':
        return emulate_conv_pixels(w, b, x, s)

    def pooled(sb, st, sf):
        pix = np.stack([np.stack([sb, 2 * st + dt, 2 * sf + df], axis=1) for dt in range(2) for df in range(2)])
        v = emulate_conv_pixels(w, b, x, pix.reshape(-1, 3)).reshape(4, len(sb), -1)
        return v.max(axis=0)

    if epi == 'maxpool':
        return pooled(s[:, 0], s[:, 1], s[:, 2])
    p = [pooled(s[:, 0], s[:, 1], np.full(len(s), j)) for j in range(4)]
    return ((((p[0] + p[1]).astype(np.float32) + p[2]).astype(np.float32) + p[3]).astype(np.float32)
            * np.float32(0.25)).astype(np.float32)


EPI_OF = {1: 'maxpool', 2: 'store', 3: 'maxpool', 4: 'store', 5: 'maxpool_fmean'}


def sample_outputs(shape, n, seed=0):
    """Up to n distinct index rows of an output [B, To, (Fo)] (channels excluded):
    the last row To - 1 of the first and last clip at bin 0 and at the last bin,
    and row 0, among them."""
    rng = np.random.default_rng(seed)
    total = int(np.prod(shape))
    idx = set(rng.choice(total, size=min(n, total), replace=False).tolist())
    last = int(np.prod(shape[1:]))
    idx |= {0, last - 1, total - 1, total - last}                       # first / last element of the first and last clip
    if len(shape) == 3:
        Fo = shape[2]
        idx |= {last - Fo, total - Fo, Fo - 1}                          # bin 0 of the last row; last bin of row 0
    idx = np.array(sorted(i for i in idx if 0 <= i < total))
    return np.stack(np.unravel_index(idx, shape), axis=1)


# ---------------------------------------------------------------------------
# launch_f_bn's shape choice (csrc/conv.hip), restated for the coverage asserts
# ---------------------------------------------------------------------------
def exact_launch_shape(B, T, F, cout, ncu):
    """'8-wave' / '4-wave' / 'small' for a launch_conv3x3 of B clips of T rows."""
    tt8, tt4 = 256 // F, 128 // F
    groups = cout // 128
    if B * ((T + tt8 - 1) // tt8) * groups >= 2 * ncu:
        return '8-wave'
    if B * ((T + tt4 - 1) // tt4) * groups >= 2 * ncu:
        return '4-wave'
    return 'small'


def layer_geometry(T):
    """(T, F, cout) of the five launch_conv3x3 launches of a T-frame input."""
    T1, T2, T3 = T // 2, T // 4, T // 8
    return [(T1, 32, 128), (T2, 16, 256), (T2, 16, 256), (T3, 8, 512), (T3, 8, 512)]


def kept_rows(T):
    """Input rows that can reach stage 55 of a T-frame input.  Each pooled row
    count Tk = T // 2^k keeps conv rows 0 .. 2 T(k+1) - 1 of level k, and a 3x3
    conv row r reads input rows r - 1 .. r + 1 clipped to the level's own row
    count (the bottom halo is zero padding, not the dropped row).  Walking back
    from stage 55: the rows of level k that matter are 0 .. need_k - 1."""
    counts = [T, T // 2, T // 4, T // 8, T // 16]          # rows of the log-mel and after each pool
    need = counts[4]                                       # pooled rows of conv4_2
    # (convs per level, from the last level back): level 3 has conv4_1, conv4_2; level 2 conv3_1, conv3_2;
    # level 1 conv2; level 0 conv1
    for level, nconv in ((3, 2), (2, 2), (1, 1), (0, 1)):
        rows = 2 * need                                    # conv rows the pool keeps
        for _ in range(nconv):
            rows = min(rows + 1, counts[level])            # each conv reads one row further down
        need = rows
    return need
