"""Layer references of the two 14-layer models (test infrastructure only):
float64 / float32 restatements of pytorch/models.py:763-789 and :1155-1182,
one function per capturable step of the library (``sedx_set_capture``,
include/sedx.h), on the pattern of ``oracle/layer_refs.py`` whose functions are
imported where they fit (bn0, block 1, conv1 + bn1 + relu of any block, the
size-generic GRU / MultiHead / AttBlock of ``oracle/sed_oracle.py``).

CPU only; nothing here imports the library.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import layer_refs as R
from oracle import sed_oracle as O
from sedx import synth

GRU14, TRF14 = 'Cnn_14layers_Gru_FrameAtt', 'Cnn_14layers_Transformer_FrameAtt'
SEEDS = dict(synth.DEEP14_GOLDEN_SEEDS)
RATIO = 32                      # interpolate_ratio (models.py:741, :1133)
DEEP_CK = 16                    # csrc/conv_deep.hip: input channels per K chunk
KEYS = ('framewise_output', 'clipwise_output', 'embedding')
# capture ids in forward order (include/sedx.h): 8 = block 4 pooled, 40..43 = b5c1, b5 pooled, b6c1, b6 + freq mean
STAGES = (0, 2, 3, 4, 5, 6, 7, 8, 40, 41, 42, 43, 9)


def state(mt, dtype):
    return R.state(mt, 25, SEEDS[mt], dtype)


def geometry(T):
    """T frames -> (T5, out_frames): five floor halvings, x32, pad to a multiple of 100 unless 1000."""
    T5 = T // 2 // 2 // 2 // 2 // 2
    n = RATIO * T5
    return T5, n if n == 1000 or n % 100 == 0 else n + 100 - n % 100


def capture_shape(stage, B, T):
    T1, T2, T3 = T // 2, T // 4, T // 8
    T4, T5 = T3 // 2, T3 // 4
    if stage in (0, 2, 3, 4, 5, 6, 7):
        return R.capture_shape(stage, B, T)
    return {8: (B, T4, 4, 512), 40: (B, T4, 4, 1024), 41: (B, T5, 2, 1024), 42: (B, T5, 2, 2048),
            43: (B, T5, 2048), 9: (B, T5, 2048)}[stage]


def from_capture(stage, a):
    """Capture layout -> NCHW activations / [B, 2048, T5] (43) / [B, T5, 2048] (9)."""
    a = torch.as_tensor(a)
    if stage in (8, 40, 41, 42):
        return a.permute(0, 3, 1, 2).contiguous()
    if stage == 43:
        return a.transpose(1, 2).contiguous()
    return R.from_capture(stage, a)


def step_conv2(sd, k, x):
    """conv2 + bn2 + relu + pool of block k: 2x2 avg-pool (blocks 2-5), or block
    6's (1, 1) pool and the mean over its 2 bins -> [B, 2048, T5] (models.py:763-771)."""
    p = 'conv_block%d' % k
    x = F.relu(O._bn(sd, p + '.bn2', F.conv2d(x, O._t(sd[p + '.conv2.weight']), padding=1)))
    return torch.mean(x, dim=3) if k == 6 else F.avg_pool2d(x, kernel_size=(2, 2))


def conv_steps():
    """(previous stage, next stage, block, step) in capture order."""
    c1 = lambda k: (lambda sd, x: R.step_conv1(sd, k, x))
    c2 = lambda k: (lambda sd, x: step_conv2(sd, k, x))
    return [(0, 2, 1, R.step_block1), (2, 3, 2, c1(2)), (3, 4, 2, c2(2)), (4, 5, 3, c1(3)), (5, 6, 3, c2(3)),
            (6, 7, 4, c1(4)), (7, 8, 4, c2(4)), (8, 40, 5, c1(5)), (40, 41, 5, c2(5)), (41, 42, 6, c1(6)),
            (42, 43, 6, c2(6))]


def step_seq(sd, mt, x):
    """stage 43 [B, 2048, T5] -> stage 9 [B, T5, 2048]."""
    x = x.transpose(1, 2)
    return O.gru_bidirectional(sd, x) if mt == GRU14 else O.multihead(sd, x)


def step_gru_proj(sd, x):
    """[B, 2048, T5] -> the input projection G [B, T5, 6144] (forward | reverse, r | z | n each)."""
    x = x.transpose(1, 2)
    return torch.cat([torch.matmul(x, O._t(sd['gru.weight_ih_l0' + s]).t()) + O._t(sd['gru.bias_ih_l0' + s])
                      for s in ('', '_reverse')], dim=2)


def step_head(sd, mt, x):
    """stage 9 [B, T5, 2048] -> the three outputs (models.py:776-789, :1167-1182)."""
    x = x.transpose(1, 2)
    clipwise, _, cla = O.att_block(sd, x)
    fw = cla.transpose(1, 2)
    B, T, C = fw.shape
    fw = fw[:, :, None, :].repeat(1, 1, RATIO, 1).reshape(B, T * RATIO, C)
    if fw.shape[1] != 1000:
        n = O.roundup(fw.shape[1])
        fw = torch.cat([fw, fw[:, -1:, :].repeat(1, n - fw.shape[1], 1)], dim=1)
    return {'framewise_output': fw, 'clipwise_output': clipwise, 'embedding': cla if mt == GRU14 else x}


def chain(sd, mt, feat):
    """features [B, 64, T] -> the three outputs, every step in sd's dtype."""
    with torch.no_grad():
        x = R.step_bn0(sd, feat)
        for _, _, _, fn in conv_steps():
            x = fn(sd, x)
        return step_head(sd, mt, step_seq(sd, mt, x))


# ---------------------------------------------------------------------------
# csrc/conv_deep.hip's summation order, emulated in fp32 on the CPU
# ---------------------------------------------------------------------------
def chain_conv_fp32(sd, k, j, x, pixels):
    """conv j (1 or 2) + bn + relu of block k at ``pixels`` (rows of (b, t, f)
    of the UNPOOLED conv output) the way conv_deep_kernel accumulates it
    (csrc/conv_deep.hip header): BN folded into the weights in float64 and
    rounded once (csrc/weights.cpp), ONE in-order fma chain per output from zero
    over chunks of 16 input channels, the 9 taps of a chunk (row-major), its 16
    channels ascending; then + bias and ReLU.  ``sd`` float64, ``x`` fp32
    [B, Cin, T, F]; returns fp32 [len(pixels), Cout].  An fma is a float64
    product (exact for fp32 operands) and sum rounded to fp32."""
    p, bn = 'conv_block%d' % k, '.bn%d' % j
    s = O._t(sd[p + bn + '.weight']) / torch.sqrt(O._t(sd[p + bn + '.running_var']) + R.BN_EPS)
    w = (O._t(sd[p + '.conv%d.weight' % j]) * s[:, None, None, None]).float().double()
    b = (O._t(sd[p + bn + '.bias']) - O._t(sd[p + bn + '.running_mean']) * s).float()
    xp = F.pad(x.double(), (1, 1, 1, 1))
    pix = torch.as_tensor(pixels, dtype=torch.long)
    pb, pt, pf = pix[:, 0], pix[:, 1], pix[:, 2]
    taps = [xp[pb, :, pt + tap // 3, pf + tap % 3].numpy() for tap in range(9)]   # [N, Cin] each
    wn = w.numpy()
    acc64 = np.zeros((len(pix), w.shape[0]), np.float64)      # the fp32 accumulator, held as float64
    acc32 = np.zeros((len(pix), w.shape[0]), np.float32)
    tmp = np.empty_like(acc64)
    for chunk in range(x.shape[1] // DEEP_CK):
        c0 = DEEP_CK * chunk
        for tap in range(9):
            a = np.ascontiguousarray(taps[tap][:, c0:c0 + DEEP_CK].T)                  # [16, N]
            wt = np.ascontiguousarray(wn[:, c0:c0 + DEEP_CK, tap // 3, tap % 3].T)   # [16, Cout]
            for i in range(DEEP_CK):
                np.multiply(a[i][:, None], wt[i][None, :], out=tmp)
                np.add(acc64, tmp, out=acc64)
                acc32[...] = acc64                                                    # one rounding per fma
                acc64[...] = acc32
    acc = torch.from_numpy(acc32)
    return F.relu(acc + b[None, :])


# ---------------------------------------------------------------------------
# the 14-layer GRU's summation order, emulated in fp32 on the CPU
# ---------------------------------------------------------------------------
def _fma_chains(a, w):
    """[..., N, K] x [..., M, K] -> [..., N, M] fp32: every output ONE in-order
    fma chain from zero over k ascending (v_mfma_f32_32x32x2_f32 applied to
    ascending k pairs: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C))).  An fma is a
    float64 product (exact for fp32 operands) and sum rounded to fp32."""
    a64 = np.ascontiguousarray(np.moveaxis(np.asarray(a, np.float64), -1, 0))      # [K, ..., N]
    w64 = np.ascontiguousarray(np.moveaxis(np.asarray(w, np.float64), -1, 0))      # [K, ..., M]
    acc64 = np.zeros(a64.shape[1:] + w64.shape[-1:], np.float64)
    acc32 = acc64.astype(np.float32)
    tmp = np.empty_like(acc64)
    for k in range(a64.shape[0]):
        np.multiply(a64[k][..., :, None], w64[k][..., None, :], out=tmp)
        np.add(acc64, tmp, out=acc64)
        acc32[...] = acc64
        acc64[...] = acc32
    return acc32


def emulate_gru14(sd, x, clip, n):
    """Stage 9 of Cnn_14layers_Gru_FrameAtt on stage 43 ``x`` [B, 2048, T5]
    (fp32) the way the library sums it, for one clip: the forward direction's
    first n = min(n, T5) frames and the reverse direction's last n (each
    direction's h_t needs only the frames it has already walked).
      input projection (csrc/seq.hip, both GEMM kernels): per output ONE
        in-order fma chain over the 2048 k from zero, then + b_ih;
      recurrent product (csrc/gru1024.hip): four chains, one per K quarter of
        256, combined ((q0 + q1) + q2) + q3; step 0 has no product;
      gates as the kernel writes them, in fp32: r = sigmoid(gr + (ar + br)),
        z likewise, n = tanh(gn + r (an + bn)), h = n + z (h_prev - n), with
        numpy's fp32 exp / tanh (the device's differ by an ulp or two).
    ``sd`` float64.  Returns (fwd [n, 1024], rev [n, 1024]) fp32: frames
    0 .. n-1 of H[:, :1024] and frames T5-n .. T5-1 of H[:, 1024:]."""
    f32 = np.float32
    xt = x[clip].t().contiguous().numpy().astype(f32)                  # [T5, 2048]
    T5 = xt.shape[0]
    n = min(n, T5)
    sig = lambda v: (f32(1) / (f32(1) + np.exp(-v, dtype=f32))).astype(f32)
    out = []
    for sfx, rows in (('', xt[:n]), ('_reverse', xt[T5 - n:][::-1])):
        g = lambda name: O._t(sd['gru.' + name + '_l0' + sfx]).numpy().astype(f32)
        wih, whh, bih, bhh = g('weight_ih'), g('weight_hh'), g('bias_ih'), g('bias_hh')
        G = _fma_chains(rows, wih) + bih[None, :]                        # [n, 3072], in walking order
        wq = np.ascontiguousarray(whh.reshape(3072, 4, 256).transpose(1, 0, 2))   # [4, 3072, 256]
        h = np.zeros(1024, f32)
        hs = []
        for s in range(n):
            if s == 0:
                a = np.zeros(3072, f32)
            else:
                p = _fma_chains(h.reshape(4, 1, 256), wq)[:, 0, :]     # [4, 3072]
                a = ((p[0] + p[1]) + p[2]) + p[3]
            ab = a + bhh
            r = sig(G[s, :1024] + ab[:1024])
            z = sig(G[s, 1024:2048] + ab[1024:2048])
            nn = np.tanh(G[s, 2048:] + r * ab[2048:], dtype=f32)
            h = (nn + z * (h - nn)).astype(f32)
            hs.append(h)
        out.append(np.stack(hs))
    return torch.from_numpy(out[0]), torch.from_numpy(out[1][::-1].copy())


def emulate_step(sd, nxt, k, x, n_pix, seed=0):
    """The library's output of conv step -> ``nxt`` at up to ``n_pix`` sampled
    OUTPUT pixels, from chain_conv_fp32 and the kernel's epilogue
    (((v00 + v01) + (v10 + v11)) * 0.25 for the pools, (v0 + v1) * 0.5 for block
    6's frequency mean).  Returns (pixels (b, t, f) of the output [f = 0 for the
    mean], values fp32 [n, Cout])."""
    B, _, T, Fq = x.shape
    j = 1 if nxt in (40, 42) else 2
    if j == 1:
        pix = R.sample_pixels(B, T, Fq, n_pix, seed)
        return pix, chain_conv_fp32(sd, k, 1, x, pix)
    # the 2 (frequency mean) or 4 (pool) conv outputs behind every sampled output, in ONE chain run
    if nxt == 43:
        pix = R.sample_pixels(B, T, 1, n_pix, seed)
        offs = [(0, 0), (0, 1)]
        src = [np.stack([pix[:, 0], pix[:, 1], np.full(len(pix), f)], 1) for _, f in offs]
    else:
        pix = R.sample_pixels(B, T // 2, Fq // 2, n_pix, seed)
        offs = [(0, 0), (0, 1), (1, 0), (1, 1)]
        src = [np.stack([pix[:, 0], 2 * pix[:, 1] + dy, 2 * pix[:, 2] + dx], 1) for dy, dx in offs]
    v = chain_conv_fp32(sd, k, 2, x, np.concatenate(src, 0)).reshape(len(offs), len(pix), -1)
    if nxt == 43:
        return pix, (v[0] + v[1]) * np.float32(0.5)
    return pix, ((v[0] + v[1]) + (v[2] + v[3])) * np.float32(0.25)
