"""Reference restatement of the average-precision definition (include/sedx.h),
CPU only: numpy int64 / float64 and ``math.fsum``.  Imports nothing from the
library under test.

For one class: order by float32 value descending (``-0.0 == +0.0``, denormals
distinct), distinct thresholds t_1 > ... > t_K, n_k = #{s >= t_k}, tp_k =
#{s >= t_k, y = 1}, P = tp_K, AP = sum_k ((tp_k - tp_{k-1}) / P) (tp_k / n_k);
P = 0 gives NaN.  ``ap_exact`` rounds the exact rational sum of the float64
terms once (fsum); the tolerance every comparison uses is ``bound(K)``.
"""
import math

import numpy as np


def bound(K):
    """|ap - reference| <= 8 (K + 4) 2^-53: both sides round each of K terms a
    few times and sum K non-negative terms of total <= 1 in float64."""
    return 8.0 * (int(K) + 4) * 2.0 ** -53


def curve(target, scores):
    """One class: (thresholds float32 [K] descending, tp int64 [K], n int64 [K])."""
    s = np.asarray(scores, np.float32).ravel()
    y = (np.asarray(target).ravel() != 0).astype(np.int64)
    s = np.where(s == 0, np.float32(0.0), s)                # -0.0 and +0.0: one threshold, reported as +0.0
    order = np.argsort(-s.astype(np.float64), kind='stable')   # float64 negation is exact, denormals kept
    s, y = s[order], y[order]
    ends = np.flatnonzero(np.append(s[1:] != s[:-1], True))
    tp = np.cumsum(y)[ends]
    return s[ends], tp.astype(np.int64), (ends + 1).astype(np.int64)


def terms(tp, n):
    P = int(tp[-1])
    prev = np.concatenate([[0], tp[:-1]])
    return ((tp - prev).astype(np.float64) / np.float64(P)) * (tp.astype(np.float64) / n.astype(np.float64))


def ap_exact(target, scores):
    """(AP rounded once from the float64 terms, P, K) of one class; NaN for P = 0."""
    thr, tp, n = curve(target, scores)
    P, K = int(tp[-1]), len(tp)
    if P == 0:
        return float('nan'), P, K
    return math.fsum(terms(tp, n).tolist()), P, K


def all_classes(target, scores):
    """[M, C] inputs -> (ap float64 [C], info int64 [C, 3] with a zero
    non-finite count, curves list of (thr, tp, n))."""
    target, scores = np.asarray(target), np.asarray(scores)
    C = scores.shape[1]
    ap = np.empty(C, np.float64)
    info = np.zeros((C, 3), np.int64)
    curves = []
    for c in range(C):
        ap[c], info[c, 0], info[c, 1] = ap_exact(target[:, c], scores[:, c])
        curves.append(curve(target[:, c], scores[:, c]))
    return ap, info, curves


# ---- seeded generators (shared by the CPU and the GPU tests) ----------------

def make_case(M, C, seed, kind='uniform', empty=None, full=None):
    """(target uint8 [M, C], scores float32 [M, C]).  Every class gets at
    least one positive except `empty` (P = 0, on purpose); `full` has P = M.
    kinds: uniform (distinct-ish), coarse (many ties), x8 (each value repeated
    eight times along the samples, as the models' frame interpolation does),
    ascending / descending (already sorted), mixed (signs, +-0.0, denormals),
    equal (one value)."""
    rng = np.random.RandomState(seed)
    if kind == 'uniform':
        s = rng.rand(M, C).astype(np.float32)
    elif kind == 'coarse':
        s = (rng.randint(0, 17, size=(M, C)) / np.float32(16)).astype(np.float32)
    elif kind == 'x8':
        s = np.repeat(rng.rand((M + 7) // 8, C).astype(np.float32), 8, axis=0)[:M]
    elif kind in ('ascending', 'descending'):
        s = np.sort(rng.rand(M, C).astype(np.float32), axis=0)
        if kind == 'descending':
            s = s[::-1]
    elif kind == 'mixed':
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-45, 1e-39, -1e-39, 1.5, -1.5, 0.25, -0.25, 1e-38, 1.0e30,
                         -1.0e30], np.float32)
        s = np.where(rng.rand(M, C) < 0.5, pool[rng.randint(0, len(pool), size=(M, C))],
                     rng.randn(M, C).astype(np.float32))
    elif kind == 'equal':
        s = np.full((M, C), 0.3, np.float32)
    else:
        raise ValueError(kind)
    s = np.ascontiguousarray(s, dtype=np.float32)
    t = (rng.rand(M, C) < 0.3).astype(np.uint8)
    t[rng.randint(0, M, size=C), np.arange(C)] = 1           # one positive everywhere
    if full is not None:
        t[:, full] = 1
    if empty is not None:
        t[:, empty] = 0
    return t, s


def digit_case(M, C, byte, seed):
    """Scores whose bit patterns differ only in byte `byte` (0 = lowest): one
    radix pass decides the order.  All finite (byte 3 keeps the exponent's top
    bits away from 0xff)."""
    rng = np.random.RandomState(seed)
    base = np.uint32(0x3e8a5c31)                            # 0.27...
    if byte == 3:
        vals = rng.choice(np.array([0x00, 0x01, 0x3e, 0x3f, 0x40, 0x7e, 0x80, 0x81, 0xbe, 0xbf, 0xc0, 0xfe],
                                   np.uint32), size=(M, C))
    else:
        vals = rng.randint(0, 256, size=(M, C)).astype(np.uint32)
    mask = np.uint32(0xff) << np.uint32(8 * byte)
    bits = (base & ~mask) | (vals << np.uint32(8 * byte))
    s = np.ascontiguousarray(bits.astype(np.uint32)).view(np.float32)
    t = (rng.rand(M, C) < 0.3).astype(np.uint8)
    t[rng.randint(0, M, size=C), np.arange(C)] = 1
    return t, s
