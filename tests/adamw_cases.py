"""The data of the AdamW tests (tests/test_adamw_ref.py on the CPU, tests/test_gpu_adamw_shards.py
on the GPU): plain numpy, seeded, no GPU and no library needed.

planes(seed, shape)      (p, g, m, v) float32 of `shape` = (blocks, blk), hard values planted at the head
                         and the tail of every block (both sides of every block boundary):
    p   N(0, 1) plus +-0, denormals, +-3e38 and bf16 ties (ties of p; p' rounds wherever it lands)
    g   N(0, 1) x 10^U{-6 .. 2} plus 0, denormals, 1e20 and 3e38 — g1^2 = Inf there (for 1e20 when the
        clip coefficient is 1, for 3e38 down to c = 1e-19), so den = Inf and the step is +-0
    m   small normal values
    v   >= 0, with planted 0 and denormals
negative_v(seed, shape)  the same with v < 0 in places: sqrtf gives NaN there — compare by class
zero_den(seed, shape)    g = 0 and v = 0 in places, for eps = 0: v' = 0, den = 0, m' / 0
norm_sq(P, seed)         a per-rank squared-norm vector on which the balanced tree and the
                         left-to-right sum differ (asserted in test_adamw_ref.py)
hyper(step, ...)         the eight float32 of allred_adamw_hyper, computed as
                         tenstorrentallreduce_amd.adamw_hyper does (float64, rounded once)
"""
import numpy as np

F = np.float32

P_PLANTED = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000,      # signed zeros, denormals
                      0x7F61B1E6, 0xFF61B1E6,                                            # +-3e38
                      0x3F808000, 0x3F818000, 0xBF808000, 0x3F807FFF, 0x3F808001],       # bf16 ties and their neighbours
                     dtype=np.uint32).view(F)
G_PLANTED = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000100, 0x007FFFFF,      # zeros, denormals
                      0x60AD78EC, 0xE0AD78EC,                                            # +-1e20: the square overflows
                      0x7F61B1E6, 0xFF61B1E6],                                           # +-3e38: (g c)^2 overflows under clipping too
                     dtype=np.uint32).view(F)
V_PLANTED = np.array([0x00000000, 0x00000001, 0x00000100, 0x007FFFFF], dtype=np.uint32).view(F)


def _plant(a, vals, shift=0):
    """vals at the head of every block (from column `shift`) and, reversed, at its tail"""
    k = len(vals)
    a[:, shift:shift + k] = vals
    a[:, a.shape[1] - shift - k:a.shape[1] - shift] = vals[::-1]
    return a


def planes(seed, shape):
    rng = np.random.default_rng(seed)
    p = _plant(rng.standard_normal(shape).astype(F), P_PLANTED)
    g = (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 3, shape)).astype(F)
    g = _plant(g, G_PLANTED, shift=3)   # not column for column on p's planted values
    m = (rng.standard_normal(shape) * 1e-2).astype(F)
    v = _plant(((rng.standard_normal(shape) * 1e-2) ** 2).astype(F), V_PLANTED, shift=5)
    assert (v >= 0).all()
    return p, g, m, v


def negative_v(seed, shape):
    p, g, m, v = planes(seed, shape)
    rng = np.random.default_rng(seed + 1)
    neg = rng.random(shape) < 0.25
    v = np.where(neg, -np.abs(v) - F(1e-3), v).astype(F)   # large enough that v' stays below zero
    return p, g, m, v


def zero_den(seed, shape):
    p, g, m, v = planes(seed, shape)
    rng = np.random.default_rng(seed + 2)
    z = rng.random(shape) < 0.25
    g = np.where(z, F(0.0), g).astype(F)
    v = np.where(z, F(0.0), v).astype(F)
    m[:, ::7] = 0.0   # some of them with m = 0 too: 0 / 0
    return p, g, m, v


def norm_sq(P, seed=0):
    """the first vector of a seeded sequence whose balanced tree and left-to-right sum differ, and with
    them the clip coefficient for max_norm = 1"""
    rng = np.random.default_rng(1000 + 10 * P + seed)
    while True:
        x = (rng.standard_normal(P) ** 2 * 10.0 ** rng.integers(-2, 3, P)).astype(F)
        pad = np.zeros(64, dtype=F)
        pad[:P] = x
        while pad.shape[0] > 1:
            pad = pad[0::2] + pad[1::2]
        seq = F(0.0)
        for t in x:
            seq = F(seq + t)
        if pad[0] != seq and F(1.0) / (np.sqrt(pad[0]) + F(1e-6)) != F(1.0) / (np.sqrt(seq) + F(1e-6)):
            return x


def hyper(step=3, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=1.0):
    bc1 = 1.0 - betas[0] ** step
    bc2_sqrt = float(np.sqrt(np.float64(1.0 - betas[1] ** step)))
    return np.array([lr, betas[0], betas[1], eps, weight_decay, bc1, bc2_sqrt, max_norm], dtype=F)
