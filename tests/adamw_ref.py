"""What allred_plan_adamw_all_gather_shards_f32 must compute, in numpy float32 (plain module, no
GPU, no library needed), on top of tests/f32_tree.py.  numpy's float32 arithmetic is IEEE: one
rounding per operation, division and square root correctly rounded, no fma, no flushing.

hyper: the eight float32 of allred_adamw_hyper — lr, beta1, beta2, eps, weight_decay, bias_corr1,
bias_corr2_sqrt, max_norm (tenstorrentallreduce_amd.adamw_hyper makes them).

uniforms(hyper, norm_sq, P)                         the call's uniform values as a dict: N, c, skip, d, o1, o2, ss
step(p, g, m, v, hyper, norm_sq, P, zero_grad)      arrays of any one shape -> ((p', g', m', v'), rows, info):
                                                    the planes after the call, rows = bf16_rne(p') as uint16
                                                    (f32_tree.bf16_rne), info = the four float32

The alternatives a correct-looking kernel could compute instead (tests/test_adamw_ref.py pins that
the GPU tests' data tells them apart) are `wrong=` of both functions: "fma", "rcp", "eps_first",
"decay_after", "no_clip", "seq_norm".
"""
import numpy as np

import f32_tree

LANES = 64
F = np.float32
WRONG = ("fma", "rcp", "eps_first", "decay_after", "no_clip", "seq_norm")


def tree64(x):
    """the balanced binary tree, in index order, over x padded with +0.0f to 64 values"""
    pad = np.zeros(LANES, dtype=F)
    pad[:len(x)] = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        while pad.shape[0] > 1:
            pad = pad[0::2] + pad[1::2]
    assert pad.dtype == F
    return pad[0]


def uniforms(hyper, norm_sq, P, wrong=None):
    lr, beta1, beta2, eps, wd, bc1, bc2, max_norm = np.asarray(hyper, dtype=F)
    with np.errstate(all="ignore"):
        if norm_sq is None:
            N, c, skip = F(0.0), F(1.0), False
        else:
            x = np.asarray(norm_sq, dtype=F)
            assert x.shape == (P,)
            if wrong == "seq_norm":
                N = F(0.0)
                for t in x:
                    N = F(N + t)
            else:
                N = tree64(x)
            skip = not bool(np.isfinite(N))
            q = F(max_norm / F(np.sqrt(N) + F(1e-6)))
            c = q if q < F(1.0) else F(1.0)
        u = dict(N=N, c=c, skip=skip, d=F(F(1.0) - F(lr * wd)), o1=F(F(1.0) - beta1), o2=F(F(1.0) - beta2), ss=F(lr / bc1),
                 beta1=beta1, beta2=beta2, eps=eps, bc2=bc2)
    assert all(isinstance(u[k], np.float32) for k in u if k != "skip")
    return u


def _fma(a, b, c):
    """round32(a * b + c) for float32 a, b, c: the product is exact in float64; the sum is rounded to
    float64 and then to float32 — double rounding apart, which is rare and irrelevant for a test that
    only needs SOME difference"""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)


def step(p, g, m, v, hyper, norm_sq, P, zero_grad, wrong=None):
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    u = uniforms(hyper, norm_sq, P, wrong)
    info = np.array([u["N"], u["c"], 1.0 if u["skip"] else 0.0, 0.0], dtype=F)
    g_out = np.zeros_like(g) if zero_grad else g.copy()
    if u["skip"]:
        return (p.copy(), g_out, m.copy(), v.copy()), f32_tree.bf16_rne(p), info
    with np.errstate(all="ignore"):
        g1 = g if wrong == "no_clip" else g * u["c"]
        p1 = p * u["d"]
        if wrong == "fma":
            m2 = _fma(m, u["beta1"], g1 * u["o1"])
            v2 = _fma(v, u["beta2"], (g1 * g1) * u["o2"])
        else:
            m2 = m * u["beta1"] + g1 * u["o1"]
            v2 = v * u["beta2"] + (g1 * g1) * u["o2"]
        if wrong == "eps_first":
            den = (np.sqrt(v2) + u["eps"]) / u["bc2"]
        else:
            den = np.sqrt(v2) / u["bc2"] + u["eps"]
        ratio = m2 * (F(1.0) / den) if wrong == "rcp" else m2 / den
        if wrong == "decay_after":
            p2 = (p - u["ss"] * ratio) * u["d"]
        else:
            p2 = p1 - u["ss"] * ratio
    assert p2.dtype == F and m2.dtype == F and v2.dtype == F
    return (p2, g_out, m2, v2), f32_tree.bf16_rne(p2), info
