"""tests/adamw_ref.py — the numpy float32 expectation of allred_plan_adamw_all_gather_shards_f32 —
pinned from two sides, on the CPU.  Neither side is the code under test.

1. Against torch.optim.AdamW(foreach=False, fused=False) on the CPU: 2^16 N(0, 1) parameters,
   lr 1e-3, betas (0.9, 0.999), eps 1e-8, weight decay 0.01, five steps.  The two differ by at most
   4.8e-7 absolute when measured (60 - 75 % of the elements bit-equal, the rest through lerp's
   rounding: torch forms m + (g - m) * o1 where the expectation writes m * beta1 + g * o1); the
   test allows 2e-6 absolute, four times that.
2. The case data (tests/adamw_cases.py) tell the right arithmetic from plausible wrong ones: each
   of adamw_ref.WRONG changes at least one bit of some plane or row in every case where it can.
   Fractions of the elements with a changed bit in p', m' or v', as measured on these data
   (printed by the test; `-s` shows them):
       case      fma     rcp     eps_first  decay_after  no_clip  seq_norm
       main     0.29    0.0056    0.093       0.16        0.98     0.28
       neg-v    0.30    0.0054    0.089       0.18        0.98     0.29
       eps0     0.20    0.0042    0 (eps = 0: the same arithmetic)  0.096  0.73  0.28
   `rcp` is the rare one: m' * (1 / den) is off by an ulp of the RATIO in about a quarter of the
   elements, and ss * ratio is some 1e-3 of p, so few of them reach p' — 23 of 4096 here, enough.
   The assertion is only that each is above zero where the variant is not degenerate.
"""
import numpy as np
import pytest

import adamw_cases
import adamw_ref
import f32_tree

SHAPE = (8, 512)
CASES = {   # name -> (planes, hyper); every one with clipping active (c < 1)
    "main": (adamw_cases.planes(1, SHAPE), adamw_cases.hyper()),
    "neg-v": (adamw_cases.negative_v(2, SHAPE), adamw_cases.hyper(step=1)),
    "eps0": (adamw_cases.zero_den(3, SHAPE), adamw_cases.hyper(step=7, eps=0.0)),
}
DEGENERATE = {("eps0", "eps_first")}   # eps = 0: adding it on either side of the division is the same


def differs(a, b):
    return ~((a.view(np.uint32) == b.view(np.uint32)) | (f32_tree.is_nan32(a) & f32_tree.is_nan32(b)))


def test_the_expectation_is_torchs_adamw():
    torch = pytest.importorskip("torch")
    n, lr, betas, eps, wd = 1 << 16, 1e-3, (0.9, 0.999), 1e-8, 0.01
    gen = torch.Generator().manual_seed(0)
    param = torch.nn.Parameter(torch.randn(n, generator=gen))
    opt = torch.optim.AdamW([param], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False, fused=False)
    p = param.detach().numpy().copy()
    m = np.zeros(n, dtype=np.float32)
    v = np.zeros(n, dtype=np.float32)
    for t in range(1, 6):
        grad = torch.randn(n, generator=gen)
        param.grad = grad.clone()
        opt.step()
        (p, _, m, v), _, _ = adamw_ref.step(p, grad.numpy(), m, v, adamw_cases.hyper(t, lr, betas, eps, wd, float("inf")), None, 8,
                                            False)
        want = param.detach().numpy()
        diff = float(np.abs(p - want).max())
        equal = float((p.view(np.uint32) == want.view(np.uint32)).mean())
        print(f"step {t}: max |expectation - torch| = {diff:.3g}, bit-equal {equal:.1%}")
        assert diff <= 2e-6
        state = opt.state[param]
        assert float(np.abs(m - state["exp_avg"].numpy()).max()) <= 2e-6
        assert float(np.abs(v - state["exp_avg_sq"].numpy()).max()) <= 2e-6


def test_the_planted_values_are_what_their_names_say():
    assert adamw_cases.P_PLANTED[5] == np.float32(3e38) and adamw_cases.G_PLANTED[5] == np.float32(1e20)
    p, g, m, v = CASES["main"][0]
    with np.errstate(all="ignore"):
        assert np.isinf(g * g).any() and (g == 0).any() and (v == 0).any()
    (p2, _, m2, v2), rows, info = adamw_ref.step(p, g, m, v, CASES["main"][1], adamw_cases.norm_sq(8), 8, False)
    big = np.abs(g) == np.float32(3e38)
    assert info[1] < 1 and info[2] == 0 and np.isinf(v2[big]).all()   # den = Inf: the step is +-0, p' = p * d
    with np.errstate(all="ignore"):
        assert np.array_equal(p2[big], (p * adamw_ref.uniforms(CASES["main"][1], None, 8)["d"])[big])
    (p2, _, _, _), _, _ = adamw_ref.step(*CASES["neg-v"][0], CASES["neg-v"][1], adamw_cases.norm_sq(8), 8, False)
    assert f32_tree.is_nan32(p2).any() and not f32_tree.is_nan32(p2).all()
    (p2, _, _, _), _, _ = adamw_ref.step(*CASES["eps0"][0], CASES["eps0"][1], adamw_cases.norm_sq(8), 8, False)
    assert f32_tree.is_nan32(p2).any() and np.isinf(p2).any()          # 0 / 0 and m' / 0


@pytest.mark.parametrize("P", [8, 16, 32, 64])
def test_the_norm_vector_tells_the_tree_from_the_left_to_right_sum(P):
    x = adamw_cases.norm_sq(P)
    right = adamw_ref.uniforms(adamw_cases.hyper(), x, P)
    wrong = adamw_ref.uniforms(adamw_cases.hyper(), x, P, wrong="seq_norm")
    assert right["N"] != wrong["N"] and right["c"] != wrong["c"] and right["c"] < 1
    assert np.isfinite(right["N"]) and not right["skip"]


@pytest.mark.parametrize("case", list(CASES))
def test_the_case_data_tell_the_arithmetic_from_wrong_ones(case):
    planes, hyper = CASES[case]
    nsq = adamw_cases.norm_sq(8)
    (p, _, m, v), rows, _ = adamw_ref.step(*planes, hyper, nsq, 8, False)
    line = []
    for wrong in adamw_ref.WRONG:
        (pw, _, mw, vw), rows_w, _ = adamw_ref.step(*planes, hyper, nsq, 8, False, wrong=wrong)
        frac = float(np.mean(differs(p, pw) | differs(m, mw) | differs(v, vw)))
        changed = frac > 0 or not f32_tree.same_bf16(rows, rows_w)
        line.append(f"{wrong} {frac:.2g}")
        assert changed or (case, wrong) in DEGENERATE, f"{case}: '{wrong}' gives the same bits as the right arithmetic"
    print(f"{case}: " + ", ".join(line))


def test_skip_and_no_norm():
    planes, hyper = CASES["main"]
    for bad in (np.inf, np.nan):
        nsq = adamw_cases.norm_sq(8)
        nsq[3] = bad
        for zero in (False, True):
            (p, g, m, v), rows, info = adamw_ref.step(*planes, hyper, nsq, 8, zero)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip((p, m, v), (planes[0], planes[2], planes[3])))
            assert np.array_equal(rows, f32_tree.bf16_rne(planes[0])) and info[2] == 1 and info[3] == 0
            assert (g.view(np.uint32) == 0).all() if zero else np.array_equal(g.view(np.uint32), planes[1].view(np.uint32))
    _, _, info = adamw_ref.step(*planes, hyper, None, 8, False)
    assert info.view(np.uint32).tolist() == [0, 0x3F800000, 0, 0]
