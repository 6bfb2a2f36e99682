"""tests/adamw_groups_cases.py tells a wrong group lookup from the right one (CPU, numpy only).

The GPU tests compare bits against adamw_ref.step with eff(group_of[i]).  That only proves the
per-bucket choice if a kernel that took ONE field from another group's set, or the group's own
max_norm instead of group 0's, would give different bits on these data.  Pinned here, for groups 1
and 2 on adamw_cases.planes(11, (8, 256)) with adamw_cases.norm_sq(8):
  one of the seven per-group fields replaced by another group's value changes at least 10 % of the
  new parameter plane's words and at least 0.5 % of the bf16 row elements;
  the group's own max_norm changes at least 10 % of the parameter plane.
Measured with exactly these values: the smallest single-field effect is eps, 21 % of the parameter
plane and 0.8 % of the rows; own-max_norm changes 65 % (group 1) and 89 % (group 2) of the
parameter plane.  The floors hold with margin.
"""
import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_ref

P = 8
DATA = adamw_cases.planes(11, (P, 256))
NSQ = adamw_cases.norm_sq(P)


def changed(h_a, h_b):
    """fractions of the new param plane's words and of the row elements that differ between two sets"""
    (pa, _, _, _), ra, _ = adamw_ref.step(*DATA, h_a, NSQ, P, False)
    (pb, _, _, _), rb, _ = adamw_ref.step(*DATA, h_b, NSQ, P, False)
    return float((pa.view(np.uint32) != pb.view(np.uint32)).mean()), float((ra != rb).mean())


def test_the_groups_differ_in_every_field():
    h = gc.hyper_array()
    assert h.shape == (3, 8) and h.dtype == np.float32
    for k in range(8):
        assert len({x.tobytes() for x in h[:, k]}) == 3, f"field {k}"
    for g in range(3):
        e = gc.eff(g)
        assert e[gc.MAX_NORM] == h[0, gc.MAX_NORM] and np.array_equal(e[:7], h[g, :7])
    u = adamw_ref.uniforms(gc.eff(1), NSQ, P)
    assert u["c"] < 1 and not u["skip"]   # clipping by group 0's max_norm is active on these data


@pytest.mark.parametrize("g", [1, 2])
def test_one_field_of_another_group_changes_the_result(g):
    smallest = (1.0, 1.0, None)
    for name, k in gc.FIELDS.items():
        for other in range(3):
            if other == g:
                continue
            mixed = gc.eff(g)
            mixed[k] = gc.GROUPS[other][k]
            planes, rows = changed(gc.eff(g), mixed)
            print(f"group {g}, {name} from group {other}: param plane {planes:.3f}, rows {rows:.4f}")
            assert planes >= 0.10 and rows >= 0.005, (g, name, other, planes, rows)
            smallest = min(smallest, (planes, rows, name))
    print(f"group {g}: smallest effect {smallest}")


@pytest.mark.parametrize("g", [1, 2])
def test_the_groups_own_max_norm_changes_the_result(g):
    planes, rows = changed(gc.eff(g), gc.GROUPS[g])
    print(f"group {g}, own max_norm: param plane {planes:.3f}, rows {rows:.4f}")
    assert planes >= 0.10
