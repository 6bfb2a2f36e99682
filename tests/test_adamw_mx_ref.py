"""tests/adamw_mx_ref.py and tests/adamw_mx_cases.py on the CPU: the composition the GPU tests expect of
allred_plan_adamw_all_gather_shards_mxfp8, and — per mistake a correct-looking kernel could make — that
the GPU tests' data tells it from the right answer, as counts of MX blocks that come out differently."""
import numpy as np
import pytest

import adamw_cases
import adamw_groups_cases as gc
import adamw_mx_cases as mc
import adamw_mx_ref as ar
import adamw_ref
import mx_cases
import mxfp8_ref as ref

FLAGS = mc.FLAGS
POS = np.array([b[2] for b in mx_cases.BLOCKS])   # where every planted block holds its amax


def blocks_differing(a, b):
    """a, b = (element bytes, scale bytes): per MX block, does any of its 33 bytes differ"""
    return (a[0].reshape(-1, 32) != b[0].reshape(-1, 32)).any(axis=1) | (a[1].reshape(-1) != b[1].reshape(-1))


@pytest.mark.parametrize("zero,rceil", FLAGS)
def test_the_composition(zero, rceil):
    """planes: adamw_ref.step's; rows: mxfp8_ref.quantize of the new param plane"""
    total = 8
    nsq = adamw_cases.norm_sq(total)
    for g in range(3):
        d = adamw_cases.planes(3, (total, 768))
        planes, (e, s), info = ar.step(*d, gc.eff(g), nsq, total, zero, rceil)
        want, _, winfo = adamw_ref.step(*d, gc.eff(g), nsq, total, zero)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(planes, want))
        assert np.array_equal(info.view(np.uint32), winfo.view(np.uint32)) and info[2] == 0
        we, ws = ref.expected_rows(want[0], rceil)
        assert np.array_equal(e, we) and np.array_equal(s, ws) and e.shape == (total * 768,) and s.shape == (total * 24,)
        assert not np.array_equal(planes[0].view(np.uint32), d[0].view(np.uint32))


@pytest.mark.parametrize("zero", [False, True])
def test_identity_buckets_carry_every_planted_block_through_the_update(zero):
    """g = m = v = 0 in the group with weight_decay = 0: p' has p's bits (NaNs by class: the update may
    quiet a payload, the quantiser does not look at it), so the rows are mx_cases' expectation"""
    total, blk = 8, 768
    assert gc.GROUPS[mc.IDENTITY_GROUP][4] == 0
    nsq = adamw_cases.norm_sq(total)
    d = mc.identity(total, blk, 5)
    for rceil in (False, True):
        planes, (e, s), _ = ar.step(*d, gc.eff(mc.IDENTITY_GROUP), nsq, total, zero, rceil)
        assert np.array_equal(planes[0].view(np.uint32), d[0].view(np.uint32))
        assert (planes[2].view(np.uint32) == 0).all() and (planes[3].view(np.uint32) == 0).all()
        we, ws = ref.expected_rows(mx_cases.shard(total, blk, 5), rceil)
        assert np.array_equal(e, we) and np.array_equal(s, ws)
    # a block of 768 floats holds every planted block once, three tiles' worth: all eight positions of a tile are met
    assert blk // 32 == mx_cases.NBLOCKS and {m % 8 for m in range(mx_cases.NBLOCKS)} == set(range(8))


@pytest.mark.parametrize("seed", [7, 8])
@pytest.mark.parametrize("rceil", [False, True])
@pytest.mark.parametrize("group,least", [(16, 18), (8, 19), (4, 19)])
def test_an_amax_over_a_sub_group_shows(seed, rceil, group, least):
    """two DPP steps where the 8-lane block needs three give an amax over 16 elements; one step, or
    none, over 8 or 4.  Whichever sub-group's scale byte is reported: at least 18 / 19 / 19 of the 24
    planted blocks differ, blocks with the amax in elements 0-15 and in 16-31 both among them."""
    x = mx_cases.tile_blocks(seed).view(np.float32)
    right = ref.quantize(x, rceil)
    for pick in range(32 // group):
        d = blocks_differing(right, ar.quantize_sub(x, rceil, group, pick))
        assert d.sum() >= least, (pick, d.sum())
        assert (d & (POS < 16)).any() and (d & (POS >= 16)).any()
    # the whole block as its own "sub-group" is the rule itself
    assert not blocks_differing(right, ar.quantize_sub(x, rceil, 32)).any()


@pytest.mark.parametrize("rceil", [False, True])
def test_quantising_the_old_parameters_or_through_bf16_shows(rceil):
    total = 8
    nsq = adamw_cases.norm_sq(total)
    d = adamw_cases.planes(3, (total, 768))
    for g in range(3):
        right = ar.step(*d, gc.eff(g), nsq, total, False, rceil)[1]
        for wrong in ("old_p", "bf16"):
            n = blocks_differing(right, ar.step(*d, gc.eff(g), nsq, total, False, rceil, wrong=wrong)[1]).sum()
            assert n >= 64, (g, wrong, n)
    # and on the planted blocks a bf16 in between moves the SCALE byte of exactly 3 (floor) / 5 (RCEIL)
    for seed in (7, 8):
        x = mx_cases.tile_blocks(seed).view(np.float32)
        assert (ref.quantize(x, rceil)[1] != ref.quantize(ar.bf16_round(x), rceil)[1]).sum() == (5 if rceil else 3)


@pytest.mark.parametrize("seed", [7, 8])
def test_floor_and_rceil_differ_on_seven_planted_blocks(seed):
    x = mx_cases.tile_blocks(seed).view(np.float32)
    assert blocks_differing(ref.quantize(x, False), ref.quantize(x, True)).sum() == 7


@pytest.mark.parametrize("zero,rceil", FLAGS)
def test_a_skipped_step_quantises_p_and_keeps_the_planes(zero, rceil):
    total = 8
    nsq = adamw_cases.norm_sq(total).copy()
    nsq[3] = np.inf
    data = mc.make(total, 11)
    planes, rows, info = mc.expect(data, mc.GROUP_OF, nsq, total, zero, rceil)
    assert info[2] == 1
    for d, pl, (e, s) in zip(data, planes, rows):
        assert all(np.array_equal(pl[k].view(np.uint32), d[k].view(np.uint32)) for k in (0, 2, 3))
        assert (pl[1].view(np.uint32) == 0).all() if zero else np.array_equal(pl[1].view(np.uint32), d[1].view(np.uint32))
        we, ws = ref.expected_rows(d[0], rceil)
        assert np.array_equal(e, we) and np.array_equal(s, ws)
    # not skipped, the update buckets' rows are another thing
    _, rows2, info2 = mc.expect(data, mc.GROUP_OF, adamw_cases.norm_sq(total), total, zero, rceil)
    assert info2[2] == 0
    for i, (_, kind, _) in enumerate(mc.LIST):
        assert blocks_differing(rows[i], rows2[i]).any() == (kind != "identity")
