"""tools/isa_diff.py: its split, normalise and pair steps on two short hand-written texts.  No compiler runs."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_diff)

OLD = """
\t.text
\t.globl\t_Z5k_oneILi8EEvPf
\t.type\t_Z5k_oneILi8EEvPf,@function
_Z5k_oneILi8EEvPf:                      ; @_Z5k_oneILi8EEvPf
; %bb.0:
\tv_lshlrev_b32_e32 v0, 2, v0          ; a comment
\tv_add_f32_e32 v1, v1, v2
.LBB3_1:                                ; =>This Inner Loop Header
\tv_mul_f32_e32 v1, v1, v1
\ts_cbranch_scc1 .LBB3_1
\ts_endpgm
.Lfunc_end3:
\t.size\t_Z5k_oneILi8EEvPf, .Lfunc_end3-_Z5k_oneILi8EEvPf
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Z5k_oneILi8EEvPf
\t\t.amdhsa_group_segment_fixed_size 1024
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 3
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
\t.text
_Z5k_twov:
\tv_mov_b32_e32 v0, v1
\ts_endpgm
.Lfunc_end4:
\t.amdhsa_kernel _Z5k_twov
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 2
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
_Z6helperv:
\ts_setpc_b64 s[30:31]
.Lfunc_end5:
"""

# k_one: the same code behind other label numbers and comments; k_two: renamed, one constant materialised
NEW = OLD.replace(".LBB3_", ".LBB7_").replace(".Lfunc_end3", ".Lfunc_end9").replace("; a comment", "; another") \
         .replace("_Z5k_twov", "_Z6k_bothv").replace("v_mov_b32_e32 v0, v1", "v_mov_b32_e32 v0, 1.0")


def kernels(text):
    return {name: isa_diff.normalise(lines) for name, lines in isa_diff.split_kernels(text).items()}


def test_split_keeps_kernels_with_their_resource_block():
    ks = isa_diff.split_kernels(OLD)
    assert sorted(ks) == ["_Z5k_oneILi8EEvPf", "_Z5k_twov"]   # the helper has no .amdhsa_kernel block: no kernel
    one = isa_diff.normalise(ks["_Z5k_oneILi8EEvPf"])
    assert one[0] == "v_lshlrev_b32_e32 v0, 2, v0" and ".LBB_1:" in one and "s_cbranch_scc1 .LBB_1" in one
    assert not any(";" in s for s in one) and ".amdhsa_next_free_vgpr 3" in one and "v_mov_b32_e32 v0, v1" not in one
    assert isa_diff.resources(one) == {"vgpr": 3, "sgpr": 8, "lds": 1024, "scratch": 0}


def test_base_names():
    f = isa_diff.base_name
    assert f("void tsa::(anonymous namespace)::k_ag_group_f32<8>(tsa::GroupSpan, tsa::(anonymous namespace)::S)") == "k_ag_group_f32<8>"
    assert f("void tsa::(anonymous namespace)::k_tree_group_f32<16, true, tsa::(anonymous namespace)::NormArgs>(unsigned char const*)") \
        == "k_tree_group_f32<16, true, NormArgs>"
    assert f("k_plain(float*)") == "k_plain"
    assert isa_diff.rename("k_two", [("k_two", "k_both")]) == "k_both"
    assert isa_diff.rename("k_two<8, false>", [("k_two", "k_both")]) == "k_both<8, false>"
    assert isa_diff.rename("k_two_more<8>", [("k_two", "k_both")]) == "k_two_more<8>"


def test_pair_and_compare():
    old = {{"_Z5k_oneILi8EEvPf": "k_one<8>", "_Z5k_twov": "k_two"}[k]: v for k, v in kernels(OLD).items()}
    new = {{"_Z5k_oneILi8EEvPf": "k_one<8>", "_Z6k_bothv": "k_both"}[k]: v for k, v in kernels(NEW).items()}
    pairs, extra = isa_diff.pair(old, new)
    assert pairs == [("k_one<8>", "k_one<8>"), ("k_two", None)] and extra == ["k_both"]   # missing on either side
    pairs, extra = isa_diff.pair(old, new, [("k_two", "k_both")])
    assert pairs == [("k_one<8>", "k_one<8>"), ("k_two", "k_both")] and extra == []
    assert isa_diff.compare(old["k_one<8>"], new["k_one<8>"]) == (0, [])
    count, first = isa_diff.compare(old["k_two"], new["k_both"])
    assert count == 2 and sorted(first) == ["+v_mov_b32_e32 v0, 1.0", "-v_mov_b32_e32 v0, v1"]
