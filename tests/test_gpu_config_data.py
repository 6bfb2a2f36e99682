"""AllredConfig's result_vec, allred_run_io's buffers and ALLRED_CHECK_ALL=device on
the MI355X (one GPU, every rank a virtual rank on device 0).

- A reference-style C++ program (tests/config_data_prog.py, include/allred_helper.hpp alone)
  calls RunProgram and then validates cfg.result_vec ITSELF with the reference's
  validate_result_vector (allred_helper.hpp:92-93).
- t.run(argv, inputs=..., outputs=True): arbitrary data through every end-to-end mode
  (ALLRED_E2E / ALLRED_E2E_CHUNKS) equals the CPU oracle bit for bit.
- ALLRED_CHECK_ALL=device (k_validate on the memory the result lives in) reports the number
  ALLRED_CHECK_ALL=1 (N host passes) reports, on a passing and on a failing run."""
import numpy as np
import pytest

import oracle
import tenstorrentallreduce_amd as t

import config_data_prog as prog

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return prog.build(tmp_path_factory.mktemp("config_data_gpu"))


@pytest.mark.parametrize("name,variant,argv", [
    ("bo_2x2_one_tile", t.BO, ["1", "1", "2", "13", "1", "0", "0", "1"]),
    ("bo_2x2_last_core", t.BO, ["0", "1", "2", "13", "1", "0", "3", "1"]),
    ("bo_8x8_64_tiles", t.BO, ["1", "1", "8", "13", "1", "0", "0", "1"]),       # the P = 64 kernels
    ("bo_8x8_64_tiles_core_63", t.BO, ["1", "1", "8", "13", "1", "0", "63", "1"]),
    ("lo_4x4", t.LO, ["1", "1", "4", "13", "4", "0"]),
    ("mem_4x4", t.MEM, ["1", "1", "4", "13", "1", "0"]),
])
def test_program_validates_its_own_result_vec(exe, name, variant, argv):
    out, facts, _ = prog.run(exe, variant, argv, True, env={"ALLRED_BF16_ROUND": "rne"})
    assert out.strip() == "All values match!", out
    assert facts["result"] == facts["num_els"] == facts["src0"] and facts["mismatches"] == 0


@pytest.mark.parametrize("print_core,which", [("0", "eq1"), ("1", "eq0")])
def test_program_without_the_kernel_reads_back_its_input(exe, print_core, which):
    """RUN_KERNEL = 0: result_vec is the unreduced input of print_core — src_vec_1 for even x,
    src_vec_0 for odd x (allred_BO_2D.cpp:79-85)."""
    out, facts, _ = prog.run(exe, t.BO, ["1", "0", "2", "13", "1", "0", print_core, "1"], True,
                             env={"ALLRED_BF16_ROUND": "rne"})
    assert facts["result"] == facts["num_els"] and facts[which] == 1
    assert facts["eq0"] + facts["eq1"] == 1 and "Mismatch at index" in out


def random_bf16(total, n, seed):
    """random bf16 in [0, 100) (truncated floats)"""
    x = np.random.default_rng(seed).uniform(0.0, 100.0, (total, n)).astype(np.float32)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


@pytest.fixture(scope="module")
def oracle_case():
    """(variant name, algo, side) -> (inputs, the oracle's result), computed once per case."""
    cache = {}

    def get(vname, algo, side, n):
        key = (vname, algo, side, n)
        if key not in cache:
            total = side * side
            data = random_bf16(total, n, seed=100 * side + algo + len(vname))
            want = [r.copy() for r in data]
            oracle.allreduce(vname, algo, side, want, total)
            data.setflags(write=False)
            cache[key] = (data, np.stack(want))
        return cache[key]
    return get


def run_argv(vname, algo, side):
    s = str(algo)
    if vname == "mem":
        return t.MEM, ["x", s, "1", str(side), "13", "1", "0"]
    return t.BO, ["x", s, "1", str(side), "13", "1", "0", "0", "1" if vname == "bo" else "0"]


MODES = {"zerocopy": {"ALLRED_E2E": "zerocopy"},
         "dma": {"ALLRED_E2E": "dma", "ALLRED_E2E_CHUNKS": "1"},
         "dma_2_chunks": {"ALLRED_E2E": "dma", "ALLRED_E2E_CHUNKS": "2"}}
IO_CASES = [(v, a, 2, m) for v in ("bo", "lo", "mem") for a in (t.SWING, t.RECDUB) for m in ("zerocopy", "dma")]
IO_CASES += [("bo", a, 2, "dma_2_chunks") for a in (t.SWING, t.RECDUB)]
IO_CASES += [("bo", a, 8, m) for a in (t.SWING, t.RECDUB) for m in MODES]   # 64 ranks x 64 tiles


@pytest.mark.parametrize("vname,algo,side,mode", IO_CASES,
                         ids=[f"{v}-{'swing' if a else 'recdub'}-{s}x{s}-{m}" for v, a, s, m in IO_CASES])
def test_run_with_inputs_equals_the_oracle_in_every_mode(monkeypatch, oracle_case, vname, algo, side, mode):
    """Arbitrary data in, every rank's result out: the plan's bits whatever the end-to-end mode.
    (8x8 Swing BO under 2 chunks: its per-block trees differ, so the call takes one copy each
    way; the RecDub and 2x2 cases run the chunked form itself.)"""
    for k in ("ALLRED_E2E", "ALLRED_E2E_CHUNKS", "ALLRED_CHECK_ALL", "ALLRED_NODES", "ALLRED_GPUS", "ALLRED_EXEC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    variant, argv = run_argv(vname, algo, side)
    a = t.parse_args(argv, variant)
    n = a.num_tiles * 1024
    assert n % (8 * side * side * 2) == 0 or vname == "lo"      # the chunk rule at 2 chunks
    data, want = oracle_case(vname, algo, side, n)
    rep, out = t.run(argv, variant, inputs=data, outputs=True)
    assert rep.mismatches == -1
    bad = int((out != want).sum())
    assert bad == 0, f"{bad} of {out.size} elements differ"
    if mode == "dma_2_chunks" and (side == 2 or algo == t.RECDUB):
        assert rep.launches == 2      # the chunked form ran: one pass per chunk


@pytest.mark.parametrize("e2e", ["zerocopy", "dma", "dma_1_chunk"])
@pytest.mark.parametrize("run_kernel", ["1", "0"])
def test_check_all_device_counts_what_the_host_loop_counts(monkeypatch, e2e, run_kernel):
    """8x8 x 64 tiles at ERROR 0 under the RNE ctor: a passing run reports 0 both ways; with
    RUN_KERNEL = 0 (nearly every element of every rank wrong) both report the same total."""
    monkeypatch.setenv("ALLRED_BF16_ROUND", "rne")
    monkeypatch.setenv("ALLRED_E2E", e2e.split("_")[0])
    if e2e == "dma_1_chunk":
        monkeypatch.setenv("ALLRED_E2E_CHUNKS", "1")
    else:
        monkeypatch.delenv("ALLRED_E2E_CHUNKS", raising=False)
    argv = ["x", "1", run_kernel, "8", "13", "1", "0", "5", "1"]
    got = {}
    for mode in ("1", "device"):
        monkeypatch.setenv("ALLRED_CHECK_ALL", mode)
        got[mode] = t.run(argv, t.BO).mismatches
    assert got["device"] == got["1"]
    if run_kernel == "1":
        assert got["device"] == 0
    else:
        assert got["device"] > 63 * 65536 * 0.9
    monkeypatch.delenv("ALLRED_CHECK_ALL")
    one = t.run(argv, t.BO).mismatches     # print_core alone: the other 63 ranks are what the switch adds
    assert one <= got["device"] and (run_kernel == "1" or one < got["device"])
