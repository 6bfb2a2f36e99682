"""AllredConfig carries its inputs and its result (allred_helper.hpp:63-65,
allred_helper.cpp:277-285, allred_helper.hpp:84-96), allred_run_io hands the
data of a run to the caller, and allred_validate_device refuses bad arguments —
all without a GPU: the runs go over the host twin (ALLRED_TRANSPORT=host)."""
import ctypes as C
import os

import numpy as np
import pytest

import tenstorrentallreduce_amd as t
from tenstorrentallreduce_amd import _lib

import config_data_prog as prog
from multi_cases import random_inputs
from test_oracle import fnv1a64

ONES = 0x3F803F80   # two bf16 1.0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return prog.build(tmp_path_factory.mktemp("config_data"))


def golden(golden_inputs, seed, nbytes, rnd):
    (v,) = [v for v in golden_inputs["vectors"] if (v["seed"], v["bytes"], v["round"]) == (seed, nbytes, rnd)]
    return v


@pytest.mark.parametrize("rnd", ["trunc", "rne"])
@pytest.mark.parametrize("argv,nbytes", [(["1", "0", "1", "13", "1"], 2048),                      # one tile
                                         (["1", "0", "8", "13", "5", "32", "0", "1"], 655360)])  # config 2
def test_constructor_fills_the_reference_input_vectors(exe, tmp_path, golden_inputs, argv, nbytes, rnd):
    """src_vec_0 / src_vec_1 = create_random_vector_of_bfloat16(2048 * NUM_TILES, 100, RND_SRC / RND_SRC + 1)
    (allred_helper.cpp:283-284): the libstdc++ fixtures of seeds 13 and 14, truncating ctor by
    default and RNE under ALLRED_BF16_ROUND=rne; result_vec stays empty until RunProgram, and
    TOTAL_NUM_TILES is never assigned (declared at allred_helper.hpp:54 only)."""
    env = {"ALLRED_BF16_ROUND": "rne"} if rnd == "rne" else {}
    _, facts, words = prog.run(exe, t.BO, argv, False, env=env, dump=str(tmp_path / "d.bin"))
    n = nbytes // 4
    assert (facts["src0"], facts["src1"], facts["result"], facts["num_els"]) == (n, n, 0, n)
    assert facts["total_num_tiles"] == 0
    assert words.size == 2 * n
    for vec, seed in ((words[:n], 13), (words[n:], 14)):
        want = golden(golden_inputs, seed, nbytes, rnd)
        assert [int(x) for x in vec[:16]] == want["head"]
        assert fnv1a64(vec) == want["fnv1a64"]


def test_constructor_seed_minus_one_is_all_ones_and_a_zero_result(exe, tmp_path):
    """RND_SRC < 0 (allred_helper.cpp:278-281): both inputs the constant 1.0, result_vec num_els zero words."""
    _, facts, words = prog.run(exe, t.BO, ["1", "0", "2", "-1", "3"], False, dump=str(tmp_path / "d.bin"))
    n = facts["num_els"]
    assert n == 4 * 512 and (facts["src0"], facts["src1"], facts["result"]) == (n, n, n)   # LO: 3 tiles -> 4
    assert facts["total_num_tiles"] == 0
    assert (words[:2 * n] == ONES).all() and (words[2 * n:] == 0).all() and words.size == 3 * n


# tests/multi_cases.py config3_recdub_bo (BASELINE config 3: 4x2 RecDub BO, 8 ranks), which
# tests/test_multi_host.py's CASES run at G = 2; ERROR (argv[6]) = 0
HOST_ENV = {"ALLRED_TRANSPORT": "host", "ALLRED_GPUS": "2", "ALLRED_BF16_ROUND": "rne", "ALLRED_NODES": "8"}


def config3(seed="13", print_core="0"):
    return ["0", "1", "4", seed, "40", "0", print_core, "1"]


@pytest.mark.parametrize("seed,print_core", [("13", "0"), ("13", "7"), ("-1", "0")])
def test_runprogram_reads_the_result_back_on_the_host_twin(exe, tmp_path, monkeypatch, seed, print_core):
    """RunProgram leaves print_core's result in result_vec (allred_helper.hpp:92): the caller's own
    validate_result_vector call on cfg.result_vec / cfg.src_vec_* prints "All values match!" at
    ERROR 0 under the RNE ctor.  No HIP call is made (host transport)."""
    out, facts, words = prog.run(exe, t.BO, config3(seed, print_core), True, env=HOST_ENV,
                                 dump=str(tmp_path / "d.bin"))
    n = facts["num_els"]
    assert n == 320 * 512 and facts["nodes"] == 8
    assert out.strip() == "All values match!", out
    assert facts["result"] == n and facts["mismatches"] == 0
    assert facts["result_before"] == (n if seed == "-1" else 0)
    if seed == "-1":   # every element is N = 8
        assert (words[2 * n:] == 0x41004100).all()
    else:              # and it is what allred_run_multi returns for that rank
        for k, v in HOST_ENV.items():
            monkeypatch.setenv(k, v)
        _, want = t.run_multi(["x", *config3(seed, print_core)], t.BO, transport=t.TRANSPORT_HOST)
        assert np.array_equal(words[2 * n:].view(np.uint16), want[int(print_core)])


def test_run_outputs_and_inputs_on_the_host_transport(monkeypatch):
    """t.run(..., outputs=True) / inputs= (allred_run_io) with ALLRED_GPUS set: the buffers are
    forwarded to allred_run_multi on the transport the environment names."""
    for k, v in HOST_ENV.items():
        monkeypatch.setenv(k, v)
    argv = ["x", *config3()]
    assert isinstance(t.run(argv, t.BO), _lib.Report)            # neither argument: the Report alone
    rep, out = t.run(argv, t.BO, outputs=True)
    rep_m, out_m = t.run_multi(argv, t.BO, transport=t.TRANSPORT_HOST)
    assert rep.mismatches == rep_m.mismatches == 0
    assert out.shape == (8, 320 * 1024) and np.array_equal(out, out_m)
    data = random_inputs(8, 320 * 1024, seed=5)
    rep, out = t.run(argv, t.BO, inputs=data, outputs=True)
    _, out_m = t.run_multi(argv, t.BO, transport=t.TRANSPORT_HOST, inputs=data)
    assert rep.mismatches == -1 and np.array_equal(out, out_m) and not np.array_equal(out, data)
    rep, none = t.run(argv, t.BO, inputs=data)
    assert rep.mismatches == -1 and none is None
    with pytest.raises(ValueError):
        t.run(argv, t.BO, inputs=data[:, :-8], outputs=True)
    with pytest.raises(ValueError):
        t.run(argv, t.BO, inputs=data[:7])


def test_run_io_result_vec_is_print_core_row(monkeypatch):
    """allred_run_io's result_vec = print_core's row of out_all, also without out_all."""
    for k, v in HOST_ENV.items():
        monkeypatch.setenv(k, v)
    a = t.parse_args(["x", *config3(print_core="5")], t.BO)
    n = a.num_tiles * 1024
    data = random_inputs(8, n, seed=6)
    out = np.zeros((8, n), dtype=np.uint16)
    res = np.zeros(n // 2, dtype=np.uint32)
    r = _lib.Report()
    t.check(_lib.lib.allred_run_io(C.byref(a), 0, C.byref(r), data.ctypes.data, out.ctypes.data, res.ctypes.data))
    assert np.array_equal(res.view(np.uint16), out[5])
    res2 = np.zeros(n // 2, dtype=np.uint32)
    t.check(_lib.lib.allred_run_io(C.byref(a), 0, C.byref(r), data.ctypes.data, None, res2.ctypes.data))
    assert np.array_equal(res2, res)


def test_validate_device_refuses_bad_arguments_without_a_gpu():
    """A null out, n = 12 and rows = 0 are ALLRED_ERR_ARG before any launch (and before any HIP call)."""
    p = 0x10000   # never dereferenced
    rec = (_lib.RankCheck * 4)()
    f = _lib.lib.allred_validate_device
    assert f(p, 16, 16, 1, p, p, 2.0, 0.0, 0, None, None) == _lib.ERR_ARG
    assert f(p, 16, 12, 1, p, p, 2.0, 0.0, 0, rec, None) == _lib.ERR_ARG
    assert f(p, 16, 16, 0, p, p, 2.0, 0.0, 0, rec, None) == _lib.ERR_ARG
    assert f(None, 16, 16, 1, p, p, 2.0, 0.0, 0, rec, None) == _lib.ERR_ARG
    assert f(p, 8, 16, 1, p, p, 2.0, 0.0, 0, rec, None) == _lib.ERR_ARG      # stride < n
    assert f(p, 16, 16, 65, p, p, 2.0, 0.0, 0, rec, None) == _lib.ERR_ARG    # rows > ALLRED_MAX_NODES
    with pytest.raises(t.AllredError):
        t.validate_device(p, 16, 12, 1, p, p, 2.0, 0.0)


def test_rank_check_layout_matches_the_header(tmp_path):
    """allred_rank_check as _lib.RankCheck mirrors it (a compiled offsetof program)."""
    import subprocess
    src = tmp_path / "layout.cpp"
    fields = [f for f, _ in _lib.RankCheck._fields_]
    body = "".join(f'    std::printf("{f} %zu\\n", offsetof(allred_rank_check, {f}));\n' for f in fields)
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "allred.h"\nint main() {\n'
                   '    std::printf("size %zu\\n", sizeof(allred_rank_check));\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(prog.ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.RankCheck) == 24
    for f in fields:
        assert int(got[f]) == getattr(_lib.RankCheck, f).offset, f
