"""Shared by tests/test_config_data.py (CPU) and tests/test_gpu_config_data.py
(GPU): one reference-style C++ program against include/allred_helper.hpp alone
(plain g++, no HIP header), the way a caller who moves over from the
reference's AllredConfig (allred_helper.hpp:47-97) would write it.

    prog <variant> <dump file or -> <run: 0|1> <reference argv[1..]>

builds AllredConfig(argv, variant, device 0), optionally calls
RunProgram(false), then validates cfg.result_vec ITSELF with the reference's
validate_result_vector (its printed report is the program's stdout) and prints
one line of facts.  The dump file receives src_vec_0 | src_vec_1 | result_vec
as raw little-endian words."""
import os
import subprocess

import numpy as np

from tenstorrentallreduce_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r'''
#include "allred_helper.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int variant = std::atoi(argv[1]);
    const char* dump = argv[2];
    const bool run = std::atoi(argv[3]) != 0;
    argv[3] = argv[0];   // the reference's argv layout from here on
    AllredConfig cfg(argc - 3, argv + 3, variant, 0);
    if (cfg.status != ALLRED_OK) return 3;
    const std::size_t before = cfg.result_vec.size();
    if (run) {
        if (cfg.RunProgram(false) != ALLRED_OK) {
            std::printf("status %d result_size %zu\n", cfg.status, cfg.result_vec.size());
            return 4;
        }
        validate_result_vector(cfg.result_vec, cfg.src_vec_0, cfg.src_vec_1, cfg.num_els, cfg.ERROR, cfg.TOTAL_NODES);
    }
    std::printf("\nfacts src0 %zu src1 %zu result_before %zu result %zu num_els %d total_num_tiles %d nodes %u "
                "mismatches %lld eq0 %d eq1 %d\n",
                cfg.src_vec_0.size(), cfg.src_vec_1.size(), before, cfg.result_vec.size(), cfg.num_els,
                cfg.TOTAL_NUM_TILES, cfg.TOTAL_NODES, (long long)cfg.report.mismatches,
                (int)(cfg.result_vec == cfg.src_vec_0), (int)(cfg.result_vec == cfg.src_vec_1));
    if (std::strcmp(dump, "-") != 0) {
        FILE* f = std::fopen(dump, "wb");
        if (!f) return 5;
        std::fwrite(cfg.src_vec_0.data(), 4, cfg.src_vec_0.size(), f);
        std::fwrite(cfg.src_vec_1.data(), 4, cfg.src_vec_1.size(), f);
        std::fwrite(cfg.result_vec.data(), 4, cfg.result_vec.size(), f);
        std::fclose(f);
    }
    return 0;
}
'''


def build(tmp_dir) -> str:
    """Compile the program the way test_allred_helper_hpp_compiles_and_runs does; returns its path."""
    src = os.path.join(str(tmp_dir), "config_data.cpp")
    exe = os.path.join(str(tmp_dir), "config_data")
    with open(src, "w") as f:
        f.write(SOURCE)
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", f"-I{ROOT}/include", src, "-o", exe, f"-L{lib_dir}", "-lallred",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


EXT_ENV = ("ALLRED_TRANSPORT", "ALLRED_GPUS", "ALLRED_BF16_ROUND", "ALLRED_NODES", "ALLRED_EXEC", "ALLRED_E2E",
           "ALLRED_E2E_CHUNKS", "ALLRED_CHECK_ALL", "ALLRED_DEVICE", "ALLRED_MEM_ACC", "ALLRED_SHARE_GPU",
           "ALLRED_PROFILE_LOG")


def run(exe, variant, argv, run_program, env=None, dump=None, timeout=300):
    """Returns (stdout lines before the facts line, facts dict, dumped words or None)."""
    e = {k: v for k, v in os.environ.items() if k not in EXT_ENV}
    e.update(env or {})
    p = subprocess.run([exe, str(variant), dump or "-", "1" if run_program else "0", *map(str, argv)],
                       capture_output=True, text=True, env=e, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    head, _, tail = p.stdout.rpartition("\nfacts ")
    tok = tail.split()
    facts = {tok[i]: int(tok[i + 1]) for i in range(0, len(tok), 2)}
    words = np.fromfile(dump, dtype="<u4") if dump else None
    return head, facts, words
