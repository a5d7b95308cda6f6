"""The planner of ivfadc_score_ids and the kernel's pair and row addressing, on the CPU under the sanitizers.

tests/c/score_plan_check.cpp is a stand-alone program with its own main: it includes csrc/score_plan.h -- the two stride forms, the query
slices under a workspace limit, the pair arithmetic in 64 bits, the tile shape, the grid -- restates the host entry's loop over the slices
and score_pairs_kernel of csrc/score.hip.h lane by lane in plain C++ on top of it, and runs them over C = 1 / 63 / 64 / 65 / 255 / 256 /
257, nq = 1 / 3 / 1000, both strides, no counts, ragged counts (zero included) and counts outside [0, C], workspace limits that cut
between and exactly at query boundaries, and pair counts on both sides of 2^31 - 1.  Every pair must be written exactly once, nothing
outside the rows may be read or written (every array has exactly the caller's size: a wrong index is an AddressSanitizer report), and the
gathered distance must be the plain triple loop's.
Built with AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary child process: nothing is preloaded, nothing is loaded
into Python."""
import os
import re
import shutil
import subprocess

import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")


def test_planner_and_kernel_arithmetic_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the score planner check"
    exe = os.path.join(str(tmp_path), "score_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           "-ffp-contract=off", os.path.join(ROOT, "tests", "c", "score_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"score_plan_check ok: (\d+) simulated calls over (\d+) shapes, (\d+) pairs written once, (\d+) scored, (\d+) slices, (\d+) plan cases",
                  r.stdout)
    assert m, r.stdout[-2000:]
    calls, shapes, pairs, scored, slices, plans = (int(x) for x in m.groups())
    assert calls >= 7 * 3 * 2 * 3 and shapes >= 8 and pairs > 1000000 and scored > pairs // 4 and slices > 2 * calls and plans > 200


def test_case_sizes_are_the_programs():
    src = open(os.path.join(ROOT, "tests", "c", "score_plan_check.cpp")).read()
    m = re.search(r"CASE_C\[\] = \{([^}]*)\}", src)
    sizes = tuple(int(x) for x in m.group(1).split(","))
    assert sizes == (1, 63, 64, 65, 255, 256, 257) and set(sr.EDGE_C) <= set(sizes)
    assert re.search(r"CASE_NQ\[\] = \{1, 3, 1000\}", src)
    for word in ("MAX_PAIRS + 1", "{46341, 46341}", "{46340, 46341}", "exact - 1, exact, exact + 1"):
        assert word in src, word


def test_plan_header_is_plain_cpp_and_shared_with_the_kernel():
    """score_plan.h names no HIP type (it compiles with g++ above) and marks its constants as reasoned, not measured; score.hip.h and the
    host runtime take the arithmetic and the plan from it instead of restating them; the kernel holds no inline assembly, reads the
    stored code and the codeword as recon_decode_kernel does, and the locate pass is the existing one, called and not copied."""
    plan = open(os.path.join(CSRC, "score_plan.h")).read()
    for word in ("hip/hip_runtime", "hipStream", "__global__", "dim3"):
        assert word not in plan, word
    assert "REASONED, NOT MEASURED" in plan and plan.count("REASONED") >= 3
    kern = open(os.path.join(CSRC, "score.hip.h")).read()
    body = kern.split("#pragma once")[1]
    assert '#include "score_plan.h"' in kern and '#include "reconstruct.hip.h"' in kern
    for cite in ("coarsequantizers.jl:33-34", "coarsequantizers.jl:40-45", "index.jl:232-236", "index.jl:242-246", "utils.jl:49-55"):
        assert cite in kern, cite
    for shared in ("score::TILE", "score::tile_slot(", "score::pair_index(", "score::loc_index(", "score::live_slots(", "score::query_row(",
                   "score::centre_vec4(", "score::codeword_vec4(", "recon::code_row(", "recon::codeword_elem(", "recon::label_slot("):
        assert shared in body, shared
    assert "asm" not in body and "fmaf" not in body and "__fmaf" not in body
    assert body.count("__global__") == 1 and "template" not in body, "written once for both code widths"
    assert "extern __shared__" in body and not re.search(r"^\s*__shared__", body, re.M), "the query is dynamic LDS"
    host = open(os.path.join(CSRC, "ivfadc_hip.hip")).read()
    entry = host[host.index("static int score_enqueue("):host.index("int ivfadc_score_ids(")]
    for shared in ("score::make_plan(", "score::slice_begin(", "score::slice_queries(", "score::id_index(", "score::TILE", "locate_device("):
        assert shared in entry, shared
    assert "h2d_copy" not in entry and "d2h_copy" not in entry and "hipStreamSynchronize" not in entry and "hipMemcpy" not in entry, \
        "what the device entry runs through only enqueues"
    assert host.count("recon_locate_kernel<") == 2 and host.count("static int locate_sorted(") == 1, "the locate pass is not copied"
    from ivfadc_jl_amd import _native as nat
    assert "-ffp-contract=off" in nat.HIPCC_FLAGS and any(s.endswith("score.hip.h") for s in nat.SOURCES) and any(
        s.endswith("score_plan.h") for s in nat.SOURCES)
