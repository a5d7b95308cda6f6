"""The planner of ivfadc_locate / ivfadc_reconstruct and both kernels' index arithmetic, on the CPU under the sanitizers.

tests/c/reconstruct_plan_check.cpp is a stand-alone program with its own main: it includes csrc/reconstruct_plan.h -- work items from the
chunk prefix (built by one workgroup on the device), the hashed filter, the exact bitmap, the key of a hit, the decode's gather -- restates recon_locate_kernel and
recon_decode_kernel of csrc/reconstruct.hip.h lane by lane in plain C++ on top of it, and runs them over the case table's list lengths
(with stale ids behind every list's end), wanted-set sizes on both sides of the LDS filter's cap, spans on both sides of the bitmap's
bound and the whole id space, and SIFT1B-sized counts.
Built with AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary child process: nothing is preloaded, nothing is loaded
into Python."""
import os
import re
import shutil
import subprocess

import reconstruct_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")


def test_planner_and_kernel_arithmetic_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the reconstruct planner check"
    exe = os.path.join(str(tmp_path), "reconstruct_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "reconstruct_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"reconstruct_plan_check ok: (\d+) simulated locates over (\d+) lengths, (\d+) ids read, (\d+) plan cases, (\d+) decode shapes",
                  r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) >= 100 and int(m.group(2)) >= len(rr.CASE_LENS) and int(m.group(3)) > 100000 and int(m.group(4)) > 100
    assert int(m.group(5)) >= 16


def test_case_table_lengths_and_constants_are_the_programs():
    src = open(os.path.join(ROOT, "tests", "c", "reconstruct_plan_check.cpp")).read()
    m = re.search(r"CASE_LENS\[\] = \{([^}]*)\}", src)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == rr.CASE_LENS
    for n in rr.EDGE_LENS:
        assert n in rr.CASE_LENS
    for size in rr.REQUEST_SIZES:
        assert re.search(r"sizes\[\] = \{[^}]*\b%d\b" % size, src), size
    for word in ("FILTER_MAX_WANTED - 1, FILTER_MAX_WANTED, FILTER_MAX_WANTED + 1", "BITMAP_MAX_BITS - 1", "(uint32_t)BITMAP_MAX_BITS", "163840"):
        assert word in src, word


def test_plan_header_is_plain_cpp_and_shared_with_the_kernels():
    """reconstruct_plan.h names no HIP type (it compiles with g++ above) and marks its constants as reasoned, not measured;
    reconstruct.hip.h and the host runtime take the arithmetic and the plan from it instead of restating them; the kernels hold no inline
    assembly and resolve a hit with one 64-bit atomic maximum."""
    plan = open(os.path.join(CSRC, "reconstruct_plan.h")).read()
    for word in ("hip/hip_runtime", "hipStream", "__global__"):
        assert word not in plan, word
    assert "REASONED, NOT MEASURED" in plan and plan.count("REASONED") >= 4
    kern = open(os.path.join(CSRC, "reconstruct.hip.h")).read()
    body = kern.split("#pragma once")[1]
    assert '#include "reconstruct_plan.h"' in kern and "utils.jl:49-55" in kern
    for shared in ("recon::item_list(", "subset::subset_point(", "recon::filter_hash(", "recon::bitmap_covers(", "recon::slot_of(",
                   "recon::span_of(", "recon::prefix_begin(", "recon::list_chunks(", "recon::hit_key(", "recon::key_list(", "recon::key_pos(", "recon::code_row(", "recon::decode_block(", "recon::codeword_elem(",
                   "recon::label_slot("):
        assert shared in body, shared
    assert "asm" not in body and body.count("atomicMax(") == 1
    assert "p < (int64_t)len" in body and "p >= (int64_t)len" in body, "nothing at or behind list_len is read as an entry"
    host = open(os.path.join(CSRC, "ivfadc_hip.hip")).read()
    entries = host[host.index("static int locate_sorted("):host.index("static int locate_host(")]
    assert "h2d_copy" not in entries and "hipStreamSynchronize" not in entries, "what the device entries run through only enqueues"
    for shared in ("recon::make_plan(", "recon::list_chunks(", "recon_chunk_prefix_kernel", "pack::label_inverse("):
        assert shared in host, shared
    pack = open(os.path.join(CSRC, "pack_operands.h")).read()
    assert "label_inverse" in pack
