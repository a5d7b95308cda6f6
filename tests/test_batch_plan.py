"""The schedule of the host-pointer searches, on the CPU under the sanitizers.

tests/c/batch_plan_check.cpp is a stand-alone program with its own main: it includes csrc/batch_plan.h -- the non-empty batches of a run,
the upload groups and their byte ranges, the step of every batch (lane, tokens, successor, lookahead), the ingest tracker, the packed
result block and the split of a batch over devices -- restates the loops ivfadc_search_batches used to hold and compares the two over
stride 1 and 2, every batch count up to 60 and the counts around each change of the group width, ragged sizes with empty batches in
front, behind and between groups.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary child process:
nothing is preloaded, nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")


def test_schedule_tracker_blocks_and_split_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the batch plan check"
    exe = os.path.join(str(tmp_path), "batch_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "batch_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"batch_plan_check ok: (\d+) schedules, (\d+) groups, (\d+) steps, (\d+) tracker runs, (\d+) blocks, (\d+) splits", r.stdout)
    assert m, r.stdout[-2000:]
    got = [int(x) for x in m.groups()]
    counts = list(range(1, 61)) + [251, 252, 253, 503, 504, 505, 755, 756, 757, 2000, 65536]
    # 2 strides x 71 counts x 4 forms of ragged sizes, + the all-zero and the empty run per stride; a step per non-empty batch
    assert got[0] == 2 * len(counts) * 4 + 4 and got[2] == 2 * 4 * sum(counts)
    # (the program is deterministic: the groups of those schedules; 2^queries answer patterns for 1 .. 7 batches + 2 x 3 x 64 drawn ones)
    assert got[1] == 30340 and got[3] == 512 + 2 * 3 * 64
    # 5 rows x 4 K + the three products above 2^31; nq 0 .. 70 x G 1 .. 9
    assert got[4] == 5 * 4 + 3 and got[5] == 71 * 9


def test_header_is_plain_cpp_and_the_host_entries_stage_and_schedule_with_it():
    """batch_plan.h names no HIP type and no handle (it compiles with g++ above, under -Wall -Wextra -Werror); the host runtime takes the
    schedule, the result block and the device split from it instead of restating them, carves no result block by hand, and decides in
    one place whether a host array of queries is read where it lies or through pin_in."""
    hdr = open(os.path.join(CSRC, "batch_plan.h")).read()
    for word in ("hip/hip_runtime", "hipStream", "hipError", "hipEvent", "__global__", "__device__", "ivfadc_index", "PinnedBuf"):
        assert word not in hdr, word
    for fn in ("inline int non_empty_batches(", "inline Groups upload_groups(", "inline ByteRange group_bytes(", "inline Step step_of(", "struct IngestTracker {",
               "inline ResultBlock result_words(", "inline ResultBlock result_bytes(", "inline int64_t mg_lo("):
        assert hdr.count(fn) == 1, fn
    host = open(os.path.join(CSRC, "ivfadc_hip.hip")).read()
    assert '#include "batch_plan.h"' in host
    # the definitions that moved: the token numbering, the groups, the tracker's state, the device split
    for word in ("token_of", "group_of", "lane_done", "ev_seen", "int64_t mg_lo("):
        assert word not in host, word
    assert host.count("batch_plan::mg_lo(") == 8 and host.count("batch_plan::step_of(") == 1 and host.count("batch_plan::upload_groups(") == 1
    assert host.count("batch_plan::IngestTracker(") == 1 and host.count("batch_plan::group_bytes(") == 1
    # no result block is carved outside the header: pin_out, the two copy-outs and both sides of the multi-device gather
    for pat in ("+ 2 * idb", "+ idb", "2 * idb", "nql * K", "nql * (2 * "):
        assert pat not in host, pat
    assert host.count("batch_plan::result_bytes(") == 3 and host.count("batch_plan::result_words(") == 1
    assert host.count("static int stage_results(ivfadc_index *h, SearchCall &c)") == 1 and host.count("stage_results(h, ") == 2
    assert host.count("static void copy_out(") == 1 and host.count("copy_out(") == 4 and host.count("if (!h->hc_out_direct) copy_out(hc, h->pin_out.p, hc.nq);") == 2
    # known to the library? else pin_in: once, for ivfadc_search, ivfadc_search_batches (whole and group by group) and the RCCL branch of
    # ivfadc_mg_search
    assert host.count("pin_in.ensure(") == 1 and len(re.findall(r"host_known\(rows, bytes\)\) src = [^;]*;\s*if \(!src\) \{\s*TRY\(h->pin_in\.ensure\(bytes\)\);", host)) == 1
    assert host.count("static int stage_queries(") == 1 and host.count("TRY(stage_queries(h, ") == 4
    assert host.count("pin_out.ensure(") == 1 and host.count("memcpy(h->pin_in.p") == 0 and host.count("h->pin_in.p + off") == 1
    # the time buckets of ivfadc_host_stats: laps of one clock, in the blocking pair and in the run of batches
    assert host.count("struct HostClock") == 1 and host.count("hstats.stage_in_us +=") == 2 and host.count("hstats.stage_out_us +=") == 2
    # the run of batches in parts, the guard still there
    for part in ("static int setup_batch_lanes(", "struct BatchDrain {", "struct BatchRun {", "static int host_wait("):
        assert host.count(part) == 1, part
    assert "BatchDrain drain{h, lane2, true};" in host and "drain.armed = false;" in host
    for kept in ("profiles/r05_batches_stream_priorities.txt", "~6 us per search", "a third of the time a search takes"):
        assert host.count(kept) == 1, kept
