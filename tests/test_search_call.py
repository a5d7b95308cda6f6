"""The search call object and the shared sort-group loop, on the CPU under the sanitizers.

tests/c/search_call_check.cpp is a stand-alone program with its own main: it includes csrc/search_call.h -- the one struct that carries a
batch from the C entries to the kernel launches, and the one function that slices it -- lays host arrays out for small batches, takes
nested slices (sub-batch, sort group, grid-y block) at every (b0, n) and checks that every pointer lands on the element a flat index
computes, that null stays null, that slices compose and that whole_batch survives only the identity slice.  The same program restates
the loop search_generic used to cut its sort groups with and compares it with range_plan::next_group, which it calls now, over totals at
the edges.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary child process: nothing is preloaded,
nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")


def test_slices_and_sort_groups_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the search call check"
    exe = os.path.join(str(tmp_path), "search_call_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "search_call_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"search_call_check ok: (\d+) shapes, (\d+) slices, (\d+) group tables, (\d+) groups", r.stdout)
    assert m, r.stdout[-2000:]
    # 5 nq x 2 d x 2 K x 2 w x 2^7 combinations of optional rows; 3 caps x (32 tables + 4 lengths x 8)
    assert int(m.group(1)) == 5 * 2 * 2 * 2 * 128 and int(m.group(2)) > 1000000 and int(m.group(3)) == 3 * (32 + 4 * 8) and int(m.group(4)) > 65535


def test_header_is_plain_cpp_and_the_host_runtime_slices_with_it():
    """search_call.h names no HIP type (it compiles with g++ above, under -Wall -Wextra -Werror); the host runtime takes the struct and
    its slice from the header instead of restating them, fills a MaskView in one place, and advances no per-query pointer of a call by
    hand; the generic path cuts its sort groups with range_plan::next_group, through the helper the range search uses."""
    hdr = open(os.path.join(CSRC, "search_call.h")).read()
    for word in ("hip/hip_runtime", "hipStream", "hipError", "__global__", "__device__", "ivfadc_index"):
        assert word not in hdr, word
    assert hdr.count("SearchCall slice(int64_t b0, int64_t n) const") == 1 and hdr.count("ProbeRows slice(int64_t g0) const") == 1
    host = open(os.path.join(CSRC, "ivfadc_hip.hip")).read()
    mask = open(os.path.join(CSRC, "maskset.hip.h")).read()
    assert '#include "search_call.h"' in host and '#include "search_call.h"' in mask
    for word in ("struct SearchCall", "struct ProbeRows", "struct PreProbes", "struct MaskArgs", "SearchCall slice(", "ProbeRows slice("):
        assert word not in host, word
    for fn in ("search_dev", "search_subbatch", "probe_stage", "scan_query_major", "scan_list_major", "search_generic", "search_small", "coarse_dev"):
        assert re.search(r"^int %s\(ivfadc_index \*h, (const Plan &pl, )?const SearchCall &c[,)]" % fn, host, re.M), fn
    assert re.search(r"^int range_dev\(ivfadc_index \*h, const SearchCall &c, ", host, re.M)
    assert host.count(".slice(") >= 10
    # the one place a MaskView is filled, and the one launch that ingests mask numbers
    assert mask.count("inline MaskView mask_view(const SearchCall &c)") == 1
    assert "mv.words =" not in host and "mv.mask_of_query =" not in host
    assert host.count("hipLaunchKernelGGL(maskset_ingest_kernel") == 1
    # the advances that every sub-batch, stage-A batch, sort group and grid-y block used to spell out
    for pat in (r"d_q \+ ", r"d_ids \+ ", r"d_dists \+ ", r"d_counts \+ ", r"d_r \+ ", r"pre_list \+ ", r"pre_dc \+ ", r"mask_of_query \+ "):
        assert not re.search(pat, host), pat
    # one sort-group loop, one failure exit
    assert host.count("range_plan::next_group(") == 1 and host.count("for_sort_groups(h, ") == 2 and host.count("range_plan::sort_cap_keys(") == 1
    assert host.count("static int finish_entry(ivfadc_index *h, int rc)") == 1 and host.count("finish_entry(h, ") == 5
    # ... which the eight host and range entries reach through five bodies: ivfadc_search, ivfadc_search_preassigned, ivfadc_coarse_search,
    # the masked pair's and the four range entries'
    for body in ("search_masked_entry(", "range_entry("):
        assert host.count("static int " + body) == 1, body
    assert host.count("return range_entry(h, ") == 4 and host.count("return search_masked_entry(h, s, ") == 2
    assert host.count("const std::string msg = g_err;") == 3, "finish_entry, and the two multi-device drains of ivfadc_mg_search / ivfadc_comm_init"
