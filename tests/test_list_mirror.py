"""The host mirror of the inverted lists, its edits, the device layout's arithmetic and the label map, on the CPU under the sanitizers.

tests/c/list_mirror_check.cpp is a stand-alone program with its own main: it includes csrc/list_mirror.h -- everything the write side of
the host runtime does to the mirror -- and drives seeded random chains of assign / append / erase / shift / layout against a naive model
(one flat vector of (list, id, code row) in insertion order), comparing the full gathered state after every step; the in-place decision
and the destination pairs of an append are checked against the model's own layout, the 2^32 refusals on lengths alone, and the label map
on identity, permuted and sparse labels with the first offender reported.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and
run as an ordinary child process: nothing is preloaded, nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")


def test_mirror_edits_against_the_naive_model_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the list mirror check"
    exe = os.path.join(str(tmp_path), "list_mirror_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "list_mirror_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"list_mirror_check ok: (\d+) shapes, (\d+) steps, (\d+) appends, (\d+) in place, (\d+) erases, (\d+) ids erased, "
                  r"(\d+) layouts, (\d+) limit cases, (\d+) label maps, (\d+) offenders", r.stdout)
    assert m, r.stdout[-2000:]
    shapes, steps, appends, inplace, erases, erased, layouts, limits, maps, offenders = (int(x) for x in m.groups())
    # 3 kc x 4 cb; per shape 6 rounds of 5 fixed appends (0, 1 and a capacity-filling 3 points in place; one on a stale layout and one
    # a point past a capacity never in place), 3 fixed layouts, 2 fixed erases and 30 random steps
    assert shapes == 12 and appends >= 12 * 6 * 5 and 12 * 6 * 3 <= inplace <= appends - 12 * 6 * 2
    assert erases >= 12 * 6 * 2 and erased >= 1000 and layouts >= 12 * (1 + 6 * 3) and steps >= appends + erases
    # 6 layouts x 3 strides + 7 offset and capacity cases; 2 ksub x 3 kinds of 16-bit maps + 2 8-bit maps; 3 positions for each map
    # that can hold a non-label
    assert limits == 6 * 3 + 7 and maps == 8 and offenders == (6 + 1) * 3


def test_header_is_plain_cpp_and_the_host_runtime_edits_the_mirror_through_it():
    """list_mirror.h names no HIP symbol (it compiles with g++ above, under -Wall -Wextra -Werror); the host runtime includes it,
    touches no list of the mirror by hand, keeps the staleness protocol in one guard type, and reaches every width pair through one body."""
    hdr = open(os.path.join(CSRC, "list_mirror.h")).read()
    for word in ("hip/hip_runtime", "hipStream", "hipError", "hipMemcpy", "__global__", "__device__", "ivfadc_index", "g_err", "DevBuf"):
        assert word not in hdr, word
    host = open(os.path.join(CSRC, "ivfadc_hip.hip")).read()
    assert '#include "list_mirror.h"' in host
    assert "hl_codes[" not in host and "hl_ids[" not in host
    for word in ("struct HostMirror", "sort_labels16", "find_label16", "labels_to_indices", "indices_to_labels", "h_label_ok", "set_lists_mirror"):
        assert word not in host, word
    # one guard type: the only place that remembers whether the copy was stale, and the only writes of the flag besides the three
    # places that have no mirror data to fall back on (a new index, synthetic lists, a subset view)
    assert host.count("struct StaleGuard {") == 1 and host.count("const bool was_dirty;") == 1
    assert len(re.findall(r"\bwas_dirty\b", host)) == 3, "its declaration, its initialiser, in_place()"
    assert len(re.findall(r"->dirty = (true|false);", host)) == 5, "the guard's two; ivfadc_create, ivfadc_synth_lists, fill_subset_lists: no mirror data"
    assert host.count("StaleGuard stale(h);") == 5, "upload_lists, assign_lists, append_encoded, delete_ids, shift_ids"
    # one body per entry pair
    for body, calls in (("set_lists_entry(", 3), ("get_lists_entry(", 2), ("encode_entry(", 2), ("append_entry(", 2), ("get_quantizers_entry(", 2)):
        assert host.count("static int " + body) == 1, body
        assert host.count("return " + body) + host.count(": " + body) == calls, body
    assert host.count("append_encoded(h, nnew, lst.data(), cod.data(), ids)") == 2, "append_entry, and ivfadc_mg_append once per replica"
    # the delete entry finds before it opens the scope, and commits only inside it
    body = host[host.index("int ivfadc_delete_ids("):host.index("int ivfadc_shift_ids(")]
    assert body.index("mirror.find_ids(") < body.index("ms.begin(") < body.index("StaleGuard stale(h);") < body.index("mirror.erase_ids(")
