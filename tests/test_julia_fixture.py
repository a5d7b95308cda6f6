"""Cross-implementation pin: fixtures produced by the REAL IVFADC.jl (tools/julia/make_fixture.jl).

The build image has no julia, so the fixture files (tests/golden/julia_*.bin, *_queries.f32, *_knn.txt) cannot be
generated here; when somebody drops them in, these tests load the Julia-written index with the native reader
(ivfadc_load_index, src/persistency.jl:1-78) and require the reference's own knn_search output: ids exact, Float32
distances within 1e-4 relative.  Until then they skip -- and say why -- and the oracle stays "parity unpinned"
(DESIGN.md section 3).  The parser itself is tested on a synthetic file in the reference's output format."""
import glob
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def parse_knn(path):
    """-> {(w, q): (ids uint32[], dists float32[])} from the lines make_fixture.jl writes."""
    out = {}
    for ln in open(path):
        ln = ln.strip()
        if not ln or ln.startswith("#"):
            continue
        left, right = ln.split("|")
        f = left.split()
        w, q, cnt = int(f[0]), int(f[1]), int(f[2])
        ids = np.array([int(x) for x in f[3:3 + cnt]], np.uint32)
        dists = np.array([float(x.replace("f0", "").replace("f", "e")) for x in right.split()], np.float32)
        assert len(ids) == cnt and len(dists) == cnt
        out[(w, q)] = (ids, dists)
    return out


def test_parser_reads_the_generator_format(tmp_path):
    p = os.path.join(str(tmp_path), "julia_x_knn.txt")
    open(p, "w").write("# K=3 d=2 nq=2\n1 0 3 4 3 6 | 1.5f0 2.25f0 1.0f-5\n1 1 2 0 1 | 0.01f0 0.0121f0\n2 0 0  | \n")
    k = parse_knn(p)
    assert np.array_equal(k[(1, 0)][0], [4, 3, 6]) and np.allclose(k[(1, 0)][1], [1.5, 2.25, 1e-5])
    assert np.array_equal(k[(1, 1)][0], [0, 1]) and len(k[(2, 0)][0]) == 0


def _fixtures():
    return sorted(glob.glob(os.path.join(GOLD, "julia_*.bin")))


@pytest.mark.gpu
def test_julia_written_index_gives_julia_results(native):
    fx = _fixtures()
    if not fx:
        pytest.skip("no tests/golden/julia_*.bin: run tools/julia/make_fixture.jl with real IVFADC.jl to pin the oracle")
    from oracle import oracle as ora
    for binp in fx:
        base = binp[:-4]
        g = native.load_ivfadc_index(binp)
        qs = np.fromfile(base + "_queries.f32", np.float32).reshape(-1, g.d)
        knn = parse_knn(base + "_knn.txt")
        K = max(len(v[0]) for v in knn.values())
        off, codes, ids = g._lists()
        oidx = ora.OracleIndex(g._centroids, g._codebooks, g._labels, off, codes, ids)
        for w in sorted({k[0] for k in knn}):
            gi, gd, gc = g.search_raw(qs, K, w)
            oi, od, oc = oidx.knn_search(qs, K, w)
            for q in range(qs.shape[0]):
                ji, jd = knn[(w, q)]
                assert gc[q] == len(ji) == oc[q], (binp, w, q)
                # the HIP path and the oracle against what IVFADC.jl itself returned
                assert np.array_equal(gi[q, :gc[q]], ji) and np.array_equal(oi[q, :oc[q]], ji), (binp, w, q, gi[q], ji)
                # against IVFADC.jl itself, whose float order DESIGN.md declares unpinned: 1e-4 relative stays, no bit comparison
                assert np.allclose(gd[q, :gc[q]], jd, rtol=1e-4, atol=0) and np.allclose(od[q, :oc[q]], jd, rtol=1e-4, atol=0)
