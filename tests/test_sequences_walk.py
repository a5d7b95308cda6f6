"""CPU checks of tests/sequences.py: the walk of the pair tests takes every ordered pair of forms exactly once and closes, and the default
seed of the sequence fuzz is steered well enough -- judged on the draws and the restated plan rules alone, never on the library."""
import pytest

import sequences as sq


@pytest.mark.parametrize("n", [1, 2, 5, 16])
def test_transition_walk_takes_every_ordered_pair_once_and_closes(n):
    walk = sq.transition_walk(n)
    assert len(walk) == n * n + 1 and walk[0] == walk[-1]
    assert all(0 <= v < n for v in walk)
    pairs = list(zip(walk[:-1], walk[1:]))
    assert len(set(pairs)) == n * n and set(pairs) == {(a, b) for a in range(n) for b in range(n)}


def test_default_seed_reaches_every_on_request_form_behind_another():
    """Every on-request form is specified at least three times by the default seed's draws, and at least once directly behind a
    DIFFERENT on-request form on the same handle."""
    rows = sq.specified_forms()
    assert len(rows) == sq.FUZZ_HANDLES and all(len(r) == sq.FUZZ_STEPS for r in rows)
    count = {f: 0 for f in sq.ON_REQUEST}
    behind = {f: set() for f in sq.ON_REQUEST}
    for row in rows:
        for i, f in enumerate(row):
            if f is None:
                continue
            count[f] += 1
            if i > 0 and row[i - 1] is not None and row[i - 1] != f:
                behind[f].add(row[i - 1])
    assert all(count[f] >= 3 for f in sq.ON_REQUEST), count
    assert all(behind[f] for f in sq.ON_REQUEST), behind


def test_default_seed_runs_every_on_request_form_in_several_sub_batches():
    """The workspace limit has a floor of 1 MiB and the sub-batch one of 64 queries, so a small limit alone splits only heavy searches:
    the draws make steered steps heavy (draw_step), and every on-request form gets at least one step whose sub-batch is certainly
    smaller than its batch -- the probe histogram, the work-queue head and the per-query bounds are then re-armed INSIDE one search."""
    sub = sq.sub_batched_forms()
    assert all(sub.get(f, 0) >= 1 for f in sq.ON_REQUEST), sub


def test_sub_batch_upper_bound_examples():
    shape = dict(m=8, dsub=16, ksub=256, kc=14, n=30000, u16=False)
    st = dict(K=64, w=8, chunk=1024, ws=sq.WS_SMALL, nq=130)
    # lists of >= 2 139 points: three chunks; per_q = 56 + 8 * 3 * 516 + 160 + 512 + 64 = 13 176 B -> 79 queries per sub-batch
    assert sq.sub_batch_upper_bound(shape, st) == 79
    assert sq.sub_batch_upper_bound(shape, dict(st, K=128)) == 64                  # the floor
    assert sq.sub_batch_upper_bound(shape, dict(st, ws=sq.WS_DEFAULT)) > 257
    assert sq.sub_batch_upper_bound(dict(shape, kc=3), dict(st, w=70)) == 65       # w is clamped to kc = 3; ten chunks


def test_expected_form_examples():
    """The restated rules, worked by hand from make_plan / make_plan_u16: tuning 4 with table modes 6 .. 9 at m = 8 and m = 16 with K
    inside and beyond each pool, the narrow-field and small-batch requests, the plan's own eight-wave choice on lists of 10 000 points,
    shapes without the kernels, a list partition, and UInt16 handles below and above K = 64 with the LDS rule of table mode 10."""
    m8 = dict(m=8, dsub=16, ksub=256, kc=14, n=30000, u16=False)
    m16 = dict(m=16, dsub=8, ksub=256, kc=14, n=30000, u16=False)
    u16 = dict(m=4, dsub=8, ksub=1024, kc=4, n=40000, u16=True)

    def s(table, qg, **kw):
        return dict(table=table, qg=qg, chunk=0, prune=1, **kw)
    assert sq.expected_form(m8, s(6, 4), 10, 3, 61) == {"last_qg": 4, "last_striped": 2, "last_nf": 0}
    assert sq.expected_form(m8, s(7, 4), 64, 3, 61)["last_striped"] == 3
    assert sq.expected_form(m8, s(8, 4), 100, 3, 61) == {"last_qg": 4, "last_striped": 4, "last_nf": 0}
    assert sq.expected_form(m8, s(9, 4), 128, 3, 61) == {"last_qg": 8, "last_striped": 5, "last_nf": 0}
    assert sq.expected_form(m8, s(9, 4), 129, 3, 61)["last_striped"] == 1            # beyond the wide pool: the four-wave kernel
    assert sq.expected_form(m8, s(6, 4), 100, 3, 61)["last_striped"] == 1
    assert sq.expected_form(m8, s(0, 8), 10, 3, 61) == {"last_qg": 8, "last_nf": 1}
    assert sq.expected_form(m8, s(0, 4), 10, 3, 61)["last_striped"] == 1            # lists of 2 100 points: not the plan's own choice
    assert sq.expected_form(dict(m8, kc=3), s(0, 4), 10, 3, 61)["last_striped"] == 2  # lists of 10 000 points: it is
    assert sq.expected_form(dict(m8, kc=3), s(5, 4), 10, 3, 61)["last_striped"] == 1
    assert sq.expected_form(m8, s(0, 0), 10, 3, 9) == {"last_qg": -3}
    assert sq.expected_form(m8, s(0, 0), 10, 3, 257) is None
    assert sq.expected_form(m8, s(3, -1), 10, 3, 61) == {"last_qg": 0}
    assert sq.expected_form(m8, s(0, 4), 2500, 3, 8) == {"last_qg": -2}
    assert sq.expected_form(m8, s(6, 4, part_n=2), 10, 3, 61)["last_striped"] == 2
    assert sq.expected_form(dict(m8, ksub=255), s(6, 4), 10, 3, 61)["last_striped"] == 0
    assert sq.expected_form(m16, s(6, 4), 64, 3, 61)["last_striped"] == 2
    assert sq.expected_form(m16, s(9, 4), 10, 3, 61) == {"last_qg": 8, "last_striped": 3, "last_nf": 0}
    assert sq.expected_form(m16, s(0, 4), 10, 3, 61)["last_striped"] == 1            # m = 16 runs the kernel on request only
    e = sq.expected_form(m16, s(8, 4), 65, 3, 61)
    assert e == sq.expected_form(m16, s(6, 4), 65, 3, 61) and e["last_qg"] == 4 and e["last_striped"] == 1
    assert sq.expected_form(dict(m16, dsub=6), s(6, 4), 10, 3, 61)["last_striped"] == 1
    assert sq.expected_form(u16, s(0, 2), 64, 3, 96) == {"last_qg": 2, "last_scan_lds": 33936, "last_striped": 0}
    assert sq.expected_form(u16, s(0, 0), 10, 3, 96)["last_qg"] == 8
    assert sq.expected_form(u16, s(0, 8), 100, 3, 96) == {"last_qg": -2}
    assert sq.expected_form(u16, s(10, 8), 65, 3, 96) == {"last_qg": 8, "last_scan_lds": 33936 + 4 * 8 * 256 * 8, "last_striped": 0}   # cap 256
    assert sq.expected_form(u16, s(10, 8), 192, 3, 96)["last_qg"] == 8             # cap 256
    assert sq.expected_form(u16, s(10, 8), 193, 3, 96)["last_qg"] == 4             # cap 512: 162 KB at eight pairs
    assert sq.expected_form(u16, s(10, 0), 1000, 3, 96)["last_qg"] == 1            # cap 2048
    assert sq.expected_form(u16, s(10, 0), 2500, 3, 96) == {"last_qg": -2}
    assert sq.expected_form(dict(u16, m=1, dsub=8), s(10, 1), 1985, 2, 12) == {"last_qg": -2}     # cap 4096 does not fit
