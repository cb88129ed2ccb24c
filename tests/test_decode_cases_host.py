"""tests/decode_cases.py without a GPU: the cases of tests/test_gpu_decode_edges.py reach the paths of
rocco_amd/csrc/decode.hip they are meant to reach (scan trips, run starts and ends on every boundary kind, full lanes,
odd and even tables, every stride count of the to-host kernel), their expected runs agree with the oracle's per-locus
loop (rocco/rocco.py:180-190) and bytes other than 1 change nothing."""
import numpy as np
import pytest

import decode_cases as dc


@pytest.fixture(scope="module")
def built():
    """name -> (n, z, begins, ends, census)"""
    out = {}
    for name, n, builder in dc.cases():
        z = builder()
        b, e = dc.expected_runs(z)
        out[name] = (n, z, b, e, dc.census(z, b, e))
    return out


def test_builders_are_named_once_sized_and_deterministic(built):
    listed = dc.cases()
    assert len({name for name, _n, _b in listed}) == len(listed)
    for name, n, builder in listed:
        z = builder()
        assert z.dtype == np.uint8 and z.shape == (n,), name
        if n <= 70000:
            assert np.array_equal(z, builder()), name
    for name in ("sparse@%d" % dc.N_TWO_TRIPS, "rand@8194#mix"):
        n, z = built[name][:2]
        assert np.array_equal(z, dict((c[0], c[2]) for c in listed)[name]()), name


def test_every_size_the_kernels_change_path_at_is_present(built):
    sizes = {v[0] for v in built.values()}
    want = {2, 3, dc.TRIP, dc.TRIP + 1, 2 * dc.TRIP + dc.TILE + 1}
    for base in (16, 4096):
        for k in (1, 2):
            want |= {base * k + d for d in (-2, -1, 0, 1, 2)}
    assert want <= sizes
    for n in want:
        for pattern in ("ones",) + (("zeros", "alt10", "alt01", "rand") if n < dc.TRIP else ()):
            assert f"{pattern}@{n}" in built
    assert {f"alt10@{dc.DENSE_N}", f"alt01@{dc.DENSE_N}"} <= set(built)
    for n in dc.PLACED_SIZES:
        for p in (0, 15, 16, 1023, 1024, 4095, 4096, n - 2, n - 1):
            assert f"single[{p}]@{n}" in built
        for p in (0, 15, 1023, 4095, n - 2):
            assert f"pair[{p},{p + 1}]@{n}" in built
        assert f"run[n-3,n)@{n}" in built


def test_census_reaches_every_path(built):
    cen = {name: v[4] for name, v in built.items()}
    assert {c["trips"] for c in cen.values()} == {1, 2, 3}
    for kind in dc.BOUNDARIES:
        seen = set().union(*(c["boundaries"][kind] for c in cen.values()))
        assert seen == {"start", "end", "cross"}, kind
    # in the multi-trip vectors themselves: runs behind the first trip, so that a lost carry moves them
    for name in (f"sparse-cross@{dc.N_THREE_TRIPS}", f"sparse-touch@{dc.N_THREE_TRIPS}"):
        b = built[name][2]
        assert np.any((b >= dc.TRIP) & (b < 2 * dc.TRIP)) and np.any(b >= 2 * dc.TRIP), name
    assert cen[f"sparse-cross@{dc.N_THREE_TRIPS}"]["boundaries"]["trip"] == {"cross"}
    assert cen[f"sparse-touch@{dc.N_THREE_TRIPS}"]["boundaries"]["trip"] == {"start", "end"}
    assert cen[f"sparse@{dc.N_TWO_TRIPS}"]["boundaries"]["trip"] == {"end"}
    assert max(c["max_starts_in_lane"] for c in cen.values()) == 8 == dc.LANE // 2
    assert cen[f"alt10@{dc.DENSE_N}"]["rows"] == cen[f"alt01@{dc.DENSE_N}"]["rows"] == 200000
    assert any(c["odd_rows"] for c in cen.values()) and any(not c["odd_rows"] and c["rows"] for c in cen.values())
    assert any(43691 <= c["rows"] <= 87381 for c in cen.values()) and any(c["rows"] >= 87382 for c in cen.values())
    assert dc.host_copy_strides(43690) == 1 and dc.host_copy_strides(43691) == 2
    assert dc.host_copy_strides(87381) == 2 and dc.host_copy_strides(87382) == 3
    # only locus n-1 set: a non-zero vector without a run
    for n in dc.PLACED_SIZES:
        c = cen[f"single[{n - 1}]@{n}"]
        assert c["nonzero"] and c["rows"] == 0
    # ones: one run [0, n-1) whatever the length;  [n-3, n) ends at n-1
    for name, (n, _z, b, e, _c) in built.items():
        if name.startswith("ones@"):
            assert (b.tolist(), e.tolist()) == ([0], [n - 1]), name
        if name.startswith("run[n-3,n)@") and "#" not in name:
            assert (b.tolist(), e.tolist()) == ([n - 3], [n - 1]), name
    # the large tables stay small: no dense pattern at the multi-trip sizes except the single run
    for name, (n, _z, b, _e, _c) in built.items():
        if n >= dc.TRIP:
            assert b.size <= n // 400, name


def test_calls_pack_the_cases_as_the_gpu_test_needs(built):
    calls = dc.batches()
    assert sorted(c[0] for call in calls for c in call) == sorted(built)
    totals = []
    for call in calls:
        assert 1 <= len(call) <= dc.BATCH_MAX
        assert call[0][1] < dc.TRIP  # a multi-trip case never has tile_begin == 0
        totals.append(sum(built[name][4]["rows"] for name, _n, _b in call))
    multi = [c for call in calls for c in call if dc.scan_trips(c[1]) > 1]
    assert len(multi) >= 2
    strides = {dc.host_copy_strides(t) for t in totals}
    assert {1, 2} <= strides and max(strides) >= 3, totals
    assert any(t & 1 for t in totals) and any(t and not t & 1 for t in totals), totals


def test_diff_statement_agrees_with_the_oracle_loop(built, oracle):
    checked = 0
    for name, (n, z, b, e, _c) in built.items():
        if n > 70000:
            continue
        recs = oracle.chrom_solution_records("c", np.arange(n, dtype=np.int64), z)
        assert [(s, t) for _c2, s, t in recs] == list(zip(b.tolist(), e.tolist())), name
        checked += 1
    assert checked >= 100


def test_byte_values_do_not_change_the_runs(built):
    variants = [name for name in built if dc.original_of(name)]
    assert len(variants) == 3 * len(dc.BYTE_VALUES) + 1
    seen_values = set()
    for name in variants:
        n, z, b, e, _c = built[name]
        n0, z0, b0, e0, _c0 = built[dc.original_of(name)]
        assert n == n0 and np.array_equal(z != 0, z0 != 0) and not np.array_equal(z, z0), name
        assert np.array_equal(b, b0) and np.array_equal(e, e0) and b.size > 0, name
        seen_values |= set(np.unique(z).tolist())
    assert {0, 2, 0x80, 0xFF} <= seen_values
    assert len(set(np.unique(built["rand@8194#mix"][1]).tolist()) - {0}) >= 4
