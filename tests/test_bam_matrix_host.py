"""Without a GPU: the host side of the one-pass chromosome matrix -- the merge of the tracks'
supports into segments against NumPy's union, the four new entry points as the header declares them, the shape the
kernels are built to, the size of the second-turn case, the two stubs that must stay as they are, and the fixture file."""
import ctypes
import os
import re

import numpy as np
import pytest

import bam_matrix_cases as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rocco_hip_alignment_chrom_range_batch", "rocco_hip_track_supports", "rocco_hip_track_matrix_fill",
               "rocco_hip_track_matrix_shape")
C_TYPES = {"rocco_hip_solver *": ctypes.c_void_p, "const int32_t *": ctypes.c_void_p, "const uint16_t *": ctypes.c_void_p,
           "const uint8_t *": ctypes.c_void_p, "const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "void *": ctypes.c_void_p,
           "const rocco_hip_count_options *": ctypes.c_void_p, "const rocco_hip_count_region *": ctypes.c_void_p,
           "const int64_t *": None, "int64_t *": None, "const double *": ctypes.POINTER(ctypes.c_double), "int *": ctypes.POINTER(ctypes.c_int),
           "size_t": ctypes.c_size_t, "int64_t": ctypes.c_longlong, "int": ctypes.c_int, "double": ctypes.c_double}


def header_text() -> str:
    with open(os.path.join(ROOT, "include", "rocco_hip.h"), encoding="utf-8") as handle:
        return handle.read()


def test_merge_of_supports_is_numpys_union():
    """A few hundred seeded support sets with touching, nested, identical and disjoint members: the columns of the segment
    table, end to end, are np.unique(np.concatenate(aranges)); segments are disjoint, ascending and never touch."""
    from rocco_amd import readtracks as rt

    rng = np.random.default_rng(20262)
    seen_gap = seen_touch = 0
    for _ in range(400):
        firsts, lasts = mx.seeded_supports(rng)
        seg_grid, seg_col, m = rt._merge_supports(firsts, lasts)
        want = mx.union_of_supports(firsts, lasts)
        assert m == want.size and seg_col[0] == 0 and seg_grid.size <= firsts.size
        assert np.array_equal(mx.columns_of_segments(seg_grid, seg_col, m), want)
        seg_last = seg_grid + np.diff(np.append(seg_col, m)) - 1
        assert np.all(seg_grid[1:] > seg_last[:-1] + 1), "two segments touch or overlap: they are one"
        starts = rt._segment_starts(seg_grid, seg_col, m, 50)
        assert starts.dtype == np.asarray([0]).astype(int).dtype and np.array_equal(starts, want * 50)
        seen_gap += seg_grid.size > 1
        seen_touch += any(a == b + 1 for a in firsts for b in lasts)
    assert seen_gap > 50 and seen_touch > 50
    # by hand: touching merges, a gap of one bin does not
    seg_grid, seg_col, m = rt._merge_supports([10, 21, 40, 31], [20, 30, 50, 38])
    assert seg_grid.tolist() == [10, 40] and seg_col.tolist() == [0, 29] and m == 40
    seg_grid, seg_col, m = rt._merge_supports([5], [5])
    assert (seg_grid.tolist(), seg_col.tolist(), m) == ([5], [0], 1)
    with pytest.raises(ValueError):
        rt._merge_supports([], [])


def test_new_entry_points_are_bound_with_the_headers_prototypes():
    from rocco_amd import _native

    text = header_text()
    bound = {p[0]: p for p in _native.PROTOTYPES}
    for name in NEW_SYMBOLS:
        declared = re.search(r"^(int|void) " + name + r"\(([^;]*)\);", text, re.M | re.S)
        assert declared, f"{name} is not declared in include/rocco_hip.h"
        assert name in bound, f"{name} has no ctypes prototype"
        _, restype, argtypes = bound[name]
        assert restype is (ctypes.c_int if declared.group(1) == "int" else None)
        params = [re.sub(r"\s+", " ", p).strip() for p in declared.group(2).split(",")]
        assert len(params) == len(argtypes), name
        for param, argtype in zip(params, argtypes):
            ctype, pname = re.match(r"(.*?[ *])(\w+)$", param).groups()
            ctype = ctype.strip()
            assert ctype in C_TYPES, (name, param)
            if ctype.endswith("*") and (pname.endswith("_dev") or C_TYPES[ctype] is ctypes.c_void_p):
                assert argtype is ctypes.c_void_p, (name, param, argtype)  # (a device array, a handle, a stream, a struct array)
            elif ctype.endswith("*"):  # a host array the call reads or fills: a typed pointer
                pointee = {"int64_t": ctypes.c_longlong, "double": ctypes.c_double, "int": ctypes.c_int}[ctype.replace("const ", "").rstrip(" *")]
                assert argtype._type_ is pointee, (name, param, argtype)
            else:
                assert argtype is C_TYPES[ctype], (name, param, argtype)
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)


def test_track_matrix_shape_is_the_headers():
    from rocco_amd import _native
    from rocco_amd import readtracks as rt

    text = header_text()
    defines = {name: int(value) for name, value in re.findall(r"#define (ROCCO_TRACK_MATRIX_\w+) (\d+)", text)}
    shape = rt.track_matrix_shape()
    assert shape == {"threads": defines["ROCCO_TRACK_MATRIX_THREADS"], "unit": defines["ROCCO_TRACK_MATRIX_UNIT"],
                     "max_grid": defines["ROCCO_TRACK_MATRIX_MAX_GRID"], "row_words": defines["ROCCO_TRACK_MATRIX_ROW_WORDS"]}
    assert shape["threads"] % 64 == 0 and shape["unit"] % shape["threads"] == 0
    # the launch caps were not extended for it
    assert int(re.search(r"#define ROCCO_LAUNCH_CAPS (\d+)", text).group(1)) == len(_native.LAUNCH_CAP_NAMES) == 16
    # the second-turn case of the GPU tests is one: K = 3 rows over one contig sized from the caps
    m = mx.second_turn_columns(shape)
    assert 3 * m > shape["unit"] * shape["max_grid"] and m * mx.STEP < 2 ** 31


def test_the_two_stubs_still_raise_their_messages():
    from rocco_amd import readtracks, rocco

    with pytest.raises(RuntimeError, match=r"rocco_amd does not decode BAM files: replace rocco_amd\.readtracks\.get_bam_chrom_reads with the "
                                           r"reference's reader \(asked for x\.bam\)"):
        readtracks.get_bam_chrom_reads("x.bam", "chrA", "t.sizes", 50)
    with pytest.raises(RuntimeError, match=r"rocco_amd does not decode BAM / bigWig files: pass \{chromosome: \(intervals, matrix\)\} or "
                                           r"replace rocco_amd\.rocco\.generate_chrom_matrix with the reference's reader"):
        rocco.generate_chrom_matrix("chrA", ["x.bam"], "t.sizes", 50)
    assert rocco.generate_chrom_matrix("chrA", {"chrB": (1, 2)}) == (None, None)


def test_fixture_holds_the_scenarios_the_gpu_tests_rely_on():
    arrays, meta = mx.golden()
    by_name = {e["name"]: e for e in meta["scenarios"]}
    assert np.unique(np.diff(arrays["gap_intervals"])).size > 1
    assert np.unique(np.diff(arrays["touch_intervals"])).size == 1 and arrays["touch_matrix"].shape[0] == 2
    assert by_name["all_excluded"]["none"] and by_name["not_in_header"]["none"]
    assert by_name["small_files"]["error"] == "failed to estimate read length"  # (the reference's own end for a file without placed reads)
    assert arrays["single_file_matrix"].shape[0] == 1
    assert arrays["low_memory_odd_matrix"].dtype == np.float32 and arrays["low_memory_odd_matrix"].shape[1] % 2 == 1
    for option, value in (("center_reads", True), ("scale_by_step", True), ("const_scale", 2.0), ("round_digits", 3), ("low_memory", True),
                          ("flag_include", 16), ("min_mapping_score", 0)):
        assert any(e["kwargs"].get(option) == value for e in meta["scenarios"]), option
    one_set = [by_name[f"all_{contig}"] for contig in ("chrA", "chrB", "chrC")]
    assert all(e["kwargs"] == one_set[0]["kwargs"] and e["files"] == one_set[0]["files"] and e["step"] == one_set[0]["step"] for e in one_set)
    assert any(level == "WARNING" and "Excluding this track" in text for e in meta["scenarios"] for level, text in e["log"])
