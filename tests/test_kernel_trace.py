"""The launch trace (include/ndwt.h: ndwt_trace_enable / ndwt_trace_get) and its parser, without a GPU.

The parser names template arguments from a table (non-decimated_wavelets_amd/trace.py: FAMILY_PARAMS); these tests keep that table
equal to the declarations in csrc/ndwt_device.h, and keep the coverage list of tests/test_gpu_dispatch.py equal to the kernels in csrc/,
so that a new template parameter or a new kernel cannot land without the dispatch tests seeing it.
"""
import ctypes
import glob
import os
import re

import pytest

import ndwt_amd as ndwt
from helpers import COVERAGE, parse_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")


def _value(v):
    v = v.strip()
    return v == "true" if v in ("true", "false") else int(v)


def _device_families():
    """{family: [(name, default)]} of every template struct in ndwt_device.h that has a block() (a kernel body)."""
    txt = open(os.path.join(CSRC, "ndwt_device.h")).read()
    decls = [(m.start(), m.group(1), m.group(2)) for m in re.finditer(r"^template\s*<([^;{}]*?)>\s*struct\s+(\w+)\s*\{", txt, re.M)]
    fams = {}
    for blk in re.finditer(r"static NDWT_DEV void block\(", txt):
        pos, params, name = [d for d in decls if d[0] < blk.start()][-1]
        out = []
        for p in params.split(","):
            m = re.fullmatch(r"\s*(?:typename|class|int|bool)\s+(\w+?)_?\s*(?:=\s*(\S+))?\s*", p)
            assert m, (name, p)
            out.append((m.group(1), None if m.group(2) is None else _value(m.group(2))))
        fams[name] = out
    return fams


def _global_kernels():
    names = set()
    for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        txt = re.sub(r"//[^\n]*", "", open(f).read())
        names |= set(re.findall(r"__global__.{0,200}?\bvoid\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\s*\(", txt, re.S))
    return names


def test_parameter_table_matches_the_kernel_family_declarations():
    fams = _device_families()
    assert len(fams) >= 12
    assert fams == ndwt.trace.FAMILY_PARAMS


def test_coverage_list_names_every_kernel_in_csrc():
    """COVERAGE (the GPU coverage test's list) holds an entry for every kernel family and every plain __global__ kernel"""
    kernels = _global_kernels()
    assert "shrink_kernel" in kernels and "fused3_kernel" in kernels
    want = set(_device_families()) | (kernels - set(ndwt.trace.WRAPPERS))
    listed = {fam for fam, _ in COVERAGE}
    assert listed == want, (sorted(want - listed), sorted(listed - want))
    assert set(ndwt.trace.PLAIN_PARAMS) == kernels - set(ndwt.trace.WRAPPERS)


def test_parser_fills_in_the_defaults_clang_leaves_out():
    r = parse_record("ndwt::Fwd3<float, 8, 64, 32, 1024, 4, true> grid=(512,1,1) block=(1024,1,1)")
    assert r.family == "Fwd3" and r.params["L"] == 8 and r.params["TY"] == 32 and r.params["VEC4"] is True
    assert r.params["WPE"] == 2 and r.params["EW"] == 1 and r.params["PIN"] is False and r.params["WLDS"] == 0
    assert r.grid == (512, 1, 1) and r.block == (1024, 1, 1)
    r = parse_record("ndwt::Inv3Y<float, 12, 64, 32, 1024, true, 4, 2, 1, 6, 0, true, true> grid=(256,1,1) block=(1024,1,1)")
    assert r.params["UNIYZ"] is True and r.params["XSC"] is True and r.params["ZLDS"] == 6
    r = parse_record("ndwt::shrink_kernel<double, 2, false> grid=(4,1,1) block=(256,1,1)")
    assert r.params == {"T": "double", "COMP": 2, "VEC": False}
    with pytest.raises(ValueError, match="unknown kernel family"):
        parse_record("ndwt::Nope<float> grid=(1,1,1) block=(1,1,1)")
    with pytest.raises(ValueError, match="template arguments"):
        parse_record("ndwt::AxisMarch<float, 8, true, 1> grid=(1,1,1) block=(256,1,1)")
    with pytest.raises(ValueError, match="no default"):
        parse_record("ndwt::AxisX<float, 8, true> grid=(1,1,1) block=(256,1,1)")


def test_trace_functions_through_ctypes():
    """on, get, off, through ctypes and without a launch: the empty log, the length contract of ndwt_trace_get, the previous state"""
    lib = ndwt.lib()
    lib.ndwt_trace_enable(0)
    assert lib.ndwt_trace_enable(1) == 0
    assert lib.ndwt_trace_enable(1) == 1                  # on again: cleared again
    assert lib.ndwt_trace_get(None, 0) == 1               # the empty log: just the terminator
    buf = ctypes.create_string_buffer(8)
    assert lib.ndwt_trace_get(buf, 8) == 1 and buf.value == b""
    assert lib.ndwt_trace_enable(0) == 1
    with ndwt.kernel_trace() as recs:
        pass
    assert recs == []
    assert lib.ndwt_trace_enable(0) == 0                  # the context manager turned it off again
