"""The tile form of the joint shrinkage and the group norms without a GPU: the trace parser's table of the two new kernel families against
the template heads of csrc/ndwt_device_joint_tile.h, and the text of include/ndwt.h that names the route and its hook.  (No new export:
the calls are those of tests/test_abi_joint.py.)
"""
import os
import re

import ndwt_amd as ndwt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc", "ndwt_device_joint_tile.h")


def test_the_trace_parser_knows_the_two_families():
    r = ndwt.trace.parse_record("ndwt::JointTile<float, 1, true> grid=(384,1,1) block=(256,1,1)")
    assert r.family == "JointTile" and r.params == {"T": "float", "COMP": 1, "VEC": True} and r.grid == (384, 1, 1) and r.block == (256, 1, 1)
    r = ndwt.trace.parse_record("ndwt::GroupNormsTile<double, 2, false> grid=(7,1,1) block=(256,1,1)")
    assert r.family == "GroupNormsTile" and r.params == {"T": "double", "COMP": 2, "VEC": False} and r.grid == (7, 1, 1)
    assert set(ndwt.trace.FAMILY_PARAMS_JOINT_TILE) == {"JointTile", "GroupNormsTile"}
    assert set(ndwt.trace.FAMILY_PARAMS_JOINT) == {"JointShrink", "GroupNorms"}          # the chunk form's table stays what it was


def test_the_table_of_the_parser_matches_the_declarations():
    """FAMILY_PARAMS_JOINT_TILE against the template heads of the header, as test_abi_joint.py holds its table to its header"""
    txt = open(HEADER).read()
    for fam, table in ndwt.trace.FAMILY_PARAMS_JOINT_TILE.items():
        m = re.search(r"template <([^>]*)> struct " + fam + r" \{", txt)
        assert m, fam
        params = []
        for p in m.group(1).split(","):
            decl, _, default = p.strip().partition("=")
            name = decl.split()[-1].rstrip("_")
            d = default.strip()
            params.append((name, None if not d else (d == "true") if d in ("true", "false") else int(d)))
        assert params == table, (fam, params)
    # every struct of the header with a kernel body is in the table
    heads = re.findall(r"template <[^>]*> struct (\w+) \{(?:(?!\ntemplate <).)*?static NDWT_DEV void block\(", txt, re.S)
    assert set(heads) == set(ndwt.trace.FAMILY_PARAMS_JOINT_TILE), heads


def test_the_new_header_adds_no_global_and_the_units_launch_through_launch_select_k():
    csrc = os.path.dirname(HEADER)
    assert "__global__" not in open(HEADER).read()
    for unit in ("ndwt_joint_tile_f32.hip", "ndwt_joint_tile_f64.hip"):
        txt = open(os.path.join(csrc, unit)).read()
        assert "__global__" not in txt and "launch_select_k<JointTile<" in txt and "launch_select_k<GroupNormsTile<" in txt, unit
        assert unit in open(os.path.join(csrc, "Makefile")).read(), unit


def test_the_header_names_the_route_and_the_hook():
    hdr = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "ndwt.h")).read())
    part = hdr[hdr.index("joint shrinkage across the items of a plan"):hdr.index("int ndwt_shrink_joint(")]
    for words in ("JointTile", "GroupNormsTile", "LDS tile", "ndwt_plan_set_variant", "variant_inv 11", "variant_inv 9", "fewer than 64 items", "same bits"):
        assert words in part, words
    # what was true stays said
    for words in ("Not built:", "Den1C", "`inner` axis", "per-item weights", "a norm fused into the shrink", "MATLAB gateway", "a NaN", "explicit zero",
                  "hipEventSynchronize", "captured into a graph"):
        assert words in part, words
