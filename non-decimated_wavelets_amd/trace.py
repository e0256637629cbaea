"""Launch trace of libndwt_hip.so (include/ndwt.h: ndwt_trace_enable / ndwt_trace_get): which kernel instances a call ran.

    with kernel_trace() as recs:
        w.dec(x, 2)
    recs[0].family, recs[0].params["TY"], recs[0].grid

The library records the compiler's spelling of each launched type, e.g. "ndwt::Fwd3<float, 8, 64, 32, 1024, 4, true>"; clang
leaves out the trailing template arguments that equal their defaults, so `parse_record` fills them in from FAMILY_PARAMS, the
parameter lists of the kernel families in csrc/ndwt_device.h (the suite checks this table against the declarations).
"""
from __future__ import annotations

import contextlib
import ctypes
import re
from dataclasses import dataclass, field

# kernel family -> [(parameter name, default or None)] in declaration order (csrc/ndwt_device.h, trailing "_" dropped)
FAMILY_PARAMS = {
    "Fwd3": [("T", None), ("L", None), ("TX", None), ("TY", None), ("NT", None), ("RY", None), ("VEC4", None), ("WPE", 2), ("EW", 1),
             ("LOWONLY", False), ("TPRE", False), ("PIN", False), ("WLDS", 0)],
    "Inv3": [("T", None), ("L", None), ("TX", None), ("TY", None), ("NT", None), ("RY", None), ("VEC4", None), ("WPE", 2), ("EW", 1)],
    "Inv3S": [("T", None), ("L", None), ("TX", None), ("TY", None), ("NT", None), ("RY", None), ("VEC4", None), ("WPE", 2), ("EW", 1)],
    "Inv3Y": [("T", None), ("L", None), ("TX", None), ("TY", None), ("NT", None), ("VEC4", None), ("WPE", 4), ("DEPTH", 1), ("EW", 1),
              ("ZLDS", 0), ("XH", 0), ("UNIYZ", False), ("XSC", False)],
    "Den3": [("T", None), ("L", None), ("NT", 1024), ("WPE", 4), ("ZLDS", 0), ("TX", 64), ("TY", 32)],
    "Fwd2S": [("T", None), ("L", None), ("VEC4", None), ("WPE", 4), ("EW", 1)],
    "Fwd2C": [("T", None), ("L", None), ("NLEV", None), ("WPE", 2), ("EW", 1)],
    "Inv2S": [("T", None), ("L", None), ("VEC4", None), ("WPE", 4), ("EW", 1)],
    "Inv2P": [("T", None), ("L", None), ("PD", 2), ("WPE", 2), ("PK", False)],
    "Inv2C": [("T", None), ("L", None), ("NLEV", None), ("PD", 1), ("WPE", 2), ("EW", 1)],
    "AxisMarch": [("T", None), ("L", None), ("SYN", None)],
    "AxisX": [("T", None), ("L", None), ("SYN", None), ("EW", None), ("VEC4", None)],
}

# the families of csrc/ndwt_device_1d.h (the cascades and the one-launch denoise of a batched 1-D plan), in a table of their own: FAMILY_PARAMS is kept equal to
# the declarations of ndwt_device.h
FAMILY_PARAMS_1D = {
    "Fwd1C": [("T", None), ("L", None), ("NLEV", None), ("EW", 1), ("WPE", 4)],
    "Inv1C": [("T", None), ("L", None), ("NLEV", None), ("EW", 1), ("WPE", 4)],
    "Den1C": [("T", None), ("L", None), ("NLEV", None), ("EW", 1), ("WPE", 4), ("ROWTHR", False)],
}

# the families of csrc/ndwt_device_axis.h (all levels of one strided axis inside one march: plans over interleaved samples), likewise
FAMILY_PARAMS_AXIS = {
    "FwdMC": [("T", None), ("L", None), ("NLEV", None)],
    "InvMC": [("T", None), ("L", None), ("NLEV", None)],
}

# the families of csrc/ndwt_device_select.h (order statistics of a band: the histogram pass and the pick step of the radix select), likewise
FAMILY_PARAMS_SELECT = {
    "BandHist": [("T", None), ("COMP", None), ("VEC", None), ("AGG", 2)],
    "BandPick": [("T", None)],
}

# the families of csrc/ndwt_device_items.h (the per-item calls: the radix select of one item in one workgroup, the shrink of every (band, item) block
# with its own threshold), likewise
FAMILY_PARAMS_ITEMS = {
    "ItemSelect": [("T", None), ("COMP", None), ("VEC", None), ("AGG", 2)],
    "ShrinkItems": [("T", None), ("COMP", None), ("VEC", None)],
}

# the families of csrc/ndwt_device_norms.h (the band norms: l1, energy, max and non-zeros of every (band, item) block in one read, and the combine of
# the chunks of a block at the launch boundary), likewise
FAMILY_PARAMS_NORMS = {
    "BandNorms": [("T", None), ("COMP", None), ("VEC", None)],
    "NormsFinish": [("NT", 64)],
}

# the families of csrc/ndwt_device_risk.h (the SURE statistics of every (band, item) block at up to 8 thresholds in one read, and the combine of the
# chunks of a block), likewise
FAMILY_PARAMS_RISK = {
    "BandRisk": [("T", None), ("COMP", None), ("VEC", None)],
    "RiskFinish": [("NT", 64)],
}

# the families of csrc/ndwt_device_joint.h (joint shrinkage across the items of a plan and the norms of the groups), likewise
FAMILY_PARAMS_JOINT = {
    "JointShrink": [("T", None), ("COMP", None), ("VEC", None), ("REG", None)],
    "GroupNorms": [("T", None), ("COMP", None), ("VEC", None)],
}

# the families of csrc/ndwt_device_joint_tile.h (the same two calls for many short items: the items staged through an LDS tile), likewise
FAMILY_PARAMS_JOINT_TILE = {
    "JointTile": [("T", None), ("COMP", None), ("VEC", None)],
    "GroupNormsTile": [("T", None), ("COMP", None), ("VEC", None)],
}

# the family of csrc/ndwt_device_neigh.h (neighbourhood shrinkage: a window's energy inside a coefficient's own band decides it), likewise
FAMILY_PARAMS_NEIGH = {
    "NeighShrink": [("T", None), ("COMP", None), ("ND", None), ("R", None)],
}

# the plain __global__ templates (csrc/ndwt_api.hip, csrc/ndwt_multi.hip), as their launch sites spell them
PLAIN_PARAMS = {
    "axis_analysis_kernel": [("T", None)],
    "axis_synthesis_kernel": [("T", None)],
    "shrink_kernel": [("T", None), ("COMP", None), ("VEC", None)],
    "segments_kernel": [("VBYTES", None), ("ADD", None)],
    "segments_strided_kernel": [("T", None), ("VBYTES", None), ("ADD", None)],
    "add_planes_kernel": [("T", None)],
}

# __global__ wrappers that launch a family's block() (the record names the family)
WRAPPERS = ("fused3_kernel", "march_kernel")


@dataclass
class KernelLaunch:
    family: str
    params: dict = field(default_factory=dict)
    grid: tuple = (1, 1, 1)
    block: tuple = (1, 1, 1)
    text: str = ""

    def __repr__(self):
        p = ", ".join(f"{k}={v}" for k, v in self.params.items())
        return f"{self.family}<{p}> grid={self.grid} block={self.block}"


def _split_args(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _value(v):
    if v in ("true", "false"):
        return v == "true"
    if re.fullmatch(r"-?\d+", v):
        return int(v)
    return v


def parse_record(line: str) -> KernelLaunch:
    """One trace record -> KernelLaunch with every template parameter named (defaults filled in)."""
    m = re.fullmatch(r"\s*(.*?)\s+grid=\((\d+),(\d+),(\d+)\)\s+block=\((\d+),(\d+),(\d+)\)\s*", line)
    if not m:
        raise ValueError(f"malformed trace record: {line!r}")
    text = m.group(1)
    t = re.fullmatch(r"(?:ndwt::)?(\w+)(?:<(.*)>)?", text)
    if not t:
        raise ValueError(f"unparsed kernel type: {text!r}")
    fam = t.group(1)
    table = FAMILY_PARAMS.get(fam) or PLAIN_PARAMS.get(fam) or FAMILY_PARAMS_1D.get(fam) or FAMILY_PARAMS_AXIS.get(fam) or FAMILY_PARAMS_SELECT.get(fam) or FAMILY_PARAMS_ITEMS.get(fam) or FAMILY_PARAMS_NORMS.get(fam) or FAMILY_PARAMS_RISK.get(fam) or FAMILY_PARAMS_JOINT.get(fam) or FAMILY_PARAMS_JOINT_TILE.get(fam) or FAMILY_PARAMS_NEIGH.get(fam)
    if table is None:
        raise ValueError(f"unknown kernel family {fam!r} in {text!r}")
    args = [_value(a) for a in _split_args(t.group(2) or "")]
    if len(args) > len(table):
        raise ValueError(f"{fam}: {len(args)} template arguments, the table knows {len(table)}: {text!r}")
    params = {}
    for i, (name, default) in enumerate(table):
        if i < len(args):
            params[name] = args[i]
        elif default is None:
            raise ValueError(f"{fam}: parameter {name} has no default and is missing in {text!r}")
        else:
            params[name] = default
    grid = tuple(int(m.group(i)) for i in (2, 3, 4))
    block = tuple(int(m.group(i)) for i in (5, 6, 7))
    return KernelLaunch(fam, params, grid, block, text)


def parse_log(text: str) -> list:
    return [parse_record(line) for line in text.splitlines() if line.strip()]


def read_log(lib) -> str:
    need = lib.ndwt_trace_get(None, 0)
    buf = ctypes.create_string_buffer(need)
    lib.ndwt_trace_get(buf, need)
    return buf.value.decode()


@contextlib.contextmanager
def kernel_trace():
    """Record the kernel launches made inside the block; yields a list that holds the parsed records once the block ends.
    Records are taken on the host at launch time: no synchronization is needed to see them."""
    from ._lib import lib
    L = lib()
    recs = []
    L.ndwt_trace_enable(1)
    try:
        yield recs
    finally:
        L.ndwt_trace_enable(0)
        recs.extend(parse_log(read_log(L)))
