"""The kernels held to their smallest taps: every listed single-precision instance of 10 taps or more (csrc/ndwt_fused_list.h), one case
per cascaded family at 8 taps and one double case per family, on the comb inputs of tests/bound_cases.py under its componentwise bound

    |got - want| <= c u (|W| |x|)   at every element,   got == 0 exactly where no tap reaches,

with c = levels * sum over the filtered axes of (L_a + 2), derived there.  The parity tests measure max|got - want| / max|want| on white
noise, which an outer tap of db7 .. db10 (2e-5 .. 5e-4 of the largest) can be wrong under; here an element that is one product of taps is
checked against its own size.

A case pins its route the way tests/test_gpu_dispatch.py does (set_variant, chunk, the shape) and asserts the launch trace, so it names the
instance that ran; test_every_listed_long_instance_ran holds the cases against the instance lists (tests/select/list_shim.cpp): no listed
float instance of 10 taps or more may be missing.  The impulses sit on the first and last sample of every axis and either side of the
tile, chunk and wave-row edges of the instance; every buffer lies between NaN guards that must stay NaN, and outputs start as NaN.
Each case prints its worst ratio against the cap (records for DESIGN.md; the assertion is the derived cap).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import bound_cases as bc
import ndwt_amd as ndwt
import ndwt_oracle as orc
from helpers import check_trace, matches, spec

pytestmark = pytest.mark.gpu

GUARD = 8                                                        # elements of NaN on either side of every buffer (keeps 16-byte alignment)
RATIOS = {}                                                      # case id -> {family: worst ratio}, of the cases that passed
_RECS = {}                                                       # case id -> launch records of a case that passed


# ---- the cases
def _wl(wn, d):
    return [wn] * d if isinstance(wn, str) else list(wn)


def mixed(L, kind="even", long_axis=0):
    """three wavelets padded to L taps: 'even' -- (L, L - 4, L - 8) taps, even zero padding (Fwd3 PIN, Inv3Y), the longest on `long_axis`;
    'uniyz' -- the same L-tap wavelet on y and z, 4 taps fewer on x (Inv3Y UNIYZ); 'odd' -- (L, L - 2, L - 2): odd padding (Inv3S);
    'yz' -- L on x and y, L - 4 on z (Inv3Y without the shared tap pairs)"""
    k = L // 2
    if kind == "uniyz":
        return [f"db{k - 2}", f"db{k}", f"db{k}"]
    if kind == "odd":
        return [f"db{k}", f"db{k - 1}", f"db{k - 1}"]
    if kind == "yz":
        return [f"db{k}", f"db{k}", f"db{k - 2}"]
    w = [f"db{k}", f"db{max(k - 2, 1)}", f"db{max(k - 4, 1)}"]
    return w[-long_axis:] + w[:-long_axis] if long_axis else w


CASES = []


def case(cid, dims, wn, dec=(), rec=(), cplx=False, prec="single", dil="reference", level=1, l2=0, fwd=-1, inv=-1, chunk=None, edges=None,
         kind="nd", K=1, inner=1, den=(), redges=None):
    """dec / rec / den: the launch specs of the call (helpers.check_trace), empty = the call is not made.  edges: per axis, the interior
    tile / chunk / wave-row starts of the analysis instance (redges: of the synthesis instance, default the same), in elements.
    kind: 'nd' a plain plan over dims; 'batch' K signals of dims[0] (ndwt_plan_create_many); 'inter' K items of dims[0] samples of `inner`
    elements (ndwt_plan_create_interleaved)"""
    d = len(dims)
    edges = edges or [[] for _ in dims]
    CASES.append(pytest.param(dict(id=cid, dims=list(dims), wn=_wl(wn, d), dec=list(dec), rec=list(rec), den=list(den), cplx=cplx, prec=prec,
                                   dil=dil, level=level, l2=l2, fwd=fwd, inv=inv, chunk=chunk, edges=edges, redges=redges or edges, kind=kind,
                                   K=K, inner=inner), id=cid))


def _e(n, *tiles):
    """edges of an axis of n under tiles of the given sizes: the starts of clipped tiles and of a last tile anchored at the end"""
    return sorted({e for t in tiles for e in bc.tile_edges(n, t, anchor_last=True)})


V4, RG, V4C, RGC, ZC = [72, 40, 33], [70, 37, 33], [36, 40, 33], [35, 37, 33], 17   # whole groups of 4 scalars / ragged rows; two z chunks
FTILE = {1: "TY=16 NT=512 RY=4", 2: "TY=32 NT=1024 RY=4", 6: "TY=32 NT=1024 RY=2"}   # Fused3Tile<float, false, V>
FTY = {1: 16, 2: 32, 6: 32}

# Fwd3, real data: (L, rows in whole groups of 4, fwd variant, tile V, PIN, WLDS) -- fused3_select, branch by branch
FWD3 = [(10, 1, 0, 6, 1, 0), (10, 1, 8, 2, 0, 0), (10, 0, 0, 2, 0, 0), (10, 1, 1, 1, 0, 0), (10, 0, 1, 1, 0, 0), (10, 1, 6, 6, 0, 0), (10, 0, 6, 6, 0, 0),
        (12, 1, 0, 6, 1, 0), (12, 1, 8, 6, 0, 0), (12, 0, 0, 6, 0, 0), (12, 1, 2, 2, 0, 0), (12, 0, 2, 2, 0, 0), (12, 1, 1, 1, 0, 0), (12, 0, 1, 1, 0, 0),
        (14, 1, 0, 6, 1, 0), (14, 1, 8, 6, 0, 0), (14, 0, 0, 6, 0, 0), (14, 1, 1, 1, 0, 0), (14, 0, 1, 1, 0, 0),
        (16, 1, 0, 6, 0, 2), (16, 1, 3, 6, 0, 0), (16, 0, 0, 6, 0, 0), (16, 1, 1, 1, 0, 0), (16, 0, 1, 1, 0, 0),
        (18, 1, 0, 1, 0, 0), (18, 0, 0, 1, 0, 2), (18, 0, 3, 1, 0, 0),
        (20, 1, 0, 1, 0, 4), (20, 1, 3, 1, 0, 0), (20, 0, 0, 1, 0, 6), (20, 0, 3, 1, 0, 0)]
for i, (L, v4, vf, V, pin, wlds) in enumerate(FWD3):
    dims = V4 if v4 else RG
    wn = mixed(L, "even", long_axis=i % 3) if i % 2 else f"db{L // 2}"          # uniform and mixed wavelets alternate; the long one moves
    case(f"fwd3-{L}-{'v4' if v4 else 'rg'}-f{vf}", dims, wn, level=1 + i % 2, l2=i % 2, fwd=vf, chunk=ZC,
         edges=[_e(dims[0], 64), _e(dims[1], FTY[V]), [ZC]],
         dec=[f"Fwd3 T=float L={L} {FTILE[V]} VEC4={'true' if v4 else 'false'} EW=1 PIN={'true' if pin else 'false'} TPRE=false WLDS={wlds}"])
# ... interleaved complex64, 10 .. 16 taps: one column per thread
for i, L in enumerate((10, 12, 14, 16)):
    for v4 in (1, 0):
        dims = V4C if v4 else RGC
        case(f"fwd3-c64-{L}-{'v4' if v4 else 'rg'}", dims, mixed(L, "even", long_axis=i % 3) if v4 else f"db{L // 2}", cplx=True, level=1 + v4, l2=v4,
             chunk=ZC, edges=[_e(dims[0], 32), _e(dims[1], 16), [ZC]],
             dec=[f"Fwd3 T=float L={L} {FTILE[1]} VEC4={'true' if v4 else 'false'} EW=2 PIN=false TPRE=false WLDS=0"])


def _y(L, v4, ew, depth, uni, xsc):
    zlds = 0 if ew != 1 else 6 if (depth == 2 and L == 12) else 2 if (depth == 2 and L == 10) else 8 if L >= 18 else 0   # inv3y_zlds
    return (f"Inv3Y T=float L={L} VEC4={'true' if v4 else 'false'} EW={ew} DEPTH={depth} ZLDS={zlds} UNIYZ={'true' if uni else 'false'} "
            f"XSC={'true' if xsc else 'false'}")


def _ytile(L, ew):
    """inv3y_tx / inv3y_ty of csrc/ndwt_fused_tile.h, TX in elements"""
    tx = (64 if L <= 10 else 48) // 2 if ew == 2 else (64 if L <= 18 else 48)
    ty = 32 if ew == 2 else (32 if L <= 16 else 24 if L <= 18 else 28)
    return tx, ty


# Inv3Y, real data: (L, rows in whole groups of 4, inv variant, wavelets, DEPTH, UNIYZ, XSC)
INV3Y = [(12, 1, 11, "uni", 2, 1, 0), (14, 1, 11, "uni", 1, 1, 0), (16, 1, 11, "uni", 1, 1, 0), (18, 1, 11, "uni", 1, 1, 0), (20, 1, 11, "uni", 1, 1, 0),
         (10, 1, 11, "uni", 2, 0, 0), (10, 1, 5, "uni", 1, 0, 0), (10, 0, 0, "uni", 1, 0, 0),
         (12, 1, 11, "yz", 2, 0, 0), (12, 1, 5, "uni", 1, 0, 0), (12, 0, 0, "even", 1, 0, 0),
         (14, 1, 11, "yz", 1, 0, 0), (14, 0, 0, "uni", 1, 0, 0), (16, 1, 11, "yz", 1, 0, 0), (16, 0, 0, "even", 1, 0, 0),
         (18, 1, 11, "yz", 1, 0, 0), (18, 0, 0, "uni", 1, 0, 0), (20, 1, 11, "yz", 1, 0, 0), (20, 0, 0, "even", 1, 0, 0),
         # the x stage in scatter form: the default from 10 taps on rows of whole groups of 4
         (10, 1, 0, "uni", 2, 0, 1), (12, 1, 0, "yz", 2, 0, 1), (12, 1, 0, "uniyz", 2, 1, 1),
         (14, 1, 0, "yz", 1, 0, 1), (14, 1, 0, "uni", 1, 1, 1), (16, 1, 0, "even", 1, 0, 1), (16, 1, 0, "uniyz", 1, 1, 1),
         (18, 1, 0, "yz", 1, 0, 1), (18, 1, 0, "uni", 1, 1, 1), (20, 1, 0, "even", 1, 0, 1), (20, 1, 0, "uniyz", 1, 1, 1)]
for i, (L, v4, vi, wk, depth, uni, xsc) in enumerate(INV3Y):
    dims = V4 if v4 else RG
    tx, ty = _ytile(L, 1)
    wn = f"db{L // 2}" if wk == "uni" else mixed(L, wk, long_axis=(i % 3 if wk == "even" else 0))
    case(f"inv3y-{L}-{'v4' if v4 else 'rg'}-i{vi}-{wk}{'-xsc' if xsc else ''}", dims, wn, level=1 + i % 2, l2=i % 2, inv=vi, chunk=ZC,
         edges=[_e(dims[0], tx), _e(dims[1], ty), [ZC]], rec=[_y(L, v4, 1, depth, uni, xsc)])
# ... interleaved complex64: scatter form by default on rows of whole groups of 4, gather form on request and on ragged rows
for i, L in enumerate((10, 12, 14, 16)):
    tx, ty = _ytile(L, 2)
    for v4, vi, xsc in ((1, 0, 1), (1, 11, 0), (0, 0, 0)):
        dims = V4C if v4 else RGC
        case(f"inv3y-c64-{L}-{'v4' if v4 else 'rg'}-i{vi}", dims, mixed(L, "even", long_axis=i % 3) if xsc else f"db{L // 2}", cplx=True,
             level=1 + (i + vi) % 2, l2=i % 2, inv=vi, chunk=ZC, edges=[_e(dims[0], tx), _e(dims[1], ty), [ZC]], rec=[_y(L, v4, 2, 1, 0, xsc)])
# Inv3S, 10 .. 16 taps: the lane-shift kernel on request (rows of whole groups of 4) and for wavelets with odd tap padding (ragged rows)
STILE = {1: "TY=32 NT=1024 RY=1", 2: "TY=32 NT=512 RY=1"}
for L, ew in ((10, 1), (12, 1), (14, 1), (16, 1), (10, 2), (12, 2)):
    V = 1 if (L, ew) == (10, 1) else 2
    for v4 in (1, 0):
        dims = ((V4C if v4 else RGC) if ew == 2 else (V4 if v4 else RG))
        case(f"inv3s-{L}-ew{ew}-{'v4' if v4 else 'rg'}", dims, f"db{L // 2}" if v4 else mixed(L, "odd"), cplx=ew == 2, level=2 - v4, l2=v4,
             inv=4 if v4 else -1, chunk=ZC, edges=[_e(dims[0], 64 // ew), _e(dims[1], 32), [ZC]],
             rec=[f"Inv3S T=float L={L} {STILE[V]} VEC4={'true' if v4 else 'false'} EW={ew}"])


# ---- one level of an image: Fwd2S / Inv2S, one wave per row segment of wave_row_width scalars; rows in chunks
def wave_row_width(syn, Lp, ew, f64=False, nlev=1):
    """csrc/ndwt_fused_tile.h: scalars of a row one wave stores"""
    (LH, RH), lpl = ((Lp // 2, Lp // 2 - 1) if syn else (Lp // 2 - 1, Lp // 2)), (4 if f64 else 8)
    GL, GR = (LH * ew + 3) // 4, (RH * ew + 3) // 4
    return 4 * (64 - GL - GR) if nlev == 1 else 4 * ((64 - nlev * (GL + GR)) // lpl * lpl)


def wpe(f64, Lp, ew):
    return 2 if (f64 or (Lp >= 14 if ew == 1 else (ew == 2 and Lp >= 10))) else 4                  # fused2s_wpe


I4, IR, I4C, IRC, YC = [260, 70], [254, 70], [130, 70], [127, 70], 35
for i, (L, ew) in enumerate([(L, 1) for L in (10, 12, 14, 16, 18, 20)] + [(L, 2) for L in (10, 12, 14, 16)]):
    for v4 in (1, 0):
        dims = ((I4C if v4 else IRC) if ew == 2 else (I4 if v4 else IR))
        wx = wave_row_width(False, L, ew) // ew
        wn = f"db{L // 2}" if (i + v4) % 2 else ([f"db{L // 2}", f"db{L // 2 - 3}"] if v4 else [f"db{L // 2 - 3}", f"db{L // 2}"])
        tail = f"T=float L={L} VEC4={'true' if v4 else 'false'} WPE={wpe(False, L, ew)} EW={ew}"
        case(f"2s-{L}-ew{ew}-{'v4' if v4 else 'rg'}", dims, wn, cplx=ew == 2, level=1 + (i + v4) % 2, l2=(i + v4) % 2, chunk=YC,
             inv=1 if (v4 and ew == 1 and L <= 12) else -1,                                        # (Inv2P would take these: keep Inv2S)
             edges=[_e(dims[0], wx), [YC]], dec=["Fwd2S " + tail], rec=["Inv2S " + tail])
# Inv2P: 12 taps packed (depth 4), with scalar FMAs, at depth 2; 10 taps
for cid, L, vi, pd, pk in (("pk", 12, -1, 4, 1), ("unpacked", 12, 7, 4, 0), ("depth2", 12, 6, 2, 0), ("10", 10, -1, 2, 0)):
    case(f"inv2p-{cid}", I4, [f"db{L // 2}", f"db{L // 2 - 2}"] if pk else f"db{L // 2}", level=1 + pk, l2=pk, inv=vi, chunk=YC,
         edges=[_e(260, wave_row_width(True, L, 1)), [YC]], rec=[f"Inv2P T=float L={L} PD={pd} PK={'true' if pk else 'false'}"])
# Fwd2C with 12 taps, two levels in one launch (on request below 24 MiB)
case("fwd2c-12", I4, "db6", level=2, l2=1, fwd=11, chunk=YC, edges=[_e(260, wave_row_width(False, 12, 1, nlev=2)), [YC]],
     dec=["Fwd2C T=float L=12 NLEV=2 WPE=2 EW=1"])


# ---- the per-axis passes
def _march_edges(n, L):
    ch = min(n, max(4 * (L - 1), 8))                             # march_chunks at few workgroups: the floor of 4 (L - 1) planes
    return list(range(ch, n, ch))


for L in (10, 12, 14, 16, 18, 20):                               # AxisMarch on a strided axis: 3 items of 100 samples of 4 floats
    case(f"march-{L}", [100], f"db{L // 2}", kind="inter", K=3, inner=4, level=2, l2=(L // 2) % 2, edges=[_march_edges(100, L)],
         dec=[f"AxisMarch T=float L={L} SYN=false"], rec=[f"AxisMarch T=float L={L} SYN=true"])
for L in (10, 12):                                               # AxisX on the contiguous axis: two wave segments, the second ragged
    for ew in (1, 2):
        for v4 in (1, 0):
            n = (300 if v4 else 302) // ew
            wx = wave_row_width(False, L, ew) // ew
            case(f"axisx-{L}-ew{ew}-{'v4' if v4 else 'rg'}", [n], f"db{L // 2}", cplx=ew == 2, level=2, l2=v4, edges=[_e(n, wx)],
                 dec=[f"AxisX T=float L={L} SYN=false EW={ew} VEC4={'true' if v4 else 'false'}"],
                 rec=[f"AxisX T=float L={L} SYN=true EW={ew} VEC4={'true' if v4 else 'false'}"])
# the element-wise kernels at 20 taps (a row below 8 L scalars has no AxisX, beyond 12 taps nothing has)
case("plain-20", [100], "db10", level=2, l2=1, edges=[[50]], dec=["axis_analysis_kernel T=float"], rec=["axis_synthesis_kernel T=float"])

# ---- the cascaded families at 8 taps: the comb straddles the wave-row edge, which is the same line at every level of the launch
W1 = wave_row_width(False, 8, 1, nlev=3)
case("fwd1c-inv1c-8", [W1 + 32], "db4", kind="batch", K=3, level=3, l2=1, edges=[[W1]], dec=["Fwd1C T=float L=8 NLEV=3 EW=1"],
     rec=["Inv1C T=float L=8 NLEV=3 EW=1"])
case("fwdmc-invmc-8", [100], "db4", kind="inter", K=3, inner=4, level=3, l2=0, fwd=11, inv=11, edges=[_march_edges(100, 8)],
     dec=["FwdMC T=float L=8 NLEV=3"], rec=["InvMC T=float L=8 NLEV=3"])
case("fwd2c-inv2c-8", I4, ["db4", "db3"], level=3, l2=1, fwd=11, inv=11, chunk=YC, edges=[_e(260, W1), [YC]],
     dec=["Fwd2C T=float L=8 NLEV=3 WPE=2 EW=1"], rec=["Inv2C T=float L=8 NLEV=3 PD=1 WPE=2 EW=1"])
WD = 4 * ((64 - 2 * 4) // 8 * 8)                                 # den1_tile_width(8, 1, false, 2)
case("den1c-8", [WD + 32], "db4", kind="batch", K=3, level=2, l2=1, fwd=11, inv=11, edges=[[WD]], den=["Den1C T=float L=8 NLEV=2 EW=1"])

# ---- a-trous dilation, one case per dilated family: the fused kernels on sub-lattices (EW = 2, 4; up to 8 taps), the lane-shift synthesis
# on request, the images, and a 1-D signal whose levels run AxisX, the element-wise kernels and AxisMarch on [8][4]
A3 = [[16], [16], [16]]
case("atrous-3d", [32, 32, 32], "db4", dil="atrous", level=3, l2=1, edges=A3,
     dec=["Fwd3 T=float L=8 EW=1", "Fwd3 T=float L=8 EW=2", "Fwd3 T=float L=8 EW=4"],
     rec=["Inv3Y L=8 EW=1", "Inv3Y L=8 EW=2 XSC=false", "Inv3Y L=8 EW=4 XSC=true"])
case("atrous-3d-inv3s", [32, 32, 32], "db4", dil="atrous", level=3, l2=0, inv=2, edges=A3,
     rec=["Inv3Y L=8 EW=1", "Inv3S T=float L=8 EW=2", "Inv3S T=float L=8 EW=4"])
case("atrous-2d", [72, 40], ["db4", "db2"], dil="atrous", level=3, l2=1, edges=[[36], [20]],
     dec=["Fwd2S T=float L=8 EW=1", "Fwd2S T=float L=8 EW=2", "Fwd2S T=float L=8 EW=4"],
     rec=["Inv2S T=float L=8 EW=1", "Inv2S T=float L=8 EW=2", "Inv2S T=float L=8 EW=4"])
case("atrous-1d", [32], "db2", dil="atrous", level=3, l2=0, edges=[[16]],
     dec=["AxisX T=float L=4 SYN=false", "axis_analysis_kernel T=float", "AxisMarch T=float L=4 SYN=false"],
     rec=["AxisX T=float L=4 SYN=true", "axis_synthesis_kernel T=float", "AxisMarch T=float L=4 SYN=true"])

# ---- double: one case per family at its longest listed tap length, real and complex128
D4, DRC, DZC = [72, 20, 20], [35, 19, 20], 10                     # (64 x 8 tiles; small: the reference of these runs in extended precision)
case("f64-fwd3-inv3s-16", D4, "db8", prec="double", level=2, l2=1, chunk=DZC, edges=[_e(72, 64), _e(20, 8), [DZC]],
     dec=["Fwd3 T=double L=16 TY=8 NT=512 VEC4=true EW=1 WLDS=2"], rec=["Inv3S T=double L=16 TY=8 NT=512 VEC4=true EW=1"])
case("c128-fwd3-12", [36, 20, 20], "db6", prec="double", cplx=True, level=1, l2=0, chunk=DZC, edges=[_e(36, 32), _e(20, 8), [DZC]],
     dec=["Fwd3 T=double L=12 TY=8 NT=512 VEC4=true EW=2 WLDS=2"])
case("c128-inv3s-10", DRC, "db5", prec="double", cplx=True, level=2, l2=1, chunk=DZC, edges=[_e(35, 32), _e(19, 8), [DZC]],
     dec=["Fwd3 T=double L=10 TY=8 NT=512 VEC4=false EW=2"], rec=["Inv3S T=double L=10 TY=8 NT=512 VEC4=false EW=2"])
case("f64-2s-16", IR, ["db8", "db5"], prec="double", level=2, l2=0, chunk=YC, edges=[_e(254, wave_row_width(False, 16, 1)), [YC]],
     dec=["Fwd2S T=double L=16 VEC4=false WPE=2 EW=1"], rec=["Inv2S T=double L=16 VEC4=false WPE=2 EW=1"])
case("c128-2s-8", I4C, "db4", prec="double", cplx=True, level=1, l2=1, chunk=YC, edges=[_e(130, wave_row_width(False, 8, 2) // 2), [YC]],
     dec=["Fwd2S T=double L=8 VEC4=true WPE=2 EW=2"], rec=["Inv2S T=double L=8 VEC4=true WPE=2 EW=2"])
case("f64-inv2p-8", I4, "db4", prec="double", level=2, l2=1, chunk=YC, edges=[_e(260, wave_row_width(True, 8, 1)), [YC]],
     dec=["Fwd2S T=double L=8 VEC4=true WPE=2 EW=1"], rec=["Inv2P T=double L=8 PD=2 PK=false"])
W2D = wave_row_width(False, 8, 1, f64=True, nlev=2)
case("f64-fwd2c-inv2c-8", I4, "db4", prec="double", level=2, l2=0, fwd=11, inv=11, chunk=YC, edges=[_e(260, W2D), [YC]],
     dec=["Fwd2C T=double L=8 NLEV=2 EW=1"], rec=["Inv2C T=double L=8 NLEV=2 EW=1"])
case("c128-fwd2c-inv2c-8", I4C, "db4", prec="double", cplx=True, level=2, l2=1, fwd=11, inv=11, chunk=YC,
     edges=[_e(130, wave_row_width(False, 8, 2, f64=True, nlev=2) // 2), [YC]], dec=["Fwd2C T=double L=8 NLEV=2 EW=2"], rec=["Inv2C T=double L=8 NLEV=2 EW=2"])
case("f64-march-20", [100], "db10", prec="double", kind="inter", K=3, inner=4, level=2, l2=1, edges=[_march_edges(100, 20)],
     dec=["AxisMarch T=double L=20 SYN=false"], rec=["AxisMarch T=double L=20 SYN=true"])
case("c128-march-20", [100], "db10", prec="double", cplx=True, kind="inter", K=2, inner=2, level=1, l2=0, edges=[_march_edges(100, 20)],
     dec=["AxisMarch T=double L=20 SYN=false"], rec=["AxisMarch T=double L=20 SYN=true"])
case("f64-axisx-12", [300], "db6", prec="double", level=2, l2=0, edges=[_e(300, wave_row_width(False, 12, 1, f64=True))],
     dec=["AxisX T=double L=12 SYN=false EW=1 VEC4=true"], rec=["AxisX T=double L=12 SYN=true EW=1 VEC4=true"])
case("c128-axisx-12", [151], "db6", prec="double", cplx=True, level=2, l2=1, edges=[_e(151, wave_row_width(False, 12, 2, f64=True) // 2)],
     dec=["AxisX T=double L=12 SYN=false EW=2 VEC4=false"], rec=["AxisX T=double L=12 SYN=true EW=2 VEC4=false"])
W1D = wave_row_width(False, 8, 1, f64=True, nlev=3)
case("f64-fwd1c-inv1c-8", [W1D + 32], "db4", prec="double", kind="batch", K=3, level=3, l2=0, edges=[[W1D]],
     dec=["Fwd1C T=double L=8 NLEV=3 EW=1"], rec=["Inv1C T=double L=8 NLEV=3 EW=1"])
W1Z = wave_row_width(False, 8, 2, f64=True, nlev=2) // 2
case("c128-fwd1c-inv1c-8", [W1Z + 16], "db4", prec="double", cplx=True, kind="batch", K=3, level=2, l2=1, edges=[[W1Z]],
     dec=["Fwd1C T=double L=8 NLEV=2 EW=2"], rec=["Inv1C T=double L=8 NLEV=2 EW=2"])
case("f64-fwdmc-invmc-8", [100], "db4", prec="double", kind="inter", K=3, inner=4, level=2, l2=1, fwd=11, inv=11, edges=[_march_edges(100, 8)],
     dec=["FwdMC T=double L=8 NLEV=2"], rec=["InvMC T=double L=8 NLEV=2"])
WDD = 4 * ((64 - 2 * 4) // 4 * 4)
case("f64-den1c-8", [WDD + 32], "db4", prec="double", kind="batch", K=3, level=2, l2=0, fwd=11, inv=11, edges=[[WDD]],
     den=["Den1C T=double L=8 NLEV=2 EW=1"])


# ---- the references: computed once per (shape, wavelets, setting, edges) and shared by the cases that differ in the pinned route only
def _reach(L, level, dil):
    return level * L if dil == "reference" else ((1 << level) - 1) * (L - 1) + 1


def _walk(direction, v, filt, level, l2, dil, hp):
    """the oracle's level walk; hp: in extended precision, for the double cases (the reference must be better than what it judges)"""
    if hp:
        v = v.astype(np.clongdouble if np.iscomplexobj(v) else np.longdouble)
    return bc.walk_dec(v, filt, level, l2, dil) if direction == "dec" else bc.walk_rec(v, filt, l2, dil, level)


@functools.lru_cache(maxsize=None)
def reference(direction, dims, wn, cplx, level, l2, dil, edges, hp, columns):
    """[(band or None, input, want, cond)] of the combs of one setting.  columns: 0 = an N-D array of `dims`; else that many 1-D signals of
    dims[0] (a batch, or the columns of interleaved samples), comb m scaled by another amplitude in every column: arrays [n, columns]"""
    filt = bc.filters(list(wn))
    pos = [bc.axis_positions(n, e) for n, e in zip(dims, edges)]
    reach = [_reach(len(f[0]), level, dil) for f in filt]
    ins = ([(None, x) for x in bc.combs(dims, pos, reach, cplx, pairs=True)] if direction == "dec" else
           bc.rec_combs(dims, pos, reach, level, cplx, pairs=True))
    out = []
    for band, v in ins:
        cols = [v * abs(bc.amplitude(k)) for k in range(columns)] if columns else [v]
        want = [_walk(direction, c, filt, level, l2, dil, hp) for c in cols]
        cond = [(bc.abs_dec(c, filt, level, l2, dil) if direction == "dec" else bc.abs_rec(c, filt, l2, dil, level)) for c in cols]
        if columns:                                              # dec: [n, columns, bands]; rec inputs: [n, columns, bands] -> [n, columns]
            v, want, cond = np.stack(cols, axis=1), np.stack(want, axis=1), np.stack(cond, axis=1)
        else:
            want, cond = want[0], cond[0]
        for a in (v, want, cond):
            a.setflags(write=False)
        out.append((band, v, want, cond))
    return out


# ---- running a case
def _dtypes(prec, cplx):
    if cplx:
        return (np.complex64, torch.complex64) if prec == "single" else (np.complex128, torch.complex128)
    return (np.float32, torch.float32) if prec == "single" else (np.float64, torch.float64)


class Guarded:
    """n elements on the device between GUARD elements of NaN on either side; `fill`: the flat contents, else NaN (an output)"""
    def __init__(self, n, tdt, fill=None):
        self.t = torch.full((n + 2 * GUARD,), float("nan"), dtype=tdt, device="cuda")
        self.view = self.t[GUARD:GUARD + n]
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)).cuda())

    def ptr(self):
        return self.view.data_ptr()

    def guards_untouched(self):
        g = torch.cat([self.t[:GUARD], self.t[-GUARD:]])
        return bool(torch.isnan(g.real if g.is_complex() else g).all())

    def numpy(self):
        return self.view.cpu().numpy()


def _to_kernel(a, c, ndt, bands):
    """an array of the reference's shape -> flat kernel order.  nd: [n1, .., nd(, bands)] -> (bands,) nd .. n1; a batch [n, K(, bands)] ->
    (bands,) K, n; interleaved samples [n, K * inner(, bands)] -> (bands,) K, n, inner"""
    if c["kind"] == "nd":
        return np.ascontiguousarray(np.transpose(a)).astype(ndt)
    n, K, inner = c["dims"][0], c["K"], c["inner"]
    a = a.reshape((n, K, inner) + ((a.shape[-1],) if bands else ()))
    return np.ascontiguousarray(np.moveaxis(a, -1, 0).transpose(0, 2, 1, 3) if bands else a.transpose(1, 0, 2)).astype(ndt)


def _from_kernel(flat, c, bands):
    if c["kind"] == "nd":
        return np.transpose(flat.reshape(([bands] if bands else []) + c["dims"][::-1]))
    n, K, inner = c["dims"][0], c["K"], c["inner"]
    if bands:
        return np.moveaxis(flat.reshape(bands, K, n, inner).transpose(0, 2, 1, 3).reshape(bands, n, K * inner), 0, -1)
    return flat.reshape(K, n, inner).transpose(1, 0, 2).reshape(n, K * inner)


def _plan(c):
    prec, cplx = c["prec"], c["cplx"]
    rdt = torch.float32 if prec == "single" else torch.float64
    kw = {"nd": {}, "batch": dict(howmany=c["K"]), "inter": dict(howmany=c["K"], inner=c["inner"])}[c["kind"]]
    plan = ndwt.Plan(c["dims"], c["wn"], rdt, cplx, bool(c["l2"]), c["dil"], max_level=c["level"], **kw)
    if c["chunk"]:
        plan.set_tuning(0, c["chunk"])
    if c["fwd"] >= 0 or c["inv"] >= 0:
        plan.set_variant(fwd=c["fwd"], inv=c["inv"])
    return plan


def run_case(c):
    cid, prec, cplx, level, l2, dil = c["id"], c["prec"], c["cplx"], c["level"], c["l2"], c["dil"]
    d = len(c["dims"])
    ndt, tdt = _dtypes(prec, cplx)
    u, hp = bc.U[prec], prec == "double"
    filt = bc.filters(c["wn"])
    cap = bc.cap(filt, level)
    columns = 0 if c["kind"] == "nd" else c["K"] * c["inner"]
    vol = int(np.prod(c["dims"])) * max(columns, 1)
    nb = orc.num_bands(d, level)
    key = (tuple(c["dims"]), tuple(c["wn"]), cplx, level, l2, dil)
    plan = _plan(c)
    stream = torch.cuda.current_stream().cuda_stream
    recs_all, worst = [], {}

    def note(recs, ratio):
        for r in recs:
            worst[r.family] = max(worst.get(r.family, 0.0), ratio)

    if c["dec"]:
        for m, (_, x, want, cond) in enumerate(reference("dec", *key, tuple(map(tuple, c["edges"])), hp, columns)):
            xb, yb = Guarded(vol, tdt, _to_kernel(x, c, ndt, False)), Guarded(nb * vol, tdt)
            with ndwt.kernel_trace() as recs:
                plan.dec(xb.ptr(), yb.ptr(), level, stream)
            torch.cuda.synchronize()
            check_trace(recs, c["dec"], f"dec {cid}")
            got = _from_kernel(yb.numpy(), c, nb)
            ratio = bc.check_componentwise(got, want, cond, cap, u, f"dec {cid} comb {m}")
            assert xb.guards_untouched() and yb.guards_untouched(), f"dec {cid}: a guard element was written"
            note(recs, ratio)
            recs_all += recs
    if c["rec"]:
        for m, (band, cf, want, cond) in enumerate(reference("rec", *key, tuple(map(tuple, c["redges"])), hp, columns)):
            cb, rb = Guarded(nb * vol, tdt, _to_kernel(cf, c, ndt, True)), Guarded(vol, tdt)
            with ndwt.kernel_trace() as recs:
                plan.rec(cb.ptr(), rb.ptr(), level, stream)
            torch.cuda.synchronize()
            check_trace(recs, c["rec"], f"rec {cid}")
            got = _from_kernel(rb.numpy(), c, 0)
            ratio = bc.check_componentwise(got, want, cond, cap, u, f"rec {cid} comb {m} in band {band}")
            assert cb.guards_untouched() and rb.guards_untouched(), f"rec {cid}: a guard element was written"
            note(recs, ratio)
            recs_all += recs
    if c["den"]:
        # thresholds 0: dec then rec in one launch is the identity.  want = x; cond = |W^-1| |W| |x|.  The synthesis half sums the low-pass and
        # the high-pass products of every level, all bands being non-zero now: 2 L + 2 per level instead of the L + 2 of a single band
        L = len(filt[0][0])
        cap_den = level * (L + 2) + level * (2 * L + 2)
        for m, (_, x, want, cond) in enumerate(reference("dec", *key, tuple(map(tuple, c["edges"])), hp, columns)):
            cond_x = np.stack([bc.abs_rec(cond[:, k], filt, l2, dil, level) for k in range(columns)], axis=1)
            xb, ob = Guarded(vol, tdt, _to_kernel(x, c, ndt, False)), Guarded(vol, tdt)
            with ndwt.kernel_trace() as recs:
                plan.denoise_bands(xb.ptr(), ob.ptr(), level, [0.0] * nb, False, stream)
            torch.cuda.synchronize()
            check_trace(recs, c["den"], f"denoise {cid}")
            got = _from_kernel(ob.numpy(), c, 0)
            ratio = bc.check_componentwise(got, x, cond_x, cap_den, u, f"denoise {cid} comb {m}")
            assert xb.guards_untouched() and ob.guards_untouched(), f"denoise {cid}: a guard element was written"
            note(recs, ratio)
            recs_all += recs
    print(f"[small-taps] {cid}: {c['dims']} {'.'.join(w[2:] for w in c['wn'])} {prec}{' complex' if cplx else ''} L{level} l2={l2} {dil}: worst "
          + ", ".join(f"{f} {r:.3g}" for f, r in sorted(worst.items())) + f" u cond (cap {cap})")
    RATIOS[cid], _RECS[cid] = worst, recs_all
    return recs_all


@pytest.mark.parametrize("c", CASES)
def test_small_taps(c):
    try:
        run_case(c)
    except AssertionError:
        raise
    except Exception as e:                                       # a device or library error: launch nothing more on a device that may have faulted
        pytest.exit(f"{c['id']}: {type(e).__name__}: {e}", returncode=3)


# ---- coverage: the instance lists, spelled as the trace spells a launch
@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("list")), "liblist_shim.so")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "select", "list_shim.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", src, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.list_instances.restype = ctypes.c_char_p
    return lib.list_instances().decode().splitlines()


def long_float_instances(lines):
    sps = [(s, spec(s)) for s in lines]
    return [(s, sp) for s, sp in sps if sp[1]["T"] == "float" and sp[1]["L"] >= 10]


def test_every_listed_long_instance_ran(listed):
    """every float instance of 10 taps or more that csrc/ndwt_fused_list.h lists was launched by a case above that passed (a case that
    has not run yet, as under -k, is run here).  Nothing is exempt: the list of unreachable instances is empty."""
    want = long_float_instances(listed)
    assert len(want) == 166, len(want)                           # 39 Fwd3, 12 Inv3S, 42 Inv3Y, 40 Fwd2S / Inv2S, 4 Inv2P, 1 Fwd2C, 12 AxisMarch, 16 AxisX
    for p in CASES:
        c = p.values[0]
        if c["id"] not in _RECS and c["prec"] == "single":
            try:
                run_case(c)
            except AssertionError:
                pass                                             # its own test reports it; its instance counts as missing here
    recs = [r for rs in _RECS.values() for r in rs]
    missing = [s for s, sp in want if not any(matches(r, sp) for r in recs)]
    assert not missing, f"{len(missing)} listed instances ran in no passing case:\n  " + "\n  ".join(missing)


def test_worst_ratios_per_family():
    """the record for DESIGN.md: the worst ratio of every family over the cases that passed (printed; the cases assert the derived cap)"""
    fam = {}
    for cid, w in RATIOS.items():
        prec = "double" if cid.startswith(("f64", "c128")) else "single"
        for f, r in w.items():
            fam[(f, prec)] = max(fam.get((f, prec), 0.0), r)
    for (f, prec), r in sorted(fam.items()):
        print(f"[small-taps] worst {f} ({prec}): {r:.3g} u cond")
    assert fam or not RATIOS
