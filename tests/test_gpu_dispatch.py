"""Every branch of the kernel dispatcher, pinned: each row names the kernels a call must launch (read from the library's launch trace,
include/ndwt.h: ndwt_trace_enable) and checks that call against the fp64 oracle.

The shapes sit on both sides of the dispatcher's thresholds (csrc/ndwt_select.h: fused3_select, fused2_select, cascade2_levels and the
eligibility predicates; ndwt_denoise in csrc/ndwt_api.hip):
if dispatch moves, the trace assertion of the row fails and names what ran instead.  The oracle is oracle/ndwt_spatial.c (signal-domain
C restatement of the transform, computed in double on the input rounded to the device precision).
"""
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
import ndwt_spatial as orc_c
import helpers
from helpers import COVERAGE, check_trace, matches

pytestmark = pytest.mark.gpu

TOL = {"single": 2e-6, "double": 1e-12}


def R(rid, dims, wn, prec="single", cplx=False, dil="reference", level=1, layout="packed", fwd=-1, inv=-1, path=None, dec=(), rec=(),
      den=None, fused_level1=None, chunk=None):
    return pytest.param(dict(dims=dims, wn=wn, prec=prec, cplx=cplx, dil=dil, level=level, layout=layout, fwd=fwd, inv=inv, path=path,
                             dec=list(dec), rec=list(rec), den=den, fused_level1=fused_level1, chunk=chunk), id=rid)


# ---- the rows.  Each comment gives the threshold and the arithmetic that puts the row on its side of it.
ROWS = [
    # float analysis, 6 / 8 taps: the tall 64x32 tile once ceil(n1/64) * ceil(n2/32) * nbatch >= 32 (n1 in scalars)
    R("tall-tile-32", [256, 256, 12], "db4", dec=["Fwd3 L=8 TY=32 NT=1024 VEC4=true PIN=false"],
      rec=["Inv3Y L=8 XSC=false VEC4=true DEPTH=2 UNIYZ=false"]),                                  # 4 * 8 = 32
    R("tall-tile-28", [256, 224, 12], "db4", dec=["Fwd3 L=8 TY=16 NT=256 VEC4=true"],
      rec=["Inv3Y L=8 XSC=false VEC4=true"]),                                                      # 4 * 7 = 28
    R("tall-tile-c64-32", [128, 256, 12], "db4", cplx=True, dec=["Fwd3 L=8 EW=2 TY=32 NT=1024"],
      rec=["Inv3Y L=8 EW=2 XSC=false VEC4=true"]),                                                 # 256 scalars: 4 * 8 = 32
    R("tall-tile-c64-28", [128, 224, 12], "db4", cplx=True, dec=["Fwd3 L=8 EW=2 TY=16 NT=256"],
      rec=["Inv3Y L=8 EW=2 XSC=false VEC4=true"]),                                                 # 4 * 7 = 28
    R("tall-tile-4d-frames-32", [128, 64, 8, 8], "db4", dec=["Fwd3 L=8 TY=32 NT=1024", "AxisMarch L=8 SYN=false"],
      rec=["Inv3Y L=8 XSC=false", "AxisMarch L=8 SYN=true"], den=["Fwd3 L=8 TY=32", "AxisMarch L=8", "Inv3Y L=8 XSC=false"]),   # 2 * 2 * 8 frames = 32
    R("tall-tile-4d-frames-16", [128, 32, 8, 8], "db4", dec=["Fwd3 L=8 TY=16 NT=256", "AxisMarch L=8 SYN=false"],
      rec=["Inv3Y L=8 XSC=false", "AxisMarch L=8 SYN=true"]),                                      # 2 * 1 * 8 = 16
    # Fwd3 PIN: 10 .. 14 taps, vec4 data, even zero padding of every axis' taps
    R("pin-db5", [64, 40, 36], "db5", level=2, dec=["Fwd3 L=10 PIN=true TY=32"], rec=["Inv3Y L=10 XSC=true UNIYZ=false DEPTH=2"],
      den=["Fwd3 L=10 PIN=true", "Inv3Y L=10 XSC=true"]),
    R("pin-db6", [64, 40, 36], "db6", dec=["Fwd3 L=12 PIN=true TY=32"], rec=["Inv3Y L=12 XSC=true UNIYZ=true DEPTH=2 ZLDS=6"]),
    R("pin-db7", [64, 40, 36], "db7", dec=["Fwd3 L=14 PIN=true TY=32"], rec=["Inv3Y L=14 XSC=true UNIYZ=true DEPTH=1"]),
    R("pin-even-mixed", [64, 40, 36], ["db6", "db4", "db6"], dec=["Fwd3 L=12 PIN=true"], rec=["Inv3Y L=12 XSC=true UNIYZ=false"]),
    R("nopin-odd-padding", [64, 40, 36], ["db5", "db4", "db5"], dec=["Fwd3 L=10 PIN=false TY=32 VEC4=true"],
      rec=["Inv3S L=10 TY=32 NT=1024 VEC4=true"], den=["Fwd3 L=10 PIN=false", "Inv3S L=10"]),      # (10 - 8) / 2 = 1: no derived high-pass taps
    R("nopin-n1-70", [70, 40, 36], "db5", dec=["Fwd3 L=10 PIN=false VEC4=false"], rec=["Inv3Y L=10 XSC=false VEC4=false DEPTH=1"]),
    R("nopin-offset", [64, 40, 36], "db5", layout="offset", dec=["Fwd3 L=10 PIN=false VEC4=false"],
      rec=["Inv3Y L=10 XSC=false VEC4=false"]),
    R("pitch-not-mult-4", [64, 40, 36], "db4", layout="pitch", dec=["Fwd3 L=8 VEC4=false"], rec=["Inv3Y L=8 VEC4=false"]),
    # pair-packed synthesis: gather form <= 8 taps, scatter form 10 .. 20 taps on vec4 rows, gather form on rows that are not
    R("inv3y-gather-8", [64, 40, 36], "db4", level=2, dec=["Fwd3 L=8 TY=16"], rec=["Inv3Y L=8 XSC=false VEC4=true DEPTH=2"],
      den=["Fwd3 L=8", "Inv3Y L=8 XSC=false"]),
    R("inv3y-scatter-16", [64, 40, 36], "db8", dec=["Fwd3 L=16 WLDS=2 TY=32 VEC4=true"], rec=["Inv3Y L=16 XSC=true UNIYZ=true"],
      den=["Fwd3 L=16 WLDS=2", "Inv3Y L=16 XSC=true"]),
    R("inv3y-scatter-18", [64, 48, 32], "db9", dec=["Fwd3 L=18 WLDS=0 TY=16 NT=512 VEC4=true"],
      rec=["Inv3Y L=18 XSC=true TY=24 UNIYZ=true"]),
    R("inv3y-scatter-20", [64, 40, 36], "db10", dec=["Fwd3 L=20 WLDS=4 VEC4=true"], rec=["Inv3Y L=20 TX=48 TY=28 XSC=true UNIYZ=true"],
      den=["Fwd3 L=20 WLDS=4", "shrink_kernel T=float", "Inv3Y L=20 XSC=true"]),   # (18 / 20 taps: no fused shrink -- fused_shrink_capable)
    R("inv3y-gather-20-ragged", [70, 37, 33], "db10", dec=["Fwd3 L=20 WLDS=6 VEC4=false"], rec=["Inv3Y L=20 TX=48 XSC=false VEC4=false"]),
    R("inv3y-gather-18-ragged", [70, 37, 33], "db9", dec=["Fwd3 L=18 WLDS=2 VEC4=false"], rec=["Inv3Y L=18 XSC=false VEC4=false"]),
    R("inv3y-uniyz-false", [72, 36, 30], ["db6", "db6", "db4"], dec=["Fwd3 L=12 PIN=true"], rec=["Inv3Y L=12 XSC=true UNIYZ=false"]),
    R("inv3s-odd-16", [64, 40, 36], ["db8", "db7", "db7"], dec=["Fwd3 L=16 WLDS=2"], rec=["Inv3S L=16 TY=32 NT=512"],
      den=["Fwd3 L=16", "Inv3S L=16"]),                                                            # (16 - 14) / 2 = 1
    R("inv3s-odd-14", [64, 40, 36], ["db7", "db6", "db6"], dec=["Fwd3 L=14 PIN=false TY=32 RY=2"], rec=["Inv3S L=14 TY=32 NT=512"]),
    # interleaved complex synthesis: Inv3Y EW = 2, scatter form from 10 taps; complex128 fused to 10 taps, 12 in the analysis only
    R("c64-db4", [32, 24, 20], "db4", cplx=True, level=2, dec=["Fwd3 L=8 EW=2 TY=16"], rec=["Inv3Y L=8 EW=2 XSC=false"],
      den=["Fwd3 L=8 EW=2", "Inv3Y L=8 EW=2 XSC=false"]),
    R("c64-db5", [32, 24, 20], "db5", cplx=True, dec=["Fwd3 L=10 EW=2 NT=512"], rec=["Inv3Y L=10 EW=2 XSC=true"],
      den=["Fwd3 L=10 EW=2", "Inv3Y L=10 EW=2 XSC=true"]),
    R("c64-db6", [32, 24, 20], "db6", cplx=True, dec=["Fwd3 L=12 EW=2"], rec=["Inv3Y L=12 EW=2 XSC=true TX=48"]),
    R("c128-db5", [32, 24, 20], "db5", prec="double", cplx=True, dec=["Fwd3 T=double L=10 EW=2 TY=8 NT=512"],
      rec=["Inv3S T=double L=10 EW=2 TY=8 NT=512"], den=["Fwd3 T=double L=10 EW=2", "Inv3S T=double L=10 EW=2"]),
    R("c128-db6", [32, 24, 20], "db6", prec="double", cplx=True, dec=["Fwd3 T=double L=12 EW=2 WLDS=2"],
      rec=["axis_synthesis_kernel T=double", "AxisMarch T=double L=12 SYN=true"]),   # x: 64 scalars < 8 * 12 -> no AxisX
    # dilated (a trous) levels: stride 2 -> EW = 2, stride 4 -> EW = 4 (float, 16-byte aligned), per-axis where a dim does not divide
    R("atrous-db2-l3", [32, 24, 16], "db2", dil="atrous", level=3, dec=["Fwd3 L=4 EW=1", "Fwd3 L=4 EW=2", "Fwd3 L=4 EW=4"],
      rec=["Inv3Y L=4 EW=1", "Inv3Y L=4 EW=2 XSC=false", "Inv3Y L=4 EW=4 XSC=false"],
      den=["Fwd3 L=4", "Inv3Y L=4", "shrink_kernel T=float COMP=1"]),
    R("atrous-db4-l3", [32, 32, 32], "db4", dil="atrous", level=3, dec=["Fwd3 L=8 EW=1", "Fwd3 L=8 EW=2", "Fwd3 L=8 EW=4"],
      rec=["Inv3Y L=8 EW=1", "Inv3Y L=8 EW=2 XSC=false", "Inv3Y L=8 EW=4 XSC=true DEPTH=2"]),
    R("atrous-db4-l3-offset", [32, 32, 32], "db4", dil="atrous", level=3, layout="offset",
      dec=["Fwd3 L=8 EW=1 VEC4=false", "Fwd3 L=8 EW=2 VEC4=false", "Fwd3 L=8 EW=4 VEC4=false"],
      rec=["Inv3Y L=8 EW=1 VEC4=false", "Inv3Y L=8 EW=2 VEC4=false", "Inv3S L=8 EW=4 VEC4=false"]),
    R("atrous-indivisible", [32, 24, 18], "db2", dil="atrous", level=3,
      dec=["Fwd3 L=4 EW=1", "Fwd3 L=4 EW=2", "AxisMarch L=4 SYN=false", "axis_analysis_kernel T=float"],
      rec=["Inv3Y L=4 EW=1", "Inv3Y L=4 EW=2", "AxisMarch L=4 SYN=true", "axis_synthesis_kernel T=float"]),   # 18 % 4 != 0
    R("atrous-2d-l3", [72, 40], ["db4", "db2"], dil="atrous", level=3, dec=["Fwd2S L=8 EW=1", "Fwd2S L=8 EW=2", "Fwd2S L=8 EW=4"],
      rec=["Inv2S L=8 EW=1", "Inv2S L=8 EW=2", "Inv2S L=8 EW=4"]),
    R("atrous-2d-f64", [72, 40], ["db4", "db2"], prec="double", dil="atrous", level=2,                # double: EW = 2 is its only dilated form
      dec=["Fwd2S T=double L=8 EW=1 WPE=2", "Fwd2S T=double L=8 EW=2 WPE=2"], rec=["Inv2S T=double L=8 EW=1 WPE=2", "Inv2S T=double L=8 EW=2 WPE=2"]),
    # fp64 3-D
    R("f64-db3", [64, 40, 36], "db3", prec="double", dec=["Fwd3 T=double L=6 TY=16 NT=512"], rec=["Inv3S T=double L=6 TY=16 NT=512"]),
    R("f64-db4", [64, 40, 36], "db4", prec="double", level=2, dec=["Fwd3 T=double L=8 TY=16 NT=512"],
      rec=["Inv3S T=double L=8 TY=16 NT=512"], den=["Fwd3 T=double L=8", "Inv3S T=double L=8"]),
    R("f64-db5", [64, 40, 36], "db5", prec="double", dec=["Fwd3 T=double L=10 TY=16 NT=512"], rec=["Inv3S T=double L=10 TY=8 NT=512"]),
    R("f64-db6", [68, 41, 30], "db6", prec="double", dec=["Fwd3 T=double L=12 TY=8 NT=512"], rec=["Inv3S T=double L=12 TY=8 NT=512"]),
    R("f64-db7", [64, 40, 36], "db7", prec="double", dec=["Fwd3 T=double L=14 TY=8 NT=512 WLDS=0"], rec=["Inv3S T=double L=14 TY=8"]),
    R("f64-db8", [64, 40, 36], "db8", prec="double", dec=["Fwd3 T=double L=16 WLDS=2"], rec=["Inv3S T=double L=16 TY=8"],
      den=["Fwd3 T=double L=16", "Inv3S T=double L=16"]),
    R("f64-db9-per-axis", [64, 40, 36], "db9", prec="double", dec=["axis_analysis_kernel T=double", "AxisMarch T=double L=18 SYN=false"],
      rec=["axis_synthesis_kernel T=double", "AxisMarch T=double L=18 SYN=true"]),
    # 2-D synthesis: Inv2P (depth 4, packed) for n2 >= 64 and tiles2 * ceil(n2 / 70) <= 1280, else Inv2S
    R("inv2p-n2-64", [256, 64], "db4", dec=["Fwd2S L=8 VEC4=true"], rec=["Inv2P L=8 PD=4 PK=true"], den=["Fwd2S L=8", "Inv2P L=8"]),
    R("inv2s-n2-63", [256, 63], "db4", dec=["Fwd2S L=8 VEC4=true"], rec=["Inv2S L=8 VEC4=true WPE=4"], den=["Fwd2S L=8", "Inv2S L=8"]),
    R("inv2p-budget-5250", [4096, 5250], "db4", dec=["Fwd2S L=8"], rec=["Inv2P L=8 PD=4 PK=true"]),   # 17 tiles * 75 chunks = 1275
    R("inv2s-budget-5251", [4096, 5251], "db4", dec=["Fwd2S L=8"], rec=["Inv2S L=8 VEC4=true"]),      # 17 * 76 = 1292
    R("2d-db3-short", [260, 96], "db3", dec=["Fwd2S L=6 VEC4=true"], rec=["Inv2P L=6 PD=2 PK=false"]),   # (packed depth 4: 4 / 8 / 12 taps)
    R("2d-db7-long", [260, 96], "db7", dec=["Fwd2S L=14 VEC4=true WPE=2"], rec=["Inv2S L=14 VEC4=true WPE=2"],
      den=["Fwd2S L=14", "Inv2S L=14"]),                                                           # (14 .. 20 taps: the 256-register budget)
    R("2d-db10-long", [512, 70], "db10", dec=["Fwd2S L=20"], rec=["Inv2S L=20"]),
    R("2d-db9-ragged", [250, 65], "db9", dec=["Fwd2S L=18 VEC4=false"], rec=["Inv2S L=18 VEC4=false"]),
    R("2d-c64-db5", [128, 70], "db5", cplx=True, dec=["Fwd2S L=10 EW=2 WPE=2"], rec=["Inv2S L=10 EW=2 WPE=2"],
      den=["Fwd2S L=10 EW=2", "Inv2S L=10 EW=2"]),
    R("2d-c64-db8", [128, 70], "db8", cplx=True, dec=["Fwd2S L=16 EW=2"], rec=["Inv2S L=16 EW=2"]),
    R("2d-f64-db8", [260, 96], "db8", prec="double", dec=["Fwd2S T=double L=16"], rec=["Inv2S T=double L=16"]),
    R("2d-f64-db4", [260, 96], "db4", prec="double", dec=["Fwd2S T=double L=8"], rec=["Inv2P T=double L=8"],
      den=["Fwd2S T=double L=8", "Inv2P T=double L=8"]),
    # complex128: fused up to 8 taps (one ragged wave tile of 128 scalars, 70 rows in chunks), the per-axis passes beyond
    R("2d-c128-db4", [64, 70], "db4", prec="double", cplx=True, dec=["Fwd2S T=double L=8 EW=2 WPE=2"], rec=["Inv2S T=double L=8 EW=2 WPE=2"]),
    R("2d-c128-db5-per-axis", [64, 70], "db5", prec="double", cplx=True,
      dec=["AxisMarch T=double L=10 SYN=false", "AxisX T=double L=10 SYN=false EW=2"],
      rec=["AxisMarch T=double L=10 SYN=true", "AxisX T=double L=10 SYN=true EW=2"]),
    # 2-D cascade: vol > 6 << 20 (= 2048 * 3072), level >= 2, n1 % 4 == 0, Lp <= 8 or 12
    R("cascade-off-6M", [2048, 3072], "db4", level=3, dec=["Fwd2S L=8"], rec=["Inv2P L=8 PD=4"]),
    R("cascade-db4-l3", [2048, 3073], "db4", level=3, dec=["Fwd2C L=8 NLEV=3"], rec=["Inv2C L=8 NLEV=3 PD=1"],
      den=["Fwd2C L=8 NLEV=3", "Inv2C L=8 NLEV=3"]),
    R("cascade-db4-l4", [2048, 3073], "db4", level=4, dec=["Fwd2C L=8 NLEV=3", "Fwd2S L=8"], rec=["Inv2C L=8 NLEV=3", "Inv2P L=8"]),
    R("cascade-db6-l3", [2048, 3073], "db6", level=3, dec=["Fwd2C L=12 NLEV=2", "Fwd2S L=12"], rec=["Inv2P L=12"]),
    R("cascade-db5-ineligible", [2048, 3073], "db5", level=3, dec=["Fwd2S L=10"], rec=["Inv2P L=10"]),
    R("cascade-n1-not-mult-4", [2050, 3073], "db4", level=3, dec=["Fwd2S L=8 VEC4=false"], rec=["Inv2S L=8 VEC4=false"]),
    # denoise: Den3 on disjoint aligned buffers (fused_level1 1: up to 6 taps), the materialising path otherwise
    R("den3-db2", [64, 40, 36], "db2", level=2, dec=["Fwd3 L=4"], rec=["Inv3Y L=4"],
      den=["Fwd3 L=4 LOWONLY=true", "Den3 L=4", "Fwd3 L=4 LOWONLY=false", "Inv3Y L=4"]),
    R("den3-db2-offset", [64, 40, 36], "db2", level=2, layout="offset", dec=["Fwd3 L=4 VEC4=false"], rec=["Inv3Y L=4 VEC4=false"],
      den=["Fwd3 L=4 LOWONLY=false", "Inv3Y L=4"]),
    R("den-4d", [24, 20, 12, 16], "db2", level=1, dec=["Fwd3 L=4", "AxisMarch L=4 SYN=false"], rec=["Inv3Y L=4", "AxisMarch L=4 SYN=true"],
      den=["Fwd3 L=4", "AxisMarch L=4", "Inv3Y L=4"]),
    # per-axis kernels
    R("1d-vec4", [4096], "db2", dec=["AxisX L=4 SYN=false VEC4=true EW=1"], rec=["AxisX L=4 SYN=true VEC4=true"],
      den=["AxisX L=4", "shrink_kernel"]),
    R("1d-ragged", [4098], "db2", layout="offset", dec=["AxisX L=4 SYN=false VEC4=false"], rec=["AxisX L=4 SYN=true VEC4=false"]),
    R("1d-c64", [1024], "db3", cplx=True, dec=["AxisX L=6 SYN=false EW=2"], rec=["AxisX L=6 SYN=true EW=2"]),
    R("1d-db7-plain", [4096], "db7", prec="double", dec=["axis_analysis_kernel T=double"], rec=["axis_synthesis_kernel T=double"]),
    R("generic-path", [64, 40, 36], "db2", path=True, dec=["axis_analysis_kernel T=float"], rec=["axis_synthesis_kernel T=float"],
      den=["axis_analysis_kernel", "axis_synthesis_kernel", "shrink_kernel"]),
    # A/B variants of Plan.set_variant: what their comments in csrc/ndwt_api.hip promise
    R("fwd3-keeps-64x16", [256, 256, 12], "db4", fwd=3, dec=["Fwd3 L=8 TY=16 NT=256"], rec=["Inv3Y L=8"]),
    R("inv3-lds-kernel", [64, 40, 36], "db4", inv=3, dec=["Fwd3 L=8"], rec=["Inv3 L=8 TY=16"], den=["Fwd3 L=8", "Inv3 L=8", "shrink_kernel"]),
    R("inv4-lane-shift", [64, 40, 36], "db4", inv=4, dec=["Fwd3 L=8"], rec=["Inv3S L=8 TY=32 NT=1024"], den=["Fwd3 L=8", "Inv3S L=8"]),
    R("fwd7-folded-t", [24, 20, 12, 16], "db2", fwd=7, dec=["Fwd3 L=4 TPRE=true"], rec=["Inv3Y L=4", "AxisMarch L=4 SYN=true"]),
    R("fwd8-no-pin", [64, 40, 36], "db5", fwd=8, dec=["Fwd3 L=10 PIN=false TY=32"], rec=["Inv3Y L=10 XSC=true"]),
    R("fwd9-inv9-cascade-off", [2048, 3073], "db4", level=3, fwd=9, inv=9, dec=["Fwd2S L=8"], rec=["Inv2P L=8"]),
    R("inv10-scatter-8", [64, 40, 36], "db4", inv=10, dec=["Fwd3 L=8"], rec=["Inv3Y L=8 XSC=true"]),
    R("inv11-gather-12", [64, 40, 36], "db6", inv=11, dec=["Fwd3 L=12 PIN=true"], rec=["Inv3Y L=12 XSC=false UNIYZ=true"]),
    R("inv9-3d-uniyz-off", [64, 40, 36], "db6", inv=9, dec=["Fwd3 L=12"], rec=["Inv3Y L=12 XSC=true UNIYZ=true"]),
    R("fwd11-inv11-small-cascade", [256, 96], "db4", level=3, fwd=11, inv=11, dec=["Fwd2C L=8 NLEV=3"], rec=["Inv2C L=8 NLEV=3 PD=1"]),
    R("fwd10-inv12-small-cascade", [256, 96], "db3", level=2, fwd=10, inv=12, dec=["Fwd2C L=6 NLEV=2"], rec=["Inv2C L=6 NLEV=2 PD=2"]),
    R("fwd11-db6-cascade-2lev", [256, 96], "db6", level=3, fwd=11, dec=["Fwd2C L=12 NLEV=2", "Fwd2S L=12"], rec=["Inv2P L=12"]),
    R("inv7-inv2p-scalar", [256, 64], "db4", inv=7, dec=["Fwd2S L=8"], rec=["Inv2P L=8 PK=false"]),
    # ... and the instance each 3-D number names where the default would run another one (the other direction stays the default's)
    R("fwd1-db7-one-column", [64, 40, 36], "db7", fwd=1, dec=["Fwd3 L=14 TY=16 NT=512 WLDS=0 PIN=false"],
      rec=["Inv3Y L=14 XSC=true UNIYZ=true DEPTH=1"]),
    R("fwd1-db8-one-column", [64, 40, 36], "db8", fwd=1, dec=["Fwd3 L=16 TY=16 NT=512 WLDS=0"], rec=["Inv3Y L=16 XSC=true UNIYZ=true"]),
    R("fwd3-db8-no-window-slots", [64, 40, 36], "db8", fwd=3, dec=["Fwd3 L=16 TY=32 NT=1024 RY=2 WLDS=0"],
      rec=["Inv3Y L=16 XSC=true UNIYZ=true"]),
    R("fwd3-db10-no-window-slots", [64, 40, 36], "db10", fwd=3, dec=["Fwd3 L=20 TY=16 NT=512 WLDS=0"],
      rec=["Inv3Y L=20 TX=48 TY=28 XSC=true UNIYZ=true"]),
    R("fwd1-db5-one-column", [64, 40, 36], "db5", fwd=1, dec=["Fwd3 L=10 TY=16 NT=512 PIN=false"],
      rec=["Inv3Y L=10 XSC=true UNIYZ=false DEPTH=2"]),
    R("fwd2-db2-tall", [64, 40, 36], "db2", fwd=2, dec=["Fwd3 L=4 TY=32 NT=1024 RY=4"], rec=["Inv3Y L=4"]),
    R("fwd6-db4-tall-ry2", [64, 40, 36], "db4", fwd=6, dec=["Fwd3 L=8 TY=32 RY=2"], rec=["Inv3Y L=8 XSC=false VEC4=true DEPTH=2"]),
    R("inv5-db4-depth1", [64, 40, 36], "db4", inv=5, dec=["Fwd3 L=8 TY=16"], rec=["Inv3Y L=8 DEPTH=1"]),
    R("inv2-atrous-keeps-inv3s", [32, 32, 32], "db4", dil="atrous", level=3, inv=2, dec=["Fwd3 L=8 EW=1", "Fwd3 L=8 EW=2", "Fwd3 L=8 EW=4"],
      rec=["Inv3Y L=8 EW=1", "Inv3S L=8 EW=2", "Inv3S L=8 EW=4"]),
    R("fwd1-f64-db3-one-column", [64, 40, 36], "db3", prec="double", fwd=1, dec=["Fwd3 T=double L=6 TY=16 NT=512"],
      rec=["Inv3S T=double L=6 TY=16 NT=512"]),
    R("fwd3-f64-db3-small-tile", [64, 40, 36], "db3", prec="double", fwd=3, dec=["Fwd3 T=double L=6 TY=8 NT=256"],
      rec=["Inv3S T=double L=6 TY=16 NT=512"]),
]


def _np_soft(c, t):
    m = np.abs(c)
    out = c * np.where(m > t, (m - t) / np.where(m > 0, m, 1.0), 0.0)
    out[..., 0] = c[..., 0]                                  # the coarsest approximation band is kept
    return out


def _dtypes(prec, cplx):
    real = np.float32 if prec == "single" else np.float64
    if not cplx:
        return real, (torch.float32 if prec == "single" else torch.float64)
    return (np.complex64 if prec == "single" else np.complex128), (torch.complex64 if prec == "single" else torch.complex128)


class _Buf:
    """a device buffer of n elements of the row's layout: packed, one element off 16 bytes, or bands at a pitch that is no multiple of 4"""
    def __init__(self, n, tdt, off):
        self.t = torch.zeros(n + 8, dtype=tdt, device="cuda")
        self.off, self.n = off, n
        self.view = self.t[off:off + n]

    def ptr(self):
        return self.view.data_ptr()


def run_row(row, trace_check=True):
    """dec, rec of random coefficients, round trip and (if the row asks) soft denoise, against the oracle; returns all launch records"""
    dims, wn, prec, cplx, dil, level = row["dims"], row["wn"], row["prec"], row["cplx"], row["dil"], row["level"]
    d = len(dims)
    wl = [wn] * d if isinstance(wn, str) else wn
    ndt, tdt = _dtypes(prec, cplx)
    tol = TOL[prec]
    rng = np.random.default_rng(zlib.crc32(repr((dims, wn, prec, cplx, dil, level)).encode()))
    x = rng.standard_normal(dims) + (1j * rng.standard_normal(dims) if cplx else 0)
    x = x.astype(ndt).astype(np.complex128 if cplx else np.float64)   # the oracle sees the input the device sees
    nb = ndwt.num_bands(d, level)
    vol = int(np.prod(dims))
    off = 1 if row["layout"] == "offset" else 0
    pitch = vol + (1 if vol % 4 == 0 else 0) + (2 if vol % 4 in (1, 3) else 0) if row["layout"] == "pitch" else vol
    assert row["layout"] != "pitch" or pitch % 4 != 0
    plan = ndwt.Plan(dims, wl, torch.float32 if prec == "single" else torch.float64, cplx, True, dil, max_level=level)
    if row.get("chunk"):                                     # planes (rows) every workgroup of a fused launch marches: tests/test_gpu_long_march.py
        plan.set_tuning(0, row["chunk"])
    if row["path"]:
        plan.set_path(True)
    if row["fwd"] >= 0 or row["inv"] >= 0:
        plan.set_variant(fwd=row["fwd"], inv=row["inv"])
    if row["fused_level1"] is not None:
        plan.set_fused_level1(row["fused_level1"])
    stream = torch.cuda.current_stream().cuda_stream
    what = f"{dims} {wn} {prec}{' complex' if cplx else ''} {dil} L{level} {row['layout']}"
    allrecs = []

    def to_kernel(a):                                        # MATLAB shape -> flat kernel order (x fastest)
        return torch.from_numpy(np.ascontiguousarray(np.transpose(a)).astype(ndt).reshape(-1))

    def coef_to_buf(c):
        ck = np.ascontiguousarray(np.transpose(c)).astype(ndt).reshape(nb, vol)      # (bands, vol)
        b = _Buf(nb * pitch, tdt, off)
        v = b.view.reshape(-1)
        for k in range(nb):
            v[k * pitch:k * pitch + vol] = torch.from_numpy(ck[k]).cuda()
        return b

    def buf_to_coef(b):
        v = b.view.reshape(-1)
        ck = torch.stack([v[k * pitch:k * pitch + vol] for k in range(nb)]).cpu().numpy().reshape([nb] + dims[::-1])
        return np.transpose(ck)

    # dec
    xb = _Buf(vol, tdt, off)
    xb.view.copy_(to_kernel(x).cuda())
    yb = _Buf(nb * pitch, tdt, off)
    with ndwt.kernel_trace() as recs:
        plan.dec(xb.ptr(), yb.ptr(), level, stream, band_pitch=0 if pitch == vol else pitch)
    torch.cuda.synchronize()
    allrecs += recs
    if trace_check:
        check_trace(recs, row["dec"], f"dec {what}")
    want = orc_c.spatial_dec(x, wl, level, 1, dil)
    y = buf_to_coef(yb)
    err = np.abs(y - want).max() / np.abs(want).max()
    assert err <= tol, (what, "dec", err)
    # rec of random coefficients
    c = rng.standard_normal(want.shape) + (1j * rng.standard_normal(want.shape) if cplx else 0)
    c = c.astype(ndt).astype(want.dtype)
    cb = coef_to_buf(c)
    rb = _Buf(vol, tdt, off)
    with ndwt.kernel_trace() as recs:
        plan.rec(cb.ptr(), rb.ptr(), level, stream, band_pitch=0 if pitch == vol else pitch)
    torch.cuda.synchronize()
    allrecs += recs
    if trace_check:
        check_trace(recs, row["rec"], f"rec {what}")
    got = np.transpose(rb.view.cpu().numpy().reshape(dims[::-1]))
    want_r = orc_c.spatial_rec(c, wl, 1, dil)
    err = np.abs(got - want_r).max() / max(np.abs(want_r).max(), np.abs(c).max())
    assert err <= 4 * tol, (what, "rec", err)
    assert float(rb.t[:off].abs().sum()) == 0 and float(rb.t[off + vol:].abs().sum()) == 0     # nothing written outside the output
    # round trip
    plan.rec(yb.ptr(), rb.ptr(), level, stream, band_pitch=0 if pitch == vol else pitch)
    torch.cuda.synchronize()
    back = np.transpose(rb.view.cpu().numpy().reshape(dims[::-1]))
    err = np.abs(back - x).max() / np.abs(x).max()
    assert err <= 20 * tol, (what, "round trip", err)
    # soft denoise: oracle dec -> numpy soft threshold of the detail bands -> oracle rec
    if row["den"] is not None:
        thr = float(np.median(np.abs(want[..., 1:])))
        ob = _Buf(vol, tdt, off)
        with ndwt.kernel_trace() as recs:
            plan.denoise(xb.ptr(), ob.ptr(), level, thr, False, stream)
        torch.cuda.synchronize()
        allrecs += recs
        if trace_check:
            check_trace(recs, row["den"], f"denoise {what}")
        got = np.transpose(ob.view.cpu().numpy().reshape(dims[::-1]))
        want_x = orc_c.spatial_rec(_np_soft(want, thr), wl, 1, dil)
        err = np.abs(got - want_x).max() / max(np.abs(want_x).max(), 1.0)
        assert err <= 20 * tol, (what, "denoise", err)
    return allrecs


@pytest.mark.parametrize("row", ROWS)
def test_dispatch_row(row):
    run_row(row)


def test_denoise_in_place_takes_the_materialising_path():
    """Den3 reads x around every output voxel while other workgroups write the output: an in-place denoise must not take it"""
    dims, wn, level, thr = [64, 40, 36], "db2", 2, 0.3
    rng = np.random.default_rng(3)
    x = rng.standard_normal(dims).astype(np.float32).astype(np.float64)
    plan = ndwt.Plan(dims, [wn] * 3, torch.float32, False, True, "reference", max_level=level)
    xt = torch.from_numpy(np.ascontiguousarray(x.T).astype(np.float32)).cuda().reshape(-1)
    with ndwt.kernel_trace() as recs:
        plan.denoise(xt.data_ptr(), xt.data_ptr(), level, thr, False, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check_trace(recs, ["Fwd3 L=4 LOWONLY=false", "Inv3Y L=4"], "in-place denoise")
    want = orc_c.spatial_dec(x, [wn] * 3, level, 1)
    want_x = orc_c.spatial_rec(_np_soft(want, thr), [wn] * 3, 1)
    got = np.transpose(xt.cpu().numpy().reshape(dims[::-1]))
    assert np.abs(got - want_x).max() <= 20 * TOL["single"] * max(np.abs(want_x).max(), 1.0)


def test_trace_is_host_side_and_changes_no_result():
    """the same call with and without the trace: the same bits; the trace off records nothing"""
    plan = ndwt.Plan([64, 40, 36], ["db4"] * 3, torch.float32, False, True, "reference", max_level=2)
    x = torch.randn(36 * 40 * 64, device="cuda")
    y0 = torch.empty(ndwt.num_bands(3, 2) * x.numel(), device="cuda")
    y1 = torch.empty_like(y0)
    s = torch.cuda.current_stream().cuda_stream
    plan.dec(x.data_ptr(), y0.data_ptr(), 2, s)
    with ndwt.kernel_trace() as recs:
        plan.dec(x.data_ptr(), y1.data_ptr(), 2, s)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and len(recs) == 2
    assert all(r.grid[0] > 0 and r.block[0] == r.params["NT"] for r in recs)
    plan.dec(x.data_ptr(), y1.data_ptr(), 2, s)
    assert ndwt.trace.read_log(ndwt.lib()) == ndwt.trace.read_log(ndwt.lib())       # untouched while off
    with ndwt.kernel_trace() as recs2:
        pass
    assert recs2 == []                                        # turning it on cleared the log


# ---- the per-axis passes: axis_select (csrc/ndwt_select.h) names the kernel of every pass and its grid, and axis_pass launches that.
# Each case is a plan and the passes its dec and its rec make, in launch order, as the queries axis_pass builds for them
# (helpers.axis_query: n, taps, then what differs from a periodic pass along the contiguous axis of float data at tap stride 1).  The
# select shim answers the queries on the host; the trace must show exactly those launches.  The shapes are the written-out cases of
# tests/test_dispatch_select.py::test_axis_pick_on_both_sides_of_every_threshold that a plan can express.
def A(aid, kind, n, wn, level=1, dil="reference", inner=1, K=0, generic=False, offset=0, dec=(), rec=()):
    return pytest.param(dict(kind=kind, n=n, wn=wn, level=level, dil=dil, inner=inner, K=K, generic=generic, offset=offset, dec=list(dec),
                             rec=list(rec)), id=aid)


def _both(n, L, times=1, strides=(1,), **kw):
    """`times` levels (or the levels of `strides`, finest first) of a 1-D transform: the passes of dec, and those of rec, coarsest first"""
    q = helpers.axis_query
    strides = list(strides) * times
    return dict(dec=[q(n, L, stride=s, **kw) for s in strides], rec=[q(n, L, syn=True, stride=s, **kw) for s in reversed(strides)])


AXIS_CASES = [
    A("1d-f32-n32", "f32", 32, "db2", level=2, **_both(32, 4, 2)),                                       # 32 = 8 L: AxisX VEC4, one segment
    A("1d-f32-n31", "f32", 31, "db2", level=2, **_both(31, 4, 2)),                                       # element-wise
    A("1d-f32-n34", "f32", 34, "db2", level=2, **_both(34, 4, 2)),                                       # rows of 34: AxisX VEC4 = false
    A("1d-f32-n32-offset", "f32", 32, "db2", level=2, offset=1, **_both(32, 4, 2, aligned=False)),       # pointers off the groups: the same
    A("1d-c64-n24", "c64", 24, "db3", level=2, **_both(24, 6, 2, comp=2)),                               # 48 scalars = 8 L: AxisX EW = 2
    A("1d-c64-n23", "c64", 23, "db3", level=2, **_both(23, 6, 2, comp=2)),                               # element-wise
    A("1d-f64-db6-n96", "f64", 96, "db6", level=2, **_both(96, 12, 2, f64=True)),                        # AxisX L = 12
    A("1d-f64-db7", "f64", 128, "db7", level=2, **_both(128, 14, 2, f64=True)),                          # no AxisX beyond 12 taps
    A("1d-generic", "f32", 64, "db2", level=2, generic=True, **_both(64, 4, 2, path_auto=False)),
    A("inter4-n40-k1", "f32", 40, "db2", inner=4, K=1, **_both(40, 4, inner=4, outer=1)),                # AxisMarch: 4 chunks of 12
    A("inter4-n40-k3", "f32", 40, "db2", inner=4, K=3, **_both(40, 4, inner=4, outer=3)),
    A("inter3-n40-k1", "f32", 40, "db2", inner=3, K=1, **_both(40, 4, inner=3, outer=1)),                 # samples of 3 scalars: element-wise
    A("inter3-n40-k3", "f32", 40, "db2", inner=3, K=3, **_both(40, 4, inner=3, outer=3)),
    A("inter4-n40-k1-offset", "f32", 40, "db2", inner=4, K=1, offset=1, **_both(40, 4, inner=4, outer=1, aligned=False)),
    A("inter4-n40-k3-offset", "f32", 40, "db2", inner=4, K=3, offset=1, **_both(40, 4, inner=4, outer=3, aligned=False)),
    A("1d-atrous-n32", "f32", 32, "db2", level=3, dil="atrous", **_both(32, 4, strides=(1, 2, 4))),      # AxisX; 2 sub-lattices: element-wise; 4: AxisMarch on [8][4]
    A("1d-atrous-n12", "f32", 12, "db2", level=3, dil="atrous", **_both(12, 4, strides=(1, 2, 4))),      # 12 < 8 L; inner 2; 3 < L samples
    A("slab-f64-db9", "slab", 20, "db9"),                                                                # _axis_slab_case: its passes are written there
]
_AXIS_KINDS = {"f32": ("single", False), "c64": ("single", True), "f64": ("double", False)}


@pytest.fixture(scope="module")
def select_shim(tmp_path_factory):
    return helpers.build_select_shim(str(tmp_path_factory.mktemp("select")))


def _check_axis_launches(shim, recs, queries, what):
    picks = helpers.axis_picks(shim, queries)
    want = [helpers.axis_launch(q, k) for q, k in zip(queries, picks)]
    shown = "\n  ".join(map(repr, recs))
    assert len(recs) == len(want), f"{what}: {len(want)} passes expected; launched:\n  {shown}"
    for r, (fam, params, grid) in zip(recs, want):
        assert matches(r, (fam, params)) and r.grid == (grid, 1, 1) and r.block == (256, 1, 1), f"{what}: the pick is {fam} {params} grid {grid}; launched:\n  {shown}"


def _oracle_1d(a, fn):
    """fn on every (item, inner index) column of a [K, n, inner] array, real and imaginary part on their own: [K, n, inner, bands..]"""
    out = None
    for k in range(a.shape[0]):
        for c in range(a.shape[2]):
            v = a[k, :, c]
            r = fn(v.real) + 1j * fn(v.imag) if np.iscomplexobj(v) else fn(v)
            if out is None:
                out = np.zeros(a.shape[:1] + r.shape[:1] + a.shape[2:3] + r.shape[1:], dtype=r.dtype)
            out[k, :, c] = r
    return out


@pytest.mark.parametrize("case", AXIS_CASES)
def test_axis_pass_launches_the_pick(select_shim, case):
    """every traced launch of dec and of rec is axis_select's pick for that pass -- family, T, L, SYN, EW, VEC4 and grid -- and the values
    hold the bounds of tests/test_gpu_parity.py against the numpy oracle: dec <= TOL, rec(dec(x)) <= 20 TOL"""
    import ndwt_oracle as orc
    if case["kind"] == "slab":
        return _axis_slab_case(select_shim, case["n"])
    prec, cplx = _AXIS_KINDS[case["kind"]]
    ndt, tdt = _dtypes(prec, cplx)
    n, wn, level, dil, inner, K, off = case["n"], case["wn"], case["level"], case["dil"], case["inner"], max(case["K"], 1), case["offset"]
    kw = dict(inner=inner, howmany=case["K"]) if case["K"] else {}
    plan = ndwt.Plan([n], [wn], torch.float32 if prec == "single" else torch.float64, cplx, True, dil, max_level=level, **kw)
    if case["generic"]:
        plan.set_path(True)
    rng = np.random.default_rng(zlib.crc32(repr((case["kind"], n, wn, level, dil, inner, K)).encode()))
    x = rng.standard_normal((K, n, inner)) + (1j * rng.standard_normal((K, n, inner)) if cplx else 0)
    x = x.astype(ndt).astype(np.complex128 if cplx else np.float64)
    nb, vol = ndwt.num_bands(1, level), K * n * inner
    want = _oracle_1d(x, lambda v: orc.spatial_dec(v, [wn], level, 1, dil))          # [K, n, inner, nb]
    xb, yb, rb = _Buf(vol, tdt, off), _Buf(nb * vol, tdt, off), _Buf(vol, tdt, off)
    xb.view.copy_(torch.from_numpy(x.astype(ndt).reshape(-1)).cuda())
    stream = torch.cuda.current_stream().cuda_stream
    what = f"{case['kind']} n={n} {wn} L{level} {dil} inner={inner} K={case['K']} offset={off}"
    with ndwt.kernel_trace() as recs:
        plan.dec(xb.ptr(), yb.ptr(), level, stream)
    torch.cuda.synchronize()
    _check_axis_launches(select_shim, recs, case["dec"], f"dec {what}")
    y = np.moveaxis(yb.view.cpu().numpy().reshape(nb, K, n, inner), 0, -1)
    err = np.abs(y - want).max() / np.abs(want).max()
    print(f"[axis-pick] {what}: dec {err:.3g} (bound {TOL[prec]:.3g})")
    assert err <= TOL[prec], (what, "dec", err)
    with ndwt.kernel_trace() as recs:
        plan.rec(yb.ptr(), rb.ptr(), level, stream)
    torch.cuda.synchronize()
    _check_axis_launches(select_shim, recs, case["rec"], f"rec {what}")
    back = rb.view.cpu().numpy().reshape(K, n, inner)
    err = np.abs(back - x).max() / np.abs(x).max()
    print(f"[axis-pick] {what}: rec(dec(x)) {err:.3g} (bound {20 * TOL[prec]:.3g})")
    assert err <= 20 * TOL[prec], (what, "round trip", err)
    for b in (yb, rb):
        assert float(b.t[:off].abs().sum()) == 0 and float(b.t[off + b.n:].abs().sum()) == 0, (what, "stored outside the output")


def _axis_slab_case(select_shim, N):
    """one level of a double db9 plan (18 taps: no fused form) on a 20 x 20 x 20 slab of the outermost axis with its 17 halo planes: the
    pass along the sharded axis is not periodic -- AxisMarch with n_in = n + L - 1 --, y marches, x runs the element-wise kernels; the
    same checks as above.  The slab is the whole periodic volume, so its halo planes are its own planes from the other end."""
    import ndwt_oracle as orc
    q, L, tol = helpers.axis_query, 18, TOL["double"]
    plan = ndwt.Plan([N, N, N], ["db9"] * 3, torch.float64, False, True, "reference", max_level=1, global_outer=N)
    ab, aa, sb, sa = plan.slab_halo(1)
    assert (ab, aa, sb, sa) == (8, 9, 9, 8)
    x = np.random.default_rng(20).standard_normal((N, N, N))
    xk = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()                         # (z, y, x)
    stream = torch.cuda.current_stream().cuda_stream
    z, yy, xx = (dict(f64=True, inner=N * N, outer=1, wrap=False, contiguous=False), dict(f64=True, inner=N, contiguous=False), dict(f64=True))
    xin = xk[torch.arange(-ab, N + aa) % N].contiguous()
    bands = torch.zeros(8, N, N, N, dtype=torch.float64, device="cuda")
    with ndwt.kernel_trace() as recs:
        plan.analysis_level_slab(xin.data_ptr(), [bands[b].data_ptr() for b in range(8)], 1, stream)
    torch.cuda.synchronize()
    half = [q(N, L, outer=N, **yy), q(N, L, outer=N * N, **xx), q(N, L, outer=N * N, **xx)]
    _check_axis_launches(select_shim, recs, [q(N, L, **z)] + half + half, "slab analysis")
    want = orc.spatial_dec(x, ["db9"] * 3, 1, 1)
    err = np.abs(np.transpose(bands.cpu().numpy()) - want).max() / np.abs(want).max()
    print(f"[axis-pick] slab double db9: dec {err:.3g} (bound {tol:.3g})")
    assert err <= tol, ("slab analysis", err)
    cin = bands[:, torch.arange(-sb, N + sa) % N].contiguous()                      # (band, 37 planes, y, x)
    out = torch.zeros(N, N, N, dtype=torch.float64, device="cuda")
    with ndwt.kernel_trace() as recs:
        plan.synthesis_level_slab([cin[b].data_ptr() for b in range(8)], out.data_ptr(), 1, stream)
    torch.cuda.synchronize()
    nh = N + L - 1
    half = [q(N, L, syn=True, outer=N * nh, **xx), q(N, L, syn=True, outer=N * nh, **xx), q(N, L, syn=True, outer=nh, **yy)]
    _check_axis_launches(select_shim, recs, half + half + [q(N, L, syn=True, **z)], "slab synthesis")
    err = float((out - xk).abs().max()) / np.abs(x).max()
    print(f"[axis-pick] slab double db9: rec(dec(x)) {err:.3g} (bound {20 * tol:.3g})")
    assert err <= 20 * tol, ("slab round trip", err)


# ---- coverage: one compact sweep of small shapes that must launch every entry of helpers.COVERAGE, every call checked against the oracle
COVERAGE_ROWS = [p.values[0] for p in ROWS if p.id in {
    "tall-tile-4d-frames-32", "tall-tile-4d-frames-16", "pin-db6", "nopin-n1-70", "inv3y-scatter-20", "inv3y-gather-20-ragged",
    "inv3y-uniyz-false", "inv3s-odd-16", "c64-db5", "c128-db5", "c128-db6", "atrous-db4-l3", "atrous-db4-l3-offset", "atrous-indivisible",
    "atrous-2d-l3", "f64-db4", "inv2p-n2-64", "2d-db9-ragged", "2d-f64-db8", "2d-f64-db4", "den3-db2", "1d-vec4", "1d-ragged", "1d-c64",
    "fwd7-folded-t", "inv3-lds-kernel", "fwd11-inv11-small-cascade", "fwd10-inv12-small-cascade", "fwd11-db6-cascade-2lev",
    "inv7-inv2p-scalar", "2d-c64-db5"}]


def test_dispatch_coverage():
    recs = []
    for row in COVERAGE_ROWS:
        recs += run_row(row, trace_check=False)
    # the copy kernels: the slab entry points (segments) and the multi-slab synthesis (add_planes)
    recs += _segment_and_multi_slab_launches()
    missing = [f"{fam} {' '.join(f'{k}={v}' for k, v in p.items())}" for fam, p in COVERAGE if not any(matches(r, (fam, p)) for r in recs)]
    assert not missing, f"not reached by the coverage sweep: {missing}"


def _segment_and_multi_slab_launches():
    api = __import__("importlib").import_module("non-decimated_wavelets_amd.api")
    recs = []
    plan = ndwt.Plan([64, 40, 36], ["db2"] * 3, torch.float32, False, True, "reference", max_level=1)
    src = torch.randn(4096, device="cuda")
    dst = torch.zeros(4096, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    with ndwt.kernel_trace() as r:
        plan.slab_segments(False, [dst.data_ptr()], [src.data_ptr()], [4096], s)
        plan.slab_segments_strided(True, [dst.data_ptr()], [src.data_ptr()], [1000], 2, [2048], [2048], s)
    torch.cuda.synchronize()
    recs += r
    assert torch.equal(dst[:1000], 2 * src[:1000]) and torch.equal(dst[2048:3048], 2 * src[2048:3048])
    # a multi-slab plan on one device: the scatter-add synthesis adds the halo planes of neighbouring slabs (add_planes_kernel)
    dims, wn = [72, 40, 50], ["db4"] * 3
    x = np.random.default_rng(5).standard_normal(dims)
    mp = api.MultiPlan(dims, wn, torch.float32, [0, 0, 0], False, True, "reference", max_level=2)
    mp.set_exchange("scatter")
    with ndwt.kernel_trace() as r:
        yk = mp.dec(np.ascontiguousarray(x.T).astype(np.float32), 2)
        rk = mp.rec(yk)
    recs += r
    assert np.abs(rk.T - x).max() <= 20 * TOL["single"] * np.abs(x).max()
    assert np.abs(yk.T - orc_c.spatial_dec(x.astype(np.float32).astype(np.float64), wn, 2, 1)).max() <= TOL["single"] * np.abs(yk).max()
    return recs
