"""The host builder of the tap tables (csrc/ndwt_taps_host.h) against the structs the kernels read them through (Taps3, Taps3Y and
TapsDen of csrc/ndwt_device.h): the library uploads the builder's scalars and the host emulation of the kernels copies them into
K::Taps, so the order of those scalars is checked once, here.

tests/emu/ndwt_taps_main.cpp is a program of its own (every even tap length 2 .. 20 in float and double, TapsDen<float> for 2 .. 8 taps,
distinct tap values, every field compared by name), built with AddressSanitizer and UBSan and run as a child process with nothing
preloaded, as tests/test_emulated_cascade1.py runs its cases.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def test_the_tap_tables_match_their_structs_under_address_and_ub_sanitizers():
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the program")
    src = os.path.join(EMU, "ndwt_taps_main.cpp")
    prog = os.path.join(EMU, "build", "ndwt_taps_asan")
    os.makedirs(os.path.dirname(prog), exist_ok=True)
    newest = max(os.path.getmtime(f) for f in (src, os.path.join(CSRC, "ndwt_taps_host.h"), os.path.join(CSRC, "ndwt_device.h")))
    if not os.path.exists(prog) or os.path.getmtime(prog) < newest:
        subprocess.check_call([CXX, "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{CSRC}",
                               src, "-o", prog])
    r = subprocess.run([prog], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "44 tap tables ok" in r.stdout                    # 10 tap lengths x (Taps3, Taps3Y) x (float, double) + 4 TapsDen
