"""The grid rule of the joint shrinkage and the group norms (csrc/ndwt_select.h: joint_chunks) without a GPU, through
tests/select/joint_shim.cpp: both sides of every condition.

  steps          a band gets a further chunk only while every one of a workgroup's 256 threads keeps max(1, kSelectTurns / items) steps:
                 one step already moves a load of every item
  cap            all workgroups together stay within num_cus * 16; above that many bands every band has one chunk
  target_blocks  an upper bound on all workgroups on top of that (0: none)
  registers      kJointReg is one of 4, 8, 16
"""
import ctypes

import pytest

from items_cases import build_named_shim

CUS = 256


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_named_shim(tmp_path_factory, "joint_shim")
    lib.sel_joint_chunks.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_joint_chunks.restype = ctypes.c_longlong
    return lib


def test_a_further_chunk_only_while_every_thread_keeps_its_steps(shim):
    turns = shim.sel_joint_turns()
    assert turns == 8
    for items in (1, 2, 3, 4, 5, 7, 8, 9, 40, 4096):
        keep = max(1, turns // items)                              # 8, 4, 2, 2, 1, 1, 1, 1, ...
        per_chunk = 256 * keep
        for comp, vec, scalars_per_step in ((1, 1, 4), (2, 1, 4), (1, 0, 1), (2, 0, 2)):
            s = per_chunk * scalars_per_step
            assert shim.sel_joint_chunks(s - scalars_per_step, comp, vec, 1, items, CUS, 0) == 1   # fewer steps than a chunk wants: one chunk
            assert shim.sel_joint_chunks(s, comp, vec, 1, items, CUS, 0) == 1
            assert shim.sel_joint_chunks(2 * s - scalars_per_step, comp, vec, 1, items, CUS, 0) == 1
            assert shim.sel_joint_chunks(2 * s, comp, vec, 1, items, CUS, 0) == 2
            assert shim.sel_joint_chunks(5 * s + 3 * scalars_per_step, comp, vec, 1, items, CUS, 0) == 5
    # both sides of turns / items >= 1: at 8 items a thread keeps one step, at 9 still one (never none)
    assert shim.sel_joint_chunks(4 * 256 * 2, 1, 1, 1, 7, CUS, 0) == 2 and shim.sel_joint_chunks(4 * 256 * 2, 1, 1, 1, 4, CUS, 0) == 1
    assert shim.sel_joint_chunks(4 * 256 * 2, 1, 1, 1, 8, CUS, 0) == shim.sel_joint_chunks(4 * 256 * 2, 1, 1, 1, 9, CUS, 0) == 2
    assert shim.sel_joint_chunks(4, 1, 1, 3, 5, CUS, 0) == 1 and shim.sel_joint_chunks(1, 1, 0, 1, 1, CUS, 0) == 1   # at least one
    # (tests/test_gpu_joint.py: 2 x 20000, level 1 -- 5000 steps, 4 a thread: 4 chunks; element-wise 20000 steps: 19)
    assert shim.sel_joint_chunks(20000, 1, 1, 2, 2, CUS, 0) == 4 and shim.sel_joint_chunks(20000, 1, 0, 2, 2, CUS, 0) == 19
    # the items do not divide the cap: unlike norms_chunks, a workgroup serves every item
    assert shim.sel_joint_chunks(1 << 30, 1, 1, 2, 1 << 20, CUS, 0) == CUS * 16 // 2


def test_the_cap_on_all_workgroups(shim):
    big = 1 << 30
    cap = CUS * 16
    assert shim.sel_joint_chunks(big, 1, 1, 1, 1, CUS, 0) == cap
    assert shim.sel_joint_chunks(big, 1, 1, 8, 1, CUS, 0) == cap // 8
    assert shim.sel_joint_chunks(big, 1, 1, 15, 3, CUS, 0) == cap // 15                           # rounded down: within the cap
    assert shim.sel_joint_chunks(big, 1, 1, 15, 3, 64, 0) == 64 * 16 // 15                        # the cap is the device's
    assert shim.sel_joint_chunks(big, 1, 1, cap // 2, 1, CUS, 0) == 2
    assert shim.sel_joint_chunks(big, 1, 1, cap // 2 + 1, 1, CUS, 0) == 1
    assert shim.sel_joint_chunks(big, 1, 1, cap, 1, CUS, 0) == 1
    assert shim.sel_joint_chunks(big, 1, 1, cap + 1, 1, CUS, 0) == 1                              # more bands than the cap: one chunk each


def test_target_blocks_is_an_upper_bound_on_top(shim):
    big = 1 << 30
    assert shim.sel_joint_chunks(big, 1, 1, 4, 2, CUS, 40) == 10
    assert shim.sel_joint_chunks(big, 1, 1, 4, 2, CUS, 1) == 1                                    # below the bands: still one each
    assert shim.sel_joint_chunks(big, 1, 1, 4, 2, CUS, 1 << 20) == CUS * 16 // 4                  # above the cap: the cap holds
    assert shim.sel_joint_chunks(20000, 1, 1, 2, 2, CUS, 40) == 4                                 # above what the steps give: they hold
    assert shim.sel_joint_chunks(20000, 1, 1, 2, 2, CUS, 6) == 3 and shim.sel_joint_chunks(20000, 1, 1, 2, 2, CUS, 1) == 1
    assert shim.sel_joint_chunks(20000, 1, 1, 2, 2, CUS, 0) == shim.sel_joint_chunks(20000, 1, 1, 2, 2, CUS, -3) == 4   # none


def test_the_registers_hold_one_of_the_three_sizes(shim):
    assert shim.sel_joint_reg() in (4, 8, 16)
