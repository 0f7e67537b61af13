"""Without a GPU: the launch arithmetic of the low-rank and the shifted-window attention kernels, as tests/test_gpu_lowrank_attn.py and tests/test_gpu_winattn.py
restate it (`reached`), says of every shape of those files what the shape is listed for (`REACHES`), and the shapes together reach every cells-per-workgroup the
host rule can return, both passes of the dK / dV second stage, and a ragged second and third trip of the table reduce."""
import pytest

import test_gpu_lowrank_attn as LR
import test_gpu_winattn as WIN


@pytest.mark.parametrize("shape", LR.SHAPES + LR.NEW_SHAPES, ids=str)
def test_the_lowrank_shape_reaches_the_code_it_is_listed_for(shape):
    want = LR.REACHES[shape]
    got = LR.reached(*shape)
    assert {k: got.get(k) for k in want} == want
    B, Hq, Wq, D = shape
    assert Hq % 8 == 0 and Wq % 8 == 0 and D in (16, 32, 64, 128)
    # the identities the kernel's walk rests on: whole cells per workgroup, all 64 cells covered, every round but the last full
    assert got["cpw"] * got["nwg"] == 64 and got["nwg"] * got["cpw"] * got["qpc"] == Hq * Wq
    assert 0 < got["last"] <= 64 and 64 * (got["rounds"] - 1) + got["last"] == got["cpw"] * got["qpc"]
    assert got["cpw"] == 1 or got["cpw"] * got["qpc"] <= 256


def test_the_lowrank_shapes_reach_every_cells_per_workgroup_and_both_passes():
    r = [LR.reached(*s) for s in LR.SHAPES + LR.NEW_SHAPES]
    # 32 cells of 8 queries are the largest that fit 256, so every power of two down to 1 is a value cells_per_wg returns
    assert {x["cpw"] for x in r} == {64, 32, 16, 8, 4, 2, 1}
    assert {x["kv_passes"] for x in r} == {1, 2}
    assert any(x["wave1_empty"] and x["last"] < 32 for x in r) and any(x["wave1_empty"] and x["last"] == 32 for x in r)
    assert any(x["cpw"] == 1 and x["rounds"] >= 4 for x in r)          # one cell's running bias sum carried over four rounds
    assert max(x["fold"] for x in r) == 17 and max(x["nwg"] for x in r) == 64
    # a step's sites (docs/kernel_table.md: batch 16, heads 4): down1 / up3 runs one cell per workgroup, down4 fills the capped grid exactly, batch 32 needs a second pass
    assert LR.reached(16, 128, 128, 16)["cpw"] == 1
    assert 16 * 4 * 2 * 64 * 128 == 4096 * 256 and LR.reached(16, 8, 8, 128)["kv_passes"] == 1 and LR.reached(32, 8, 8, 128)["kv_passes"] == 2


@pytest.mark.parametrize("shape", WIN.SHAPES + WIN.NEW_SHAPES, ids=str)
def test_the_window_shape_reaches_the_code_it_is_listed_for(shape):
    want = WIN.REACHES[shape]
    got = WIN.reached(*shape)
    assert {k: got.get(k) for k in want} == want
    B, H, W, heads, shift = shape
    assert H % 8 == 0 and W % 8 == 0 and (shift == 0 or (shift == 4 and H > 8 and W > 8))


def test_the_window_shapes_reach_shift_0_over_several_windows_and_a_ragged_later_trip():
    r = [WIN.reached(*s) for s in WIN.SHAPES + WIN.NEW_SHAPES]
    assert any(x["shift"] == 0 and x["nw"] > 1 for x in r)
    assert any(x["ragged"] and x["reduce_iters"] >= 3 for x in r)          # more than 8 partial rows, no multiple of 8
    assert any(x["nblk"] == 256 for x in r)                                 # a step's stage-0 grid at 4 images
    assert all(x["reduce_iters"] <= 2 for x in (WIN.reached(*s) for s in WIN.SHAPES))          # what the first four shapes alone reach
