"""Without a GPU: the launch arithmetic of the per-image report's kernels, as tests/test_gpu_report.py restates it (`reached`), says of every shape of that
file what the shape is listed for (`REACHES`); the restatement gives the workspace sizes the library itself reports; and the shapes together reach a partial
word, whole words, a ragged last tile in both directions, an image inside the 31-pixel window, several workgroups on one image and a ragged second trip of
both fold kernels."""
import pytest

import test_gpu_report as REP


@pytest.mark.parametrize("case", list(REP.CASES))
def test_the_report_shape_reaches_the_code_it_is_listed_for(case):
    images, H, W = REP.CASES[case]
    want, got = REP.REACHES[case], REP.reached(images, H, W)
    assert {k: got.get(k) for k in want} == want
    from mdvit_amd import _lib
    lib = _lib.load()
    n = sum(images)
    assert lib.mdvit_eval_images_ws_bytes(n, H * W) == got["ws_images"] and lib.mdvit_eval_structure_ws_bytes(n, H, W) == got["ws_structure"]


def test_the_report_shapes_reach_every_path_together():
    r = {c: REP.reached(*REP.CASES[c]) for c in REP.CASES}
    assert any(x["words"] == 1 and x["tail_bits"] for x in r.values()) and any(x["tail_bits"] == 0 for x in r.values())
    assert any(x["words"] > 1 and x["tail_bits"] for x in r.values())
    assert any(x["ragged_tile"] == (True, True) and x["tiles"][0] > 1 and x["tiles"][1] > 1 for x in r.values())
    assert any(x["inside_window"] == (True, True) for x in r.values()) and any(x["inside_window"] == (True, False) for x in r.values())
    assert any(x["n"] == 1 and x["nblk"] > 1 for x in r.values())
    assert any(x["count_fold_ragged"] and x["count_fold_trips"] >= 2 for x in r.values())
    assert any(x["sum_fold_ragged"] and x["sum_fold_trips"] >= 2 for x in r.values())
    assert {len(REP.CASES[c][0]) for c in REP.CASES} == {1, 2, 3} and len(set(REP.CASES["odd_20x37"][0])) == 3          # unequal groups
    # the sizes the entries refuse have no workspace
    from mdvit_amd import _lib
    lib = _lib.load()
    assert lib.mdvit_eval_images_ws_bytes(1, (1 << 30) + 1) == 0 and lib.mdvit_eval_structure_ws_bytes(65536, 8, 8) == 0
    # the cap: past 1024 x 16 words a workgroup takes more words, and no workgroup is empty
    big = REP.reached((1,), 4096, 4096)
    assert big["words"] == 262144 and big["nblk"] == 1024 and lib.mdvit_eval_images_ws_bytes(1, 4096 * 4096) == big["ws_images"]
    odd = REP.reached((1,), 1, 64 * (1024 * 16 + 1))
    assert odd["nblk"] == 964 == -(-16385 // 17) and lib.mdvit_eval_images_ws_bytes(1, 64 * (1024 * 16 + 1)) == odd["ws_images"]
