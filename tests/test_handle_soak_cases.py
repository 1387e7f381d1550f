"""The GPU handle soak's slice (tests/test_gpu_handle_soak.py) is not vacuous: the generator alone (soak_handles.case, no GPU), over
exactly the seeds that module runs, meets every operation kind, every ordered pair of streams for two renders with no host wait
between them -- of one handle and across two --, every pass of kFramePassTable, and leaves no handle without a frame; it is deterministic,
and its reference frames (the oracle and the models: no GPU either) show terrain and change when a pass is switched."""
import collections
import functools

import numpy as np

import soak_handles as sh
from test_gpu_handle_soak import CASES, FIRST_SEED

SEEDS = range(FIRST_SEED, FIRST_SEED + CASES)


@functools.lru_cache(maxsize=None)
def cases():
    return [sh.case(seed) for seed in SEEDS]


def test_every_operation_kind_occurs_and_the_cases_have_the_stated_shape():
    kinds = collections.Counter(op["kind"] for c in cases() for op in c["ops"])
    print(dict(kinds))
    assert all(kinds[k] >= 2 for k in sh.KINDS), kinds
    for c in cases():
        assert 2 <= len(c["handles"]) <= 3 and 2 <= c["streams"] <= 3 and 12 <= len(c["ops"]) <= 20, c["name"]
    assert {len(c["handles"]) for c in cases()} == {2, 3} and {c["streams"] for c in cases()} == {2, 3}
    ops = [op for c in cases() for op in c["ops"]]
    assert {op["field"] for op in ops if op["kind"] == "field_host"} | {op["field"] for op in ops if op["kind"] == "field_device"} == set(sh.FIELDS)
    assert {"lines", "contours"} <= {op["layer"][0] for op in ops if "layer" in op} and any(op["kind"] == "toggle_layer" and "layer" not in op for op in ops)


def test_every_ordered_stream_pair_occurs_for_one_handle_and_across_handles():
    same, across = set(), set()
    for c in cases():
        a, b = sh.render_pairs(c)
        same |= a
        across |= b
    every = {(a, b) for a in range(3) for b in range(3) if a != b}
    assert same == every and across == every, (sorted(same), sorted(across))


def test_every_pass_is_on_in_some_frame_and_every_handle_renders():
    on = collections.Counter()
    for c in cases():
        drawn = set()
        for op in c["ops"]:
            if op["kind"] == "render":
                drawn.add(op["h"])
                on.update(op["inputs"]["on"])
                on.update(["layers"] if op["inputs"]["layers"] else [])
        assert drawn == set(range(len(c["handles"]))), c["name"]
    print(dict(on))
    assert all(on[p] >= 2 for p in sh.PASSES) and on["layers"] >= 2, on
    # ... and several at once, which is where their order shows
    assert any(len(op["inputs"]["on"]) >= 3 for c in cases() for op in c["ops"] if op["kind"] == "render")


def test_a_read_back_follows_a_frame_of_the_same_handle_and_handle_0_stays():
    for c in cases():
        for i, op in enumerate(c["ops"]):
            assert not (op["kind"] == "recreate" and op["h"] == 0)
            if op["kind"] == "read_rgba":
                assert sh.x_of_last_frame(c, i) is not None


def test_the_generator_is_deterministic():
    a, b = sh.case(FIRST_SEED + 3), sh.case(FIRST_SEED + 3)
    assert [(o["kind"], o["h"], o.get("s"), o.get("field"), o.get("p")) for o in a["ops"]] == [(o["kind"], o["h"], o.get("s"), o.get("field"), o.get("p")) for o in b["ops"]]
    for x, y in zip(a["handles"], b["handles"]):
        assert np.array_equal(x["h"], y["h"]) and (x["W"], x["H"], x["G"], x["on"], x["cam"]) == (y["W"], y["H"], y["G"], y["on"], y["cam"])
    assert sh.case(FIRST_SEED + 4)["ops"] != a["ops"]


def test_the_reference_shows_terrain_and_follows_the_passes(oracle):
    """(one case: the frames of the reference are not empty, and a pass that is switched changes them)"""
    c = sh.case(FIRST_SEED)
    memo = {}
    frames = [(op["inputs"], sh.expected(op["inputs"], memo)) for op in c["ops"] if op["kind"] == "render"]
    assert frames and all((e["vis"] != 0).mean() > (0.1 if x["H"] >= 64 else 0.0) for x, e in frames)
    x = next(x for x in c["handles"] if x["H"] >= 64)                # (the 130 x 3 strip shows a few pixels of terrain: too few for every pass)
    bare = sh.expected(sh.changed(x, on=(), layers=[]), memo)["frame"]
    for p in sh.PASSES:
        assert (sh.expected(sh.changed(x, on=(p,), layers=[]), memo)["frame"] != bare).any(), p
