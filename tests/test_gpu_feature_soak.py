"""A bounded slice of the feature soak (tests/soak_features.py) inside the suite: the hand-written corners, one test each, and twelve
blocks of four seeded random cases.  Every pass that runs after the tile kernel -- geometry buffers and pick, the shadow and
sky-view fields and their shade passes, the draped image with its mip pyramid and anisotropic taps, the viewshed, cumulative-viewshed
and sun-exposure fields and their tints, the flood's and the spill's fields (at two group sizes, the spill's with and without its
activity flags), the water and the sink tint, the haze, point / line / polygon / contour overlays with occlusion, their point, line
and contour layers under the haze where a case flags them (set_layer_haze directly after a layer's add or after all adds, a ladder
of hazed points across the frame's depths) -- equals its CPU model on the oracle's frame, on one handle, before and after four
mutations of the handle and after the drape is cleared; the vertex
fields and the pyramid are computed as often as include/vf_hip.h says; a case with a factor above 1 runs the same passes on a
supersampled second handle.  Fixed seeds (a failure reproduces from the commit alone); VF_FEATURE_SOAK_FIRST_SEED moves the window.
tests/test_feature_soak_cases.py asserts, without a GPU, that these very cases are not vacuous."""
import os

import pytest

import soak_features as sf

pytestmark = pytest.mark.gpu

FIRST_SEED, BLOCKS, PER_BLOCK = 7000, 12, 4                # (the same 48 seeds as six blocks of eight held before the late passes)


def first_seed():
    return int(os.environ.get("VF_FEATURE_SOAK_FIRST_SEED", str(FIRST_SEED)))


def report(bad):
    return "\n".join(f"{m[0]} step {m[1]}: {m[2]}: {m[3]} differ, first at {m[4]}" for m in bad[:10])


@pytest.mark.parametrize("corner", sf.CORNERS.names)
def test_corners(corner):
    import oracle  # noqa: F401
    from vulkan_forge_amd import cabi  # noqa: F401
    bad = sf.run_case(sf.CORNERS.named(corner))
    assert not bad, report(bad)


@pytest.mark.parametrize("block", range(BLOCKS))
def test_slice(block):
    import oracle  # noqa: F401
    from vulkan_forge_amd import cabi  # noqa: F401
    res = sf.run(first=first_seed() + PER_BLOCK * block, cases=PER_BLOCK, budget=float("inf"), verbose=False, corners=False)
    print("\n" + res["summary"])
    assert not res["bad"], report(res["bad"])
    assert res["cases"] == PER_BLOCK, res["summary"]          # (no case skipped: test_feature_soak_cases.py asserts it of the default window)
