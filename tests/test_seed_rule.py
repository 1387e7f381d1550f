"""The seed-list rule of set_flood and set_spill is one rule: the same list gives both calls the same array, and a
malformed one is refused with each feature's own wording.  No device."""
import numpy as np
import pytest

from vulkan_forge_amd._flood import flood_args
from vulkan_forge_amd._spill import spill_args

FLOOD_WHAT, SPILL_WHAT = 'seeds must be None, "edges" or (N, 2) numbers', 'seeds must be "edges" or (N, 2) numbers'


def xz_of(args):
    (xz,) = [a for a in args if isinstance(a, np.ndarray)]
    return xz


@pytest.mark.parametrize("seeds", ([(0.1, 0.2)], [[1, 2], [3, 4], [1, 2]], np.arange(12, dtype=np.float64).reshape(6, 2)[::2],
                                   np.linspace(-2, 2, 2 * 65535, dtype=np.float32).reshape(65535, 2), np.array([[1, 2]], np.uint8)))
def test_both_calls_make_the_same_array_of_a_seed_list(seeds):
    f, s = xz_of(flood_args(0.0, seeds)), xz_of(spill_args(seeds))
    assert f.dtype == s.dtype == np.float32 and f.shape == s.shape == (len(seeds), 2)
    assert f.flags.c_contiguous and s.flags.c_contiguous
    assert f.tobytes() == s.tobytes() == np.asarray(seeds, np.float32).tobytes()


@pytest.mark.parametrize("bad, exc, said", (
    (np.array([["a", "b"]]), TypeError, "{what}, got dtype <U1"),
    (np.zeros((2, 3)), ValueError, "seeds must be (N, 2) numbers, got shape (2, 3)"),
    (np.zeros((0, 2)), ValueError, "seeds must hold 1 to 65535 rows, got 0"),
    (np.zeros((65536, 2)), ValueError, "seeds must hold 1 to 65535 rows, got 65536"),
    ([(0.0, 0.0), (float("nan"), 0.1)], ValueError, "seeds must be finite"),
))
def test_a_malformed_list_is_refused_in_the_features_own_words(bad, exc, said):
    for call, what in ((lambda: flood_args(0.0, bad), FLOOD_WHAT), (lambda: spill_args(bad), SPILL_WHAT)):
        with pytest.raises(exc) as e:
            call()
        assert str(e.value) == said.format(what=what)
