"""The seeded interleaving soak (tests/soak_handles.py) on the GPU: a fixed window of seeds -- two or three handles of one
context on two or three streams of the caller's, 12 - 20 operations each, every frame, field and read-back held to the CPU models.
tests/test_handle_soak_cases.py shows without a GPU that this window meets every operation, every stream pair and every pass."""
import time

import pytest

import soak_handles as sh

pytestmark = pytest.mark.gpu

FIRST_SEED, CASES = 4100, 96


def test_the_window_of_seeds(oracle):
    t0 = time.time()
    res = sh.run(FIRST_SEED, CASES, budget=120.0, verbose=True)
    print(f"handle soak window: {res['cases']} cases in {time.time() - t0:.1f} s")
    assert res["cases"] == CASES, res["summary"]
    assert res["bad"] == [], res["bad"][:8]
    # the interleaving was real: work went onto a second stream while the first still had some
    assert res["stats"]["not_ready"] > 0, f"vacuous: {res['summary']}"
