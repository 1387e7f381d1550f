"""The tile kernel's span solver and line loop as DEVICE code, held against references that share nothing with them.

tests/test_raster_spans.py checks vf_raster.h compiled for the host; on the GPU the header's reciprocal, floor and median are
other instructions, span_exact runs on device FP64, everything is built with the library's -O3 / -mllvm switches, and raster_fast
(vf_kernels.h: four-line groups, ballots between a triangle's lanes, final-pixel masks, skewed LDS paint) exists as device code
only.  Whole terrain frames reach a narrow family of triangles; these tests reach the rest:

  - tests/hip/raster_device_fuzz.hip, built here with the library's flags and run ONCE as a child process: the case stream of the
    host test (same count, same seed: the same triangles) through the solver on the GPU against the brute-force int64 rasteriser,
    and raster_fast<GROUPS> on triangle soup -- every kind, every lane split, final-pixel sets from empty to full, exact and lagging
    four-line masks -- against the same brute force, whole 64 x 64 tiles compared;
  - whole frames whose grid vertices sit ON pixel centres (tests/raster_lattice.py; tests/test_raster_lattice.py shows on the CPU
    that they do), against the oracle as everywhere else: visibility and EXACT colour equal, FAST colour within 1 LSB.
Every comparison is equality."""
import os
import subprocess

import numpy as np
import pytest

import raster_lattice as rl
from support import ROOT

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "hip", "raster_device_fuzz.hip")
DRAWS, SEED, SOUP = 250000, 20250816, 24000           # draws and seed of tests/test_raster_spans.py (ulps 0)
LIMIT_EXTENT, LIMIT_SEED = 16384, 20261018            # extent and seed of tests/test_raster_spans.py's run around the largest frame
_RUN = {}                                              # the child's outcome: it runs once, whatever becomes of it


def _build(exe):
    """hipcc with the library's own flags (an executable: no -shared / -fPIC); like build(), without the -mllvm tuning switches
    when this compiler refuses them.  Then the 64-bit-shift lint of tools/isa_lint.py, which applies to test kernels as well."""
    import __graft_entry__ as g
    from tools import isa_lint
    strip = ("-shared", "-fPIC")
    cmd = [g._hipcc(), *[f for f in g.HIPCC_FLAGS if f not in strip], SRC, "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(f"hipcc refused the tuned command line; building without the code-generation switches:\n{r.stdout[-600:]}")
        subprocess.check_call([g._hipcc(), *[f for f in g.HIPCC_BASE if f not in strip], SRC, "-o", exe])
    kernels, _checked, found = isa_lint.lint(exe)
    assert kernels >= 3, "the lint did not see the program's kernels"
    assert found == [], f"hazardous 64-bit shifts in the test program (reserve a VGPR as vf_device.h shows): {found}"


def _child(tmp_path_factory):
    if not _RUN:
        exe = _RUN["exe"] = str(tmp_path_factory.mktemp("raster_device") / "raster_device_fuzz")
        _RUN["rc"], _RUN["out"] = None, ""
        _build(exe)
        try:
            r = subprocess.run([exe, str(DRAWS), str(SEED), str(SOUP)], capture_output=True, text=True, timeout=120)
            _RUN["rc"], _RUN["out"] = r.returncode, r.stdout + r.stderr
        except subprocess.TimeoutExpired as e:
            _RUN["rc"], _RUN["out"] = "timeout", str(e.stdout or "")
        print(_RUN["out"])
    # 0: all checks passed, 1: some check failed (the tests below say which); anything else: the program did not finish
    assert _RUN["rc"] in (0, 1), f"raster_device_fuzz did not finish (exit {_RUN['rc']}); nothing else of this module is started:\n{_RUN['out'][-3000:]}"
    return _RUN["out"]


@pytest.fixture
def fuzz_output(tmp_path_factory):
    return _child(tmp_path_factory)


def test_span_solver_as_device_code_against_brute_force(fuzz_output):
    lines = fuzz_output.splitlines()
    summary = [l for l in lines if l.startswith("triangles")][0]
    assert int(summary.rsplit("failures", 1)[1]) == 0, "\n".join(lines[:14])
    assert any(l.startswith("device vs host build") for l in lines)
    kinds = {}
    for line in lines:
        f = line.split()
        if f[:1] == ["kind"]:
            kinds[int(f[1].rstrip(":"))] = (int(f[3]), float(f[5]), int(f[8]), float(f[10]))   # triangles, irregular %, lines, fallback % of lines
    assert sorted(kinds) == list(range(10))
    for k, (tris, irregular, nlines, fallback) in kinds.items():
        assert tris > 0 and nlines > 0, f"kind {k} contributed nothing"
        # the terrain's primitives (slivers, general and sub-pixel triangles: kinds 2-6, 8) must be decided in FP32 almost always: the
        # bounds of the host test carry over (eps, and with it the fallback decision, is computed from the inputs alone)
        if k in (2, 3, 4, 5, 6, 8):
            assert irregular < 0.2 and fallback < 0.1, (k, kinds[k])


def test_span_solver_as_device_code_around_a_16384_target(fuzz_output):
    """The span part alone (no soup) on the stream around the largest frame the C ABI accepts: centres up to 16384 * 256 + 51424.
    The solver works in window-relative coordinates, so the bounds of the run above carry over.  (`fuzz_output`: the program is
    built once, and after a first run that did not finish this one is not started.)"""
    r = subprocess.run([_RUN["exe"], str(DRAWS), str(LIMIT_SEED), "0", str(LIMIT_EXTENT)], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode in (0, 1), f"raster_device_fuzz did not finish (exit {r.returncode}):\n{out[-3000:]}"
    test_span_solver_as_device_code_against_brute_force(out)
    assert not any(l.startswith("soup") for l in out.splitlines())


def test_raster_fast_on_triangle_soup_against_brute_force(fuzz_output):
    lines = fuzz_output.splitlines()
    soup = [l for l in lines if l.startswith("soup GROUPS")]
    assert len(soup) == 2
    for g, line in enumerate(soup):
        f = line.split()
        assert f[2] == f"{g}:" and int(f[4]) >= 20000, line
        assert int(f[6]) == 0, "\n".join(l for l in lines if l.startswith("soup"))
        per = line.split("per nsub")[1].split()                # "<nsub>:", cases, "cases", failed, "failed"
        counts = {int(per[i].rstrip(":")): int(per[i + 1]) for i in range(0, len(per), 5)}
        assert sorted(counts) == [1, 2, 4, 8, 16, 32, 64] and all(c > 0 for c in counts.values()), line      # every (nsub, GROUPS) pair
    info = [l for l in lines if l.startswith("soup kinds:")][0]
    kinds = [int(x) for x in info.split("final sets")[0].split()[2:]]
    assert len(kinds) == 10 and all(k > 0 for k in kinds), info
    sets = [int(x) for x in info.split("all):")[1].split()[:5]]
    assert all(s > 0 for s in sets), info
    residues = [int(x) for x in info.split("mod 4:")[1].split()[:4]]
    assert all(r > 0 for r in residues), info
    assert int(info.split("lagging four-line masks:")[1].split()[0]) > 0 and int(info.split("pixels painted:")[1]) > 100000, info


@pytest.mark.parametrize("cell,name", rl.CASES)
def test_frames_with_vertices_on_pixel_centres(fuzz_output, oracle, luts, cell, name):
    """(`fuzz_output`: after a child that did not finish, no frame is started either.)"""
    from vulkan_forge_amd import cabi
    cabi.load()
    EXACT = 0
    u = rl.uniforms(cell, name)
    G, lut = rl.GRID[cell], luts["viridis"]
    ref_rgba, ref_vis = oracle.render_terrain(u, rl.W, rl.H, G, oracle.SPIKE_DUMMY_HEIGHT, lut)
    assert (ref_vis != 0).mean() > 0.3
    t = cabi.Terrain(rl.W, rl.H, G, lut)
    try:
        t.set_uniforms(u)
        t.render()
        fast, vis_fast = t.read_rgba(), t.read_visibility()
        t.set_shade_precision(EXACT)
        t.render()
        rgba, vis = t.read_rgba(), t.read_visibility()
    finally:
        t.close()
    # as assert_parity of tests/test_gpu_parity.py: identical visibility, EXACT colour equal, FAST colour within 1 LSB of the oracle
    assert vis.shape == ref_vis.shape and rgba.shape == ref_rgba.shape
    bad = int((vis != ref_vis).sum())
    assert bad == 0, f"visibility differs at {bad} pixels"
    assert np.array_equal(vis_fast, vis)
    d = int(np.abs(rgba.astype(np.int16) - ref_rgba.astype(np.int16)).max(initial=0))
    assert d == 0, f"EXACT RGBA differs from the oracle by {d} LSB"
    df = int(np.abs(fast.astype(np.int16) - ref_rgba.astype(np.int16)).max(initial=0))
    assert df <= 1, f"fast fragment path differs from the oracle by {df} LSB"
