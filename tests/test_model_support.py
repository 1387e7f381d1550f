"""tests/model_support.py does what the model loaders rely on, and fails when it should (no GPU, gcc only): the sources of every model
are the lists its loader wrote out by hand before, a stale library is rebuilt when a source two includes away is newer, and a call
refuses every array it would have to convert."""
import glob
import os

import numpy as np
import pytest

import model_support as ms

# What every loader wrote out by hand before model_support derived it: the model's C file, then the files it rebuilt the library
# for, as model directory names.  The record of what "unchanged" means for sources().
CHAIN = ["gbuffer_model", "occlusion_model", "polygon_model", "overlay_model"]
SHADOW = ["shadow_model", *CHAIN]
DRAPE = ["drape_model", "ambient_model", *SHADOW]
VIEWSHED = ["viewshed_model", *SHADOW]
SOURCES = {
    "overlay_model": ["overlay_model"],
    "polygon_model": ["polygon_model", "overlay_model"],
    "occlusion_model": ["occlusion_model", "polygon_model", "overlay_model"],
    "contour_model": ["contour_model", "overlay_model"],
    "gbuffer_model": CHAIN,
    "overlay_haze_model": ["overlay_haze_model", "occlusion_model", "polygon_model", "overlay_model"],
    "haze_model": ["haze_model", *CHAIN],
    "shadow_model": SHADOW,
    "ambient_model": ["ambient_model", *SHADOW],
    "drape_model": DRAPE,
    "drape_mip_model": ["drape_mip_model", *DRAPE],
    "drape_aniso_model": ["drape_aniso_model", "drape_mip_model", *DRAPE],
    "viewshed_model": VIEWSHED,
    "flood_model": ["flood_model", *VIEWSHED],
    "spill_model": ["spill_model", *VIEWSHED],
}
# the models whose library is built by model_support.load (tests/walk_model builds the oracle's C with flags of its own)
LOADED = sorted(os.path.basename(os.path.dirname(p)) for p in glob.glob(os.path.join(ms.HERE, "*_model", "*.c")) if "walk_model" not in p)


def test_every_model_with_a_c_file_has_its_recorded_sources():
    assert LOADED == sorted(SOURCES)


@pytest.mark.parametrize("name", sorted(SOURCES))
def test_sources_are_the_list_the_loader_wrote_out(name):
    assert ms.sources(name) == [os.path.join(ms.HERE, m, m + ".c") for m in SOURCES[name]]


# ---- made-up models: a includes b includes c ----

A = ('#include "../b_model/b_model.c"\n#include <stdint.h>\n'
     "int a_scale(float *out, const float *in, uint32_t n) { if (!out || !in) return -1; for (uint32_t k = 0; k < n; ++k) out[k] = in[k] * b_two(); return 0; }\n"
     "int a_count(const float *in, uint32_t n) { return in ? (int)n : -1; }\n")
B = '  #  include "../c_model/c_model.c"\nstatic float b_two(void) { return c_one() + c_one(); }\n'
C_ = "/* #include \"../d_model/d_model.c\" is only a comment's text on a line of code */ static float c_one(void) { return 1.0f; }\n"
SIGNATURES = {"a_scale": "i32(f32*, f32*, u32)", "a_count": "i32(f32*?, u32)"}


@pytest.fixture()
def made_up(tmp_path):
    """-> (the path of a_model.c, a build directory), with an empty library cache for the test"""
    for name, text in (("a", A), ("b", B), ("c", C_)):
        d = tmp_path / f"{name}_model"
        d.mkdir()
        (d / f"{name}_model.c").write_text(text)
    saved = dict(ms._loaded)
    ms._loaded.clear()
    yield str(tmp_path / "a_model" / "a_model.c"), str(tmp_path / "build")
    ms._loaded.clear()
    ms._loaded.update(saved)


def test_sources_follow_the_includes_of_the_files_themselves(made_up, tmp_path):
    src, _ = made_up
    assert ms.sources(src) == [str(tmp_path / f"{m}_model" / f"{m}_model.c") for m in "abc"]


def test_a_library_is_rebuilt_when_a_source_two_includes_away_is_newer_and_not_otherwise(made_up, tmp_path):
    src, build = made_up
    out = os.path.join(build, "liba_model.so")
    lib = ms.load(src, SIGNATURES, build_dir=build)
    assert ms.load(src, SIGNATURES, build_dir=build) is lib           # one library per process
    first = os.stat(out)
    ms._loaded.clear()
    ms.load(src, SIGNATURES, build_dir=build)
    assert (os.stat(out).st_mtime_ns, os.stat(out).st_ino) == (first.st_mtime_ns, first.st_ino), "nothing touched: not rebuilt"
    later = first.st_mtime_ns + 5 * 10**9
    os.utime(tmp_path / "c_model" / "c_model.c", ns=(later, later))
    ms._loaded.clear()
    ms.load(src, SIGNATURES, build_dir=build)
    assert os.stat(out).st_mtime_ns != first.st_mtime_ns and os.stat(out).st_ino != first.st_ino, "the grandparent source is newer: rebuilt"
    assert not [f for f in os.listdir(build) if f.endswith(".tmp")]


def test_a_call_takes_exact_arrays_and_writes_through_them(made_up):
    src, build = made_up
    lib = ms.load(src, SIGNATURES, build_dir=build)
    a, out = np.arange(6, dtype=np.float32), np.full(6, -1, np.float32)
    assert lib.a_scale(out, a, 6) == 0
    assert (out == 2 * a).all()
    ro = a.copy()
    ro.setflags(write=False)                                           # (what a cache hands out: read-only is no reason to copy)
    assert lib.a_scale(out, ro, 6) == 0


@pytest.mark.parametrize("what, bad", [("float64", lambda a: a.astype(np.float64)), ("strided", lambda a: np.repeat(a, 2)[::2]),
                                        ("list", lambda a: a.tolist()), ("None", lambda a: None), ("address", lambda a: a.ctypes.data)])
def test_a_call_refuses_what_it_would_have_to_convert_and_leaves_the_output(made_up, what, bad):
    src, build = made_up
    lib = ms.load(src, SIGNATURES, build_dir=build)
    a, out = np.arange(6, dtype=np.float32), np.full(6, -1, np.float32)
    arg = bad(a)
    if what == "strided":
        assert (arg == a).all() and not arg.flags.c_contiguous
    with pytest.raises(TypeError, match=r"a_scale parameter 1\b"):
        lib.a_scale(out, arg, 6)
    assert (out == -1).all()
    with pytest.raises(TypeError, match=r"a_scale parameter 0\b"):     # the output pointer is held to the same rule
        lib.a_scale(out.astype(np.float64), a, 6)
    with pytest.raises(TypeError, match="a_scale: takes 3 arguments, got 2"):
        lib.a_scale(out, a)


def test_none_passes_only_where_the_signature_marks_it(made_up):
    src, build = made_up
    lib = ms.load(src, SIGNATURES, build_dir=build)
    assert lib.a_count(None, 4) == -1 and lib.a_count(np.zeros(4, np.float32), 4) == 4
    with pytest.raises(TypeError, match=r"a_count parameter 0\b"):
        lib.a_count(np.zeros(4, np.float64), 4)


def test_a_signature_for_a_function_the_library_lacks_fails_at_load(made_up):
    src, build = made_up
    with pytest.raises(AttributeError, match="a_missing"):
        ms.load(src, {**SIGNATURES, "a_missing": "void(f32*)"}, build_dir=build)
    assert not ms._loaded                                              # (and leaves no half-declared library behind)


def test_a_record_pointer_goes_by_the_item_size():
    import overlay_model as om
    p = ms.Pointer("rec48*")
    recs = np.zeros(3, om.OVIN)
    assert p.address(recs, "x") == recs.ctypes.data
    for bad in (np.zeros(3 * 48, np.uint8), np.zeros((3, 12), np.float32), recs[::2], None):
        with pytest.raises(TypeError, match="x: wants rec48"):
            p.address(bad, "x")


# ---- one pack ----

def test_the_three_packs_are_one():
    import haze_model as hzm
    import overlay_model as om
    import viewshed_model as vsm
    assert hzm.pack is vsm.pack is om._rgba_word is ms.pack
    for rgba, word in (((0, 0, 0, 0), 0), ((255, 0, 0, 0), 0xFF), ((0, 0, 0, 255), 0xFF000000), ((255, 255, 255, 255), 0xFFFFFFFF),
                       ((1, 2, 3, 4), 0x04030201)):
        assert hzm.pack(rgba) == vsm.pack(rgba) == om._rgba_word(rgba) == word
        assert om._rgba_word(np.array(rgba, np.uint8)) == word            # (the layers hand it rows of a uint8 array)


# ---- the shared opening lines ----

def test_frame_hands_out_a_copy_and_the_scene_in_the_c_order():
    rgba = np.arange(3 * 5 * 4, dtype=np.uint8)                        # flat, as the oracle returns it
    vis = np.arange(15, dtype=np.int64).reshape(3, 5)
    u = np.arange(44, dtype=np.float64)
    out, v, W, H, u44, tex, tw, th = ms.frame(rgba, vis, u, np.zeros((7, 9)))
    assert out.shape == (3, 5, 4) and out.flags.writeable and not np.shares_memory(out, rgba) and (out.ravel() == rgba).all()
    assert v.dtype == np.uint32 and v.flags.c_contiguous and (W, H) == (5, 3)
    assert u44.dtype == np.float32 and u44.shape == (44,) and tex.dtype == np.float32 and (tw, th) == (9, 7)
    assert ms.frame(None, vis, u, np.zeros((7, 9)))[0] is None
    with pytest.raises(ValueError):
        ms.u44(np.zeros(43))
