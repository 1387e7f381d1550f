"""The shared assertions of tests/support.py and tests/abi_support.py fail when they should (no GPU): an assertion that moved into a
helper must not have turned into a no-op on the way."""
import ctypes
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_support as abi
import support

F = np.float32


def field():
    a = np.linspace(-1, 1, 12, dtype=F).reshape(3, 4)
    a[0, 1], a[2, 3] = np.nan, -0.0
    return a


# ---- support.assert_field ----

def test_assert_field_passes_for_equal_arrays_with_nan_and_negative_zero():
    support.assert_field(field(), field(), "equal")


def test_assert_field_sees_one_mantissa_bit_in_one_vertex():
    b = field()
    support.bits(b)[1, 2] ^= 1
    with pytest.raises(AssertionError, match=r"one bit: 1 vertices differ, first at \[\[1, 2\]\]"):
        support.assert_field(b, field(), "one bit")


def test_assert_field_tells_the_zeros_apart():
    a, b = np.zeros((2, 2), F), np.zeros((2, 2), F)
    b[1, 0] = -0.0
    assert (a == b).all()
    with pytest.raises(AssertionError, match=r"\[\[1, 0\]\]"):
        support.assert_field(b, a, "zeros")


def test_assert_field_tells_nan_payloads_apart():
    a, b = np.zeros(3, F), np.zeros(3, F)
    support.bits(a)[1], support.bits(b)[1] = 0x7FC00000, 0x7FC00001
    assert np.isnan(a[1]) and np.isnan(b[1])
    with pytest.raises(AssertionError, match="1 vertices differ"):
        support.assert_field(b, a, "payloads")


def test_assert_field_refuses_another_dtype_or_shape():
    with pytest.raises(AssertionError, match="float64"):
        support.assert_field(np.ones((3, 4), np.float64), np.ones((3, 4), F), "dtype")
    with pytest.raises(AssertionError, match=r"\(4, 3\)"):
        support.assert_field(np.ones((4, 3), F), np.ones((3, 4), F), "shape")


# ---- support.assert_frame ----

def test_assert_frame_names_the_pixel_of_one_differing_byte():
    want = np.arange(5 * 7 * 4, dtype=np.uint8).reshape(5, 7, 4)
    support.assert_frame(want.copy(), want, "equal")
    got = want.copy()
    got[3, 5, 2] ^= 1
    with pytest.raises(AssertionError, match=r"one byte: 1 pixels differ, first at \[\[3, 5\]\]"):
        support.assert_frame(got, want, "one byte")


# ---- the oracle cache's key, and what a cache hands out ----

def test_the_height_digest_reads_the_whole_field():
    a = np.zeros((8, 8), F)
    b = a.copy()
    b[7, 7] = 1.0
    assert a.tobytes()[:64] == b.tobytes()[:64]
    assert support.digest(a) != support.digest(b) and support.digest(a) == support.digest(a.copy())
    assert support.digest(a) != support.digest(a.reshape(4, 16))
    u = np.zeros(44, F)
    assert support.oracle_key(u, 8, 8, 8, a) != support.oracle_key(u, 8, 8, 8, b)
    assert support.oracle_key(u, 8, 8, 8, a) == support.oracle_key(u.copy(), 8, 8, 8, a.copy())
    assert support.oracle_key(u, 8, 8, 8, a) != support.oracle_key(u, 8, 8, 8, a, "spec_t32")


def test_what_a_cache_hands_out_is_read_only():
    class Result:
        def __init__(self):
            self.depth, self.n = np.zeros(3, F), 3
    rgba, vis = support.frozen((np.zeros((2, 2, 4), np.uint8).reshape(2, 2, 4), np.zeros((2, 2), np.uint32)))
    r, d = support.frozen(Result()), support.frozen({"samples": np.zeros(2, F)})
    for a in (rgba, vis, r.depth, d["samples"]):
        assert not a.flags.writeable
        with pytest.raises(ValueError, match="read-only"):
            a[...] = 1


# ---- abi_support, against doctored copies of the header ----

CALLS = {"vf_terrain_set_shadows": ["t", "enable", "strength", "softness", "bias"], "vf_terrain_read_shadow_field": ["t", "lit"]}
DECLARATION = r"int\s+vf_terrain_read_shadow_field\s*\([^)]*\)\s*;"


def test_check_entry_points_holds_on_the_header_and_sees_a_renamed_parameter():
    text = abi.header_text()
    abi.check_entry_points(CALLS)
    abi.check_entry_points(CALLS, text)
    with pytest.raises(AssertionError, match="vf_terrain_set_shadows"):
        abi.check_entry_points(CALLS, re.sub(r"(vf_terrain_set_shadows\s*\([^)]*)\bsoftness\b", r"\1softening", abi.code(text)))
    with pytest.raises(AssertionError, match="vf_terrain_read_shadow_field"):
        abi.check_entry_points({**CALLS, "vf_terrain_read_shadow_field": ["t", "lit", "stream"]}, text)


def test_prototypes_miss_a_removed_declaration_and_one_that_stands_in_a_comment_only():
    src = abi.code()
    assert len(re.findall(DECLARATION, src)) == 1
    for doctored in (re.sub(DECLARATION, "", src), re.sub("(" + DECLARATION + ")", r"/* \1 */", src)):
        with pytest.raises(AssertionError, match="vf_terrain_read_shadow_field is not declared in include/vf_hip.h"):
            abi.prototypes(CALLS, doctored)
        with pytest.raises(AssertionError, match="vf_terrain_read_shadow_field is not declared in include/vf_hip.h"):
            abi.check_entry_points(CALLS, doctored)


def test_check_defines_wants_the_whole_value():
    text = "#define VF_SHADOW_BIAS 0.002f\n#define VF_FLOOD_SEEDS 2   /* a mode */\n#define VF_X_MAX 65535u"
    abi.check_defines("SHADOW", (("BIAS", "0.002f"),), text)
    abi.check_defines("FLOOD", (("SEEDS", 2),), text)
    abi.check_defines("X", (("MAX", "65535u"),), text)
    for prefix, pair in (("SHADOW", ("BIAS", "0.003f")), ("SHADOW", ("BIAS", "0.002")), ("X", ("MAX", "6553")), ("FLOOD", ("SEEDS", 1)), ("FLOOD", ("EDGES", 1))):
        with pytest.raises(AssertionError, match=f"VF_{prefix}_{pair[0]}"):
            abi.check_defines(prefix, (pair,), text)


class Info(ctypes.Structure):
    _fields_ = [("enabled", ctypes.c_int32), ("count", ctypes.c_uint32), ("rgba", ctypes.c_uint8 * 4), ("level", ctypes.c_float)]


def test_check_info_struct_sees_swapped_fields_and_a_wrong_size():
    text = "typedef struct vf_x_info {\n    int32_t enabled; uint32_t count;   /* how many */\n    uint8_t rgba[4];\n    float level;\n} vf_x_info;"
    assert abi.check_info_struct("vf_x_info", Info, 16, text) == ["enabled", "count", "rgba", "level"]
    with pytest.raises(AssertionError, match="vf_x_info"):
        abi.check_info_struct("vf_x_info", Info, 16, text.replace("int32_t enabled; uint32_t count;", "uint32_t count; int32_t enabled;"))
    with pytest.raises(AssertionError, match="vf_x_info"):
        abi.check_info_struct("vf_x_info", Info, 20, text)


def test_check_header_documents_misses_a_paragraph_and_a_phrase():
    text = "/* the x pass: what it is for\n * vf_x_set: sets it, or VF_ERR_INVALID\n * vf_x_read: reads\n * it back */\nint vf_x_set(void);\n/* the next pass\n * vf_x_clear: clears */"
    abi.check_header_documents("the x pass", ["vf_x_set", "vf_x_read"], ["VF_ERR_INVALID", "reads\n * it back"], text)
    with pytest.raises(AssertionError, match="vf_x_stage has no paragraph"):
        abi.check_header_documents("the x pass", ["vf_x_set", "vf_x_stage"], [], text)
    with pytest.raises(AssertionError, match="survives"):
        abi.check_header_documents("the x pass", ["vf_x_set"], ["VF_ERR_INVALID", "survives"], text)
    abi.check_header_documents("the x pass", ["vf_x_clear"], [], text)
    with pytest.raises(AssertionError, match="vf_x_clear has no paragraph"):
        abi.check_header_documents("the x pass", ["vf_x_clear"], [], text, until="int vf_x_set")
    with pytest.raises(AssertionError, match="the y pass"):
        abi.check_header_documents("the y pass", [], [], text)


# ---- support.run_check ----

def child(tmp_path, body):
    p = tmp_path / "child_check.py"
    p.write_text(body)
    return str(p)


def test_run_check_wants_the_marker_the_exit_status_and_an_end(tmp_path):
    support.run_check(child(tmp_path, "import sys\nprint('CHILD OK', sys.argv[1])"), "CHILD OK 7", args=("7",))
    with pytest.raises(AssertionError, match="no marker here"):
        support.run_check(child(tmp_path, "print('no marker here')"), "CHILD OK")
    with pytest.raises(AssertionError, match="CHILD OK"):
        support.run_check(child(tmp_path, "import sys\nprint('CHILD OK')\nsys.exit(1)"), "CHILD OK")
    with pytest.raises(subprocess.TimeoutExpired):
        support.run_check(child(tmp_path, "import time\nprint('CHILD OK', flush=True)\ntime.sleep(30)"), "CHILD OK", timeout=1)


# ---- importing the helpers imports nothing native ----

def test_importing_the_helpers_imports_nothing_native():
    code = ("import importlib, sys, support, abi_support\n"
            "print([m for m in ('oracle', 'vulkan_forge', 'vulkan_forge_amd', 'torch') if m in sys.modules])\n"
            "before = list(sys.path); importlib.reload(support)\n"
            "print(sys.path == before, sys.path.count(support.ROOT), sorted({sys.path.count(p) for p in sys.path if p.endswith('_model')}))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60, cwd=support.HERE)
    assert r.returncode == 0 and r.stdout.split("\n")[:2] == ["[]", "True 1 [1]"], (r.stdout, r.stderr[-2000:])
