"""Sun exposure without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the header
documents them, the Python methods exist on both classes with the documented signatures, and the argument rules refuse what they
should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_sun_exposure": ["t", "enable", "suns_xyz", "weights", "count", "incidence", "softness", "bias", "high_rgba", "low_rgba"],
                "vf_terrain_clear_sun_exposure": ["t"],
                "vf_terrain_read_sun_exposure_field": ["t", "exposure"],
                "vf_terrain_sun_exposure_field_device": ["t", "dev_exposure", "stream"],
                "vf_terrain_sun_exposure_info": ["t", "out"],
                "vf_terrain_debug_sun_exposure_batch": ["t", "batch"],
                "vf_terrain_debug_sun_exposure_scans": ["t", "count"],
                "vf_terrain_debug_sun_exposure_stage": ["t", "repeats", "ms"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import cabi
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("SUN_EXPOSURE", (("MAX_SUNS", "65535u"), ("HIGH_RGBA", "0xA040D0FFu"), ("LOW_RGBA", "0x00000000u")))
    assert 0xA040D0FF == 255 | 208 << 8 | 64 << 16 | 160 << 24
    fields = abi.check_info_struct("vf_sun_exposure_info", cabi.SunExposureInfo, 4 * 8 + 8)
    assert fields == ["enabled", "count", "counted", "weight_total", "incidence", "batch", "softness", "bias", "high_rgba", "low_rgba"]


def test_the_header_documents_the_calls():
    abi.check_header_documents("sun exposure: the weighted sum of the shadow fields of N suns", list(ENTRY_POINTS)[:5],
                               ("DESIGN.md 4n", "VF_ERR_INVALID", "whether or not sun exposure is enabled", "NULL: the context's", "1 <= count <= 65535",
                                "rint(lit * c * w * 65536)", "is not counted", "weights in\n * [0, 1]", "or NULL: all 1"))


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    out = np.zeros(4, np.float32)
    xyz, w, col = np.ones((2, 3), np.float32), np.ones(2, np.float32), (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    abi.check_null_refusals([("vf_terrain_set_sun_exposure", (1, xyz.ctypes.data, w.ctypes.data, 2, 0, 0.02, 0.002, col, col)),
                             ("vf_terrain_clear_sun_exposure", ()),
                             ("vf_terrain_read_sun_exposure_field", (out.ctypes.data,)),
                             ("vf_terrain_sun_exposure_field_device", (None, None)),
                             ("vf_terrain_sun_exposure_info", (ctypes.byref(cabi.SunExposureInfo()),)),
                             ("vf_terrain_debug_sun_exposure_batch", (4,)),
                             ("vf_terrain_debug_sun_exposure_scans", (ctypes.byref(ctypes.c_uint32()),)),
                             ("vf_terrain_debug_sun_exposure_stage", (1, ctypes.byref(ctypes.c_float())))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    abi.check_method_docs(cls, {
        "set_sun_exposure": r"set_sun_exposure\(self: [\w.]+, suns: object, \*, weights: object = None, incidence: object = False, enabled: object = True, "
                            r"softness: object = 0.019\d+, bias: object = 0.002\d*, high_rgba: object = \(255, 208, 64, 160\), "
                            r"low_rgba: object = \(0, 0, 0, 0\)\) -> None",
        "clear_sun_exposure": r"clear_sun_exposure\(self: [\w.]+\) -> None",
        "sun_exposure_field": r"sun_exposure_field\(self: [\w.]+\) -> numpy",
        "sun_exposure_info": r"sun_exposure_info\(self: [\w.]+\) -> object"},
        cabi_methods=("set_sun_exposure", "clear_sun_exposure", "sun_exposure_field", "sun_exposure_field_device", "sun_exposure_info", "sun_exposure_batch",
                      "sun_exposure_scans", "sun_exposure_stage"))


def test_argument_rules():
    from vulkan_forge_amd._sun_exposure import DEFAULTS, MAX_SUNS, sun_exposure_args, sun_exposure_info
    assert MAX_SUNS == 65535
    assert DEFAULTS == {"weights": None, "incidence": False, "softness": 0.02, "bias": 0.002, "high_rgba": (255, 208, 64, 160), "low_rgba": (0, 0, 0, 0)}
    a = sun_exposure_args([(30, 120), (45.5, -90)])
    assert a[0] == 1 and a[3:] == (0, 0.02, 0.002, (255, 208, 64, 160), (0, 0, 0, 0))
    assert a[1].dtype == np.float32 and a[1].shape == (2, 2) and a[1].flags.c_contiguous and a[1].tolist() == [[30.0, 120.0], [45.5, -90.0]]
    assert a[2].dtype == np.float32 and a[2].tolist() == [1.0, 1.0]
    a = sun_exposure_args(np.arange(18, dtype=np.float64).reshape(2, 9)[:, ::3], np.array([0, 1], np.int64), 1, False, 1, 0, [1, 2, 3, 4],
                          np.array([5, 6, 7, 8], np.uint8))
    assert a[0] == 0 and a[1].tolist() == [[0.0, 3.0, 6.0], [9.0, 12.0, 15.0]] and a[1].flags.c_contiguous and a[1].dtype == np.float32
    assert a[2].tolist() == [0.0, 1.0] and a[2].dtype == np.float32 and a[3:] == (1, 1.0, 0.0, (1, 2, 3, 4), (5, 6, 7, 8))
    assert sun_exposure_args(np.ones((MAX_SUNS, 3)))[1].shape == (MAX_SUNS, 3)
    assert sun_exposure_args([(0, 0, 0), (0.5, -0.2, 0.1)])[1].shape == (2, 3)          # (zero and sunken suns are allowed: they are not counted)
    ok = {k: v for k, v in DEFAULTS.items() if k not in ("weights", "incidence")}
    one = [(1.0, 1.0, 0.0)]
    for name, bad, exc, msg in (("softness", 0.0, ValueError, "softness must be > 0"), ("softness", -1.0, ValueError, "softness must be > 0"),
                                ("bias", -1e-9, ValueError, "bias must be >= 0"),
                                ("high_rgba", (1, 2, 3), ValueError, "high_rgba must be 4 ints"), ("low_rgba", (1, 2, 3, 256), ValueError, "low_rgba must be 4 ints"),
                                ("low_rgba", (1, 2, 3, -1), ValueError, "low_rgba must be 4 ints"), ("high_rgba", (1, 2, 3, 4.5), TypeError, "high_rgba must be 4 ints"),
                                ("high_rgba", 7, TypeError, "high_rgba must be 4 ints"), ("softness", "soft", TypeError, "softness must be a number"),
                                ("bias", None, TypeError, "bias must be a number")):
        with pytest.raises(exc, match=msg):
            sun_exposure_args(one, None, False, True, **{**ok, name: bad})
    for name in ("softness", "bias"):
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="must be finite"):
                sun_exposure_args(one, None, False, True, **{**ok, name: bad})
    for bad in ([(float("nan"), 0.0, 1.0)], [(0.0, 1.0, 0.0), (0.0, float("-inf"), 0.0)], [(30.0, float("inf"))], [(1e39, 1.0, 0.0)]):
        with pytest.raises(ValueError, match="suns must be finite"):
            sun_exposure_args(bad)
    for bad in ((0.0, 1.0, 0.0), [(0.0, 0.0, 0.0, 0.0)], [(1.0,)], np.zeros((2, 2, 3))):
        with pytest.raises(ValueError, match=r"suns must be \(N, 2\) angles or \(N, 3\) vectors"):
            sun_exposure_args(bad)
    for bad in (np.zeros((0, 3)), np.zeros((MAX_SUNS + 1, 2))):
        with pytest.raises(ValueError, match="suns must hold 1 to 65535 rows"):
            sun_exposure_args(bad)
    for bad in ([("a", "b")], [(None, 1.0, 0.0)], [(1j, 0.0, 1.0)]):
        with pytest.raises(TypeError, match=r"suns must be \(N, 2\) angles or \(N, 3\) vectors"):
            sun_exposure_args(bad)
    for bad in ([1.0, 1.0], [[1.0]], 1.0, np.ones((1, 1))):
        with pytest.raises(ValueError, match=r"weights must have shape \(1,\)"):
            sun_exposure_args(one, bad)
    for bad in ([-0.01], [1.0001], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match=r"weights must be finite and lie in \[0, 1\]"):
            sun_exposure_args(one, bad)
    for bad in (["w"], [None], [1j]):
        with pytest.raises(TypeError, match=r"weights must be \(N,\) numbers"):
            sun_exposure_args(one, bad)
    assert sun_exposure_args(one, [0.0])[2].tolist() == [0.0] and sun_exposure_args(one, [1])[2].tolist() == [1.0]
    with pytest.raises(TypeError, match="enabled must be a bool"):
        sun_exposure_args(one, None, False, "yes")
    with pytest.raises(TypeError, match="incidence must be a bool"):
        sun_exposure_args(one, None, "cos")
    d = sun_exposure_info(1, 34, 30, 18.5, 1, 16, 0.02, 0.002, (255, 208, 64, 160), (0, 0, 0, 0))
    assert d == {"enabled": True, "suns": 34, "counted": 30, "weight_total": 18.5, "incidence": True, "batch": 16, "softness": 0.02, "bias": 0.002,
                 "high_rgba": (255, 208, 64, 160), "low_rgba": (0, 0, 0, 0)}
    d = sun_exposure_info(0, 0, 0, 0.0, 0, 0, 0.02, 0.002, (1, 2, 3, 4), (5, 6, 7, 8))
    assert d["enabled"] is False and d["incidence"] is False and d["suns"] == 0 and d["high_rgba"] == (1, 2, 3, 4)


def test_the_c_abi_wrapper_takes_vectors_only():
    from vulkan_forge_amd import cabi

    class NoDevice(cabi.Terrain):
        def __init__(self):
            pass

        def __del__(self):
            pass
    with pytest.raises(ValueError, match=r"\(N, 3\) direction vectors"):
        NoDevice().set_sun_exposure([(30.0, 120.0)])
