"""ctypes view of the C-ABI (include/vf_hip.h) -- for callers that own device memory and streams
(bench.py, the torch.distributed shard driver, the C-ABI tests).  The drop-in Python classes live in
the compiled `_vulkan_forge` module; this file only declares the same entry points for ctypes.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.environ.get("VF_HIP_LIB") or os.path.join(_HERE, "libvf_hip.so")     # override: kernel experiments only

VF_OK, VF_ERR_NO_DEVICE, VF_ERR_HIP, VF_ERR_INVALID, VF_ERR_NOMEM = 0, -1, -2, -3, -4
VF_DRAPE_SIZE_MAX, VF_DRAPE_NEAREST, VF_DRAPE_LINEAR = 16384, 0, 1                       # a draped image layer
VF_DRAPE_MIP_BIAS_MAX, VF_DRAPE_MIP_LEVELS_MAX = 16.0, 15                                # its mip pyramid
VF_DRAPE_ANISOTROPY_MAX = 16                                                             # anisotropic taps through it
VF_SUPERSAMPLE_MAX = 4                                                                   # supersampled terrain frames
VF_PLAN_FIRST, VF_PLAN_FRESH, VF_PLAN_MOTION_MAP, VF_PLAN_DILATE, VF_PLAN_QUEUED_AHEAD = 1, 2, 4, 8, 16   # vf_terrain_debug_plan_mode
VF_PLAN_TILE_LISTS = 64        # ... and for "the tile kernel read the plan state's per-tile candidate lists" (DESIGN.md 3): Terrain.tile_lists()
VF_PLAN_GEOMETRY_REUSED = 32   # ... its bit for "the block boxes and set-up records were not rebuilt" (DESIGN.md 3): Terrain.geometry_reused()

class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 256), ("arch", C.c_char * 64), ("device_ordinal", C.c_int32), ("compute_units", C.c_int32),
                ("wavefront_size", C.c_int32), ("clock_khz", C.c_int32), ("total_mem_bytes", C.c_uint64),
                ("lds_bytes_per_cu", C.c_uint64), ("pci_bus_id", C.c_int32), ("pci_device_id", C.c_int32)]


class Timings(C.Structure):
    _fields_ = [("ranges_ms", C.c_float), ("plan_ms", C.c_float), ("tile_ms", C.c_float), ("total_ms", C.c_float),
                ("blocks_rasterised", C.c_uint32), ("tiles", C.c_uint32), ("frames", C.c_uint32), ("blocks_distinct", C.c_uint32)]


class FragmentTiming(C.Structure):
    _fields_ = [("resolve_ms", C.c_float), ("covered_pixels", C.c_uint32), ("repeats", C.c_uint32), ("equal_to_frame", C.c_uint32)]


class ViewshedInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("has_observer", C.c_int32), ("vertex", C.c_uint32 * 2), ("observer_xyz", C.c_float * 3), ("eye_y", C.c_float),
                ("eye_height", C.c_float), ("target_height", C.c_float), ("radius", C.c_float), ("softness", C.c_float), ("bias", C.c_float),
                ("visible_rgba", C.c_uint8 * 4), ("hidden_rgba", C.c_uint8 * 4)]


class CumulativeViewshedInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("count", C.c_uint32), ("batch", C.c_uint32), ("eye_height", C.c_float), ("target_height", C.c_float),
                ("radius", C.c_float), ("softness", C.c_float), ("bias", C.c_float), ("high_rgba", C.c_uint8 * 4), ("low_rgba", C.c_uint8 * 4)]


class SunExposureInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("count", C.c_uint32), ("counted", C.c_uint32), ("weight_total", C.c_float), ("incidence", C.c_int32),
                ("batch", C.c_uint32), ("softness", C.c_float), ("bias", C.c_float), ("high_rgba", C.c_uint8 * 4), ("low_rgba", C.c_uint8 * 4)]


class HazeInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("background", C.c_int32), ("density", C.c_float), ("start", C.c_float), ("falloff", C.c_float),
                ("base", C.c_float), ("max_opacity", C.c_float), ("rgba", C.c_uint8 * 4), ("has_eye", C.c_int32), ("eye_y", C.c_float)]


class FloodInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("has_flood", C.c_int32), ("mode", C.c_int32), ("count", C.c_uint32), ("level", C.c_float),
                ("depth_full", C.c_float), ("shallow_rgba", C.c_uint8 * 4), ("deep_rgba", C.c_uint8 * 4), ("flooded_vertices", C.c_uint32),
                ("wettable_vertices", C.c_uint32), ("passes", C.c_uint32), ("scans", C.c_uint32), ("group", C.c_uint32)]


class SpillInfo(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("has_spill", C.c_int32), ("mode", C.c_int32), ("count", C.c_uint32), ("depth_full", C.c_float),
                ("shallow_rgba", C.c_uint8 * 4), ("deep_rgba", C.c_uint8 * 4), ("reached_vertices", C.c_uint32), ("sink_vertices", C.c_uint32),
                ("passes", C.c_uint32), ("scans", C.c_uint32), ("group", C.c_uint32), ("tile_runs", C.c_uint32)]


DIST_UNIQUE_ID_BYTES = 128
_vp, _u32, _f, _i = C.c_void_p, C.c_uint32, C.c_float, C.c_int
_PROTOS = {
    "vf_last_error": (C.c_char_p, []),
    "vf_device_count": (_i, [C.POINTER(_i)]),
    "vf_device_query": (_i, [_i, C.POINTER(DeviceInfo)]),
    "vf_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "vf_ctx_destroy": (None, [_vp]),
    "vf_ctx_device_info": (_i, [_vp, C.POINTER(DeviceInfo)]),
    "vf_ctx_stream": (_i, [_vp, C.POINTER(_vp)]),
    "vf_terrain_create": (_i, [_vp, _u32, _u32, _u32, _vp, _i, C.POINTER(_vp)]),
    "vf_terrain_destroy": (None, [_vp]),
    "vf_terrain_set_uniforms": (_i, [_vp, _vp]),
    "vf_terrain_set_height": (_i, [_vp, _vp, _u32, _u32]),
    "vf_terrain_set_height_device": (_i, [_vp, _vp, _u32, _u32]),
    "vf_terrain_set_shade_mode": (_i, [_vp, _i]),
    "vf_terrain_set_shade_precision": (_i, [_vp, _i]),
    "vf_terrain_set_raster_groups": (_i, [_vp, _i]),
    "vf_terrain_raster_groups": (_i, [_vp, C.POINTER(_i), _vp]),
    "vf_terrain_set_shard": (_i, [_vp, _u32, _u32, _u32]),
    "vf_terrain_local_rows": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_set_tile_shard": (_i, [_vp, _u32, _u32, _u32]),
    "vf_terrain_add_points": (_i, [_vp, _vp, _u32, _vp, _vp, _f, _vp, _i, _i, C.POINTER(_u32)]),
    "vf_terrain_add_lines": (_i, [_vp, _vp, _vp, _u32, _f, _vp, _i, _i, C.POINTER(_u32)]),
    "vf_terrain_add_polygons": (_i, [_vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _f, _i, C.POINTER(_u32)]),
    "vf_terrain_set_layer_occlusion": (_i, [_vp, _u32, _i, _f]),
    "vf_terrain_set_layer_haze": (_i, [_vp, _u32, _i]),
    "vf_terrain_layer_haze": (_i, [_vp, _u32, C.POINTER(C.c_int)]),
    "vf_terrain_add_contours": (_i, [_vp, _vp, _u32, _f, _vp, _f, _i, _i, _f, C.POINTER(_u32), C.POINTER(_u32)]),
    "vf_terrain_height_bounds": (_i, [_vp, C.POINTER(_f), C.POINTER(_f)]),
    "vf_terrain_layer_primitive_count": (_i, [_vp, _u32, C.POINTER(_u32)]),
    "vf_terrain_clear_overlays": (_i, [_vp]),
    "vf_terrain_local_tiles": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_read_tiles": (_i, [_vp, _vp, _u32, _u32]),
    "vf_tile_layout": (_i, [_u32, _u32, _u32, _u32, _u32, _vp, _u32, C.POINTER(_u32)]),
    "vf_terrain_set_output_device": (_i, [_vp, _vp]),
    "vf_terrain_rgba_device": (_i, [_vp, C.POINTER(_vp)]),
    "vf_terrain_render": (_i, [_vp, _vp]),
    "vf_terrain_render_batch": (_i, [_vp, _vp, _u32, _vp, _vp]),
    "vf_terrain_render_batch_host": (_i, [_vp, _vp, _u32, _vp]),
    "vf_terrain_sync": (_i, [_vp]),
    "vf_terrain_read_rgba": (_i, [_vp, _vp, _u32, _u32]),
    "vf_terrain_read_png_scanlines": (_i, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "vf_terrain_read_visibility": (_i, [_vp, _vp]),
    "vf_terrain_enable_timing": (_i, [_vp, _i]),
    "vf_terrain_timings": (_i, [_vp, C.POINTER(Timings)]),
    "vf_terrain_frame_times": (_i, [_vp, _vp, _vp, _u32, C.POINTER(_u32)]),
    "vf_terrain_debug_item_stats": (_i, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "vf_terrain_debug_band_masks": (_i, [_vp, _vp, _vp, _vp, _u32, C.POINTER(_u32)]),
    "vf_terrain_debug_set_plan_feedback": (_i, [_vp, _vp, _vp, _vp, _u32]),
    "vf_terrain_debug_plan_mode": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_debug_tile_lists": (_i, [_vp, _vp]),
    "vf_terrain_debug_set_tile_list_capacity": (_i, [_vp, _u32]),
    "vf_terrain_debug_phase_cycles": (_i, [_vp, _vp, _u32]),
    "vf_terrain_tile_times": (_i, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "vf_balance_stripes": (_i, [_vp, _u32, _u32, _vp]),
    "vf_tile_layout_register_map": (_i, [_vp, _u32, _u32, _u32, C.POINTER(_u32)]),
    "vf_host_alloc": (_i, [C.c_size_t, C.POINTER(_vp)]),
    "vf_host_free": (None, [_vp]),
    "vf_grid_generate": (_i, [_vp, _u32, _u32, _f, _f, _vp, _vp, _vp]),
    "vf_grid_generate_device": (_i, [_vp, _u32, _u32, _f, _f, _vp, _vp, _vp, _vp]),
    "vf_triangle_render": (_i, [_vp, _u32, _u32, _vp]),
    "vf_stitch_bands_device": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp]),
    "vf_stitch_tiles_device": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp]),
    "vf_dist_available": (_i, []),
    "vf_dist_version": (_i, [C.POINTER(_i)]),
    "vf_dist_unique_id": (_i, [_vp]),
    "vf_dist_comm_init": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "vf_dist_comm_destroy": (None, [_vp]),
    "vf_dist_gather_tiles": (_i, [_vp, _vp, _i, _vp, _u32, _vp]),
    "vf_dist_gather_bands": (_i, [_vp, _vp, _i, _vp, _vp]),
    "vf_dist_exchange_bands": (_i, [_vp, _vp, _i, _vp, _vp]),
    "vf_terrain_debug_fragment_stage": (_i, [_vp, _u32, C.POINTER(FragmentTiming)]),
    "vf_terrain_gbuffer_device": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "vf_terrain_read_gbuffer": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "vf_terrain_pick": (_i, [_vp, _vp, _u32, _vp]),
    "vf_terrain_debug_gbuffer_stage": (_i, [_vp, _u32, _u32, C.POINTER(_f)]),
    "vf_terrain_set_shadows": (_i, [_vp, _i, _f, _f, _f]),
    "vf_terrain_read_shadow_field": (_i, [_vp, _vp]),
    "vf_terrain_shadow_field_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_debug_shadow_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_debug_shadow_scans": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_set_ambient": (_i, [_vp, _i, _f, _f, _u32, _vp]),
    "vf_terrain_read_sky_view_field": (_i, [_vp, _vp]),
    "vf_terrain_sky_view_field_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_debug_ambient_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_debug_ambient_scans": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_set_drape": (_i, [_vp, _vp, _u32, _u32, _u32, C.POINTER(_f), _f, _i]),
    "vf_terrain_set_drape_device": (_i, [_vp, _vp, _u32, _u32, C.POINTER(_f), _f, _i, _vp]),
    "vf_terrain_clear_drape": (_i, [_vp]),
    "vf_terrain_drape_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "vf_terrain_debug_drape_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_set_drape_mips": (_i, [_vp, _i, _f]),
    "vf_terrain_drape_mip_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_u32), C.POINTER(_f), C.POINTER(C.c_uint64), C.POINTER(_u32)]),
    "vf_terrain_read_drape_level": (_i, [_vp, _u32, _vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "vf_terrain_debug_drape_mip_build": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_set_drape_anisotropy": (_i, [_vp, _u32]),
    "vf_terrain_drape_anisotropy": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_set_viewshed": (_i, [_vp, _i, C.POINTER(_f), _f, _f, _f, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _f, _f]),
    "vf_terrain_read_viewshed_field": (_i, [_vp, _vp]),
    "vf_terrain_viewshed_field_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_viewshed_info": (_i, [_vp, C.POINTER(ViewshedInfo)]),
    "vf_terrain_debug_viewshed_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_debug_viewshed_scans": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_set_cumulative_viewshed": (_i, [_vp, _i, _vp, _u32, _f, _f, _f, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _f, _f]),
    "vf_terrain_read_cumulative_viewshed_field": (_i, [_vp, _vp]),
    "vf_terrain_cumulative_viewshed_field_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_cumulative_viewshed_info": (_i, [_vp, C.POINTER(CumulativeViewshedInfo)]),
    "vf_terrain_read_cumulative_viewshed_vertices": (_i, [_vp, _vp]),
    "vf_terrain_debug_cumulative_viewshed_batch": (_i, [_vp, _u32]),
    "vf_terrain_debug_cumulative_viewshed_scans": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_debug_cumulative_viewshed_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_set_sun_exposure": (_i, [_vp, _i, _vp, _vp, _u32, _i, _f, _f, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "vf_terrain_clear_sun_exposure": (_i, [_vp]),
    "vf_terrain_read_sun_exposure_field": (_i, [_vp, _vp]),
    "vf_terrain_sun_exposure_field_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_sun_exposure_info": (_i, [_vp, C.POINTER(SunExposureInfo)]),
    "vf_terrain_debug_sun_exposure_batch": (_i, [_vp, _u32]),
    "vf_terrain_debug_sun_exposure_scans": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_debug_sun_exposure_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_create_supersampled": (_i, [_vp, _u32, _u32, _u32, _vp, _i, _u32, C.POINTER(_vp)]),
    "vf_terrain_supersampling": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "vf_terrain_read_samples": (_i, [_vp, _vp]),
    "vf_terrain_samples_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_debug_resolve_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_set_haze": (_i, [_vp, _i, _f, C.POINTER(C.c_uint8), _f, _f, _f, _f, _i]),
    "vf_terrain_clear_haze": (_i, [_vp]),
    "vf_terrain_haze_info": (_i, [_vp, C.POINTER(HazeInfo)]),
    "vf_terrain_read_haze_opacity": (_i, [_vp, _vp]),
    "vf_terrain_haze_opacity_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_debug_haze_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_set_flood": (_i, [_vp, _i, _f, _i, _vp, _u32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _f]),
    "vf_terrain_clear_flood": (_i, [_vp]),
    "vf_terrain_read_flood_field": (_i, [_vp, _vp]),
    "vf_terrain_flood_field_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_flood_info": (_i, [_vp, C.POINTER(FloodInfo)]),
    "vf_terrain_read_flood_seeds": (_i, [_vp, _vp]),
    "vf_terrain_debug_flood_scans": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_debug_flood_group": (_i, [_vp, _u32]),
    "vf_terrain_debug_flood_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_terrain_set_spill": (_i, [_vp, _i, _i, _vp, _u32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _f]),
    "vf_terrain_clear_spill": (_i, [_vp]),
    "vf_terrain_read_spill_field": (_i, [_vp, _vp]),
    "vf_terrain_spill_field_device": (_i, [_vp, _vp, _vp]),
    "vf_terrain_read_sink_depth": (_i, [_vp, _vp]),
    "vf_terrain_spill_info": (_i, [_vp, C.POINTER(SpillInfo)]),
    "vf_terrain_read_spill_seeds": (_i, [_vp, _vp]),
    "vf_terrain_debug_spill_scans": (_i, [_vp, C.POINTER(_u32)]),
    "vf_terrain_debug_spill_group": (_i, [_vp, _u32]),
    "vf_terrain_debug_spill_stage": (_i, [_vp, _u32, C.POINTER(_f)]),
    "vf_dem_create": (_i, [_vp, C.POINTER(_vp)]),
    "vf_dem_destroy": (None, [_vp]),
    "vf_dem_set_heights_f32": (_i, [_vp, _vp, _u32, _u32, _f]),
    "vf_dem_set_heights_f64": (_i, [_vp, _vp, _u32, _u32, _f]),
    "vf_dem_stats": (_i, [_vp, _vp]),
    "vf_dem_percentile_range": (_i, [_vp, C.POINTER(_f), C.POINTER(_f)]),
    "vf_dem_normalize": (_i, [_vp, _i, _f, _f, _f]),
    "vf_dem_upload_height": (_i, [_vp]),
    "vf_dem_texture_size": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "vf_dem_read_patch": (_i, [_vp, _u32, _u32, _u32, _u32, _vp]),
}
# every symbol include/vf_hip.h declares (checked by tests/test_cabi_symbols.py): the prototypes above are the one list
SYMBOLS = list(_PROTOS)


def load(path: str = DEFAULT_LIB) -> C.CDLL:
    """dlopen the library and attach prototypes.  Raises OSError when it is missing: there is no fallback."""
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class VfError(RuntimeError):
    pass


def _rgba(c):
    """a colour, four numbers in 0 .. 255 -> the uint8[4] a C call takes (pass it as it is, or C.cast it to a void pointer)"""
    return (C.c_uint8 * 4)(*map(int, c))


def tile_layout(width, height, rank, nranks, skew=3, lib=None):
    """Tiles of `rank` in its storage order as an (n, 2) int array of (tx, ty) -- vf_tile_layout, host arithmetic only."""
    lib = lib or load()
    n = _u32()
    if lib.vf_tile_layout(width, height, rank, nranks, skew, None, 0, C.byref(n)) != VF_OK:
        raise VfError(lib.vf_last_error().decode())
    packed = np.zeros(max(n.value, 1), np.uint32)
    if lib.vf_tile_layout(width, height, rank, nranks, skew, packed.ctypes.data, n.value, C.byref(n)) != VF_OK:
        raise VfError(lib.vf_last_error().decode())
    packed = packed[:n.value]
    return np.stack([packed & 0xFFFF, packed >> 16], axis=1).astype(np.int64)


def balance_stripes(stripe_ms, nranks, lib=None):
    """vf_balance_stripes: per-stripe times -> owner per stripe (uint8), every rank with the same number of stripes."""
    lib = lib or load()
    ms = np.ascontiguousarray(stripe_ms, np.float32)
    owner = np.zeros(len(ms), np.uint8)
    if lib.vf_balance_stripes(ms.ctypes.data, len(ms), nranks, owner.ctypes.data) != VF_OK:
        raise VfError(lib.vf_last_error().decode())
    return owner


def register_stripe_map(stripe_owner, stripe_log2, nranks, lib=None):
    """vf_tile_layout_register_map: owner table -> layout word accepted wherever a layout is (set_tile_shard, tile_layout, stitch_tiles)."""
    lib = lib or load()
    owner = np.ascontiguousarray(stripe_owner, np.uint8)
    word = _u32()
    if lib.vf_tile_layout_register_map(owner.ctypes.data, len(owner), stripe_log2, nranks, C.byref(word)) != VF_OK:
        raise VfError(lib.vf_last_error().decode())
    return word.value


class Terrain:
    """Thin RAII wrapper over vf_ctx + vf_terrain for callers that pass raw device pointers / streams."""

    def __init__(self, width, height, grid, lut_rgba8, lut_is_srgb=True, device=0, lib=None, share_ctx=None, supersample=None):
        """`share_ctx`: another Terrain whose context (vf_ctx: device, stream, the side streams handles borrow) this one uses too -- what the
        drop-in module does for every object of a process (one context per process and device); the other Terrain must outlive this one.
        `supersample`: None -- vf_terrain_create; a factor -- vf_terrain_create_supersampled, handed to the library as it
        is (its refusals raise VfError).  W, H stay the frame's size; SW, SH are the sample size, which visibility and geometry buffers have."""
        self.lib = lib or load()
        self.W, self.H, self.grid = int(width), int(height), int(grid)
        self.ss = 1 if supersample is None else int(supersample)
        self.SW, self.SH = self.ss * self.W, self.ss * self.H
        self.ctx, self.t = _vp(), _vp()
        self._own_ctx = share_ctx is None
        if share_ctx is None:
            self._check(self.lib.vf_ctx_create(int(device), C.byref(self.ctx)))
        else:
            self.ctx = share_ctx.ctx
        lut = np.ascontiguousarray(lut_rgba8, dtype=np.uint8).reshape(1024)
        if supersample is None:
            self._check(self.lib.vf_terrain_create(self.ctx, self.W, self.H, self.grid, lut.ctypes.data, int(bool(lut_is_srgb)),
                                                   C.byref(self.t)))
        else:
            self._check(self.lib.vf_terrain_create_supersampled(self.ctx, self.W, self.H, self.grid, lut.ctypes.data, int(bool(lut_is_srgb)),
                                                                self.ss, C.byref(self.t)))

    def _check(self, rc):
        if rc != VF_OK:
            msg = self.lib.vf_last_error().decode()
            raise VfError("No suitable GPU adapter" if rc == VF_ERR_NO_DEVICE else msg)

    # ---- the call shapes the methods below share.  Every failure goes through _check: VfError with vf_last_error(). ----
    def _grid_field(self, read):
        """A per-vertex field through its vf_terrain_read_* call: (grid, grid) float32 (the library holds at least 2 x 2 vertices)."""
        n = max(self.grid, 2)
        out = np.empty((n, n), np.float32)
        self._check(read(self.t, out.ctypes.data))
        return out

    def _to_device(self, fn, dev, stream):
        """A vf_terrain_*_device call: into the device address `dev`, asynchronous on `stream` (None: the context's)."""
        self._check(fn(self.t, dev, stream))

    def _count(self, fn):
        """One uint32 the handle keeps on the host: a scan counter, a count, a setting."""
        n = _u32()
        self._check(fn(self.t, C.byref(n)))
        return n.value

    def _stage(self, fn, repeats, n=1):
        """A vf_terrain_debug_*_stage call, which times `repeats` launches: its n figures in ms -- a float for n = 1, else a tuple."""
        ms = (_f * n)()
        self._check(fn(self.t, int(repeats), ms))
        return ms[0] if n == 1 else tuple(ms)

    def _vertices(self, count, read):
        """The vertices of a list of `count` seeds or observers, (count, 2) uint32; None: no list, or no uniforms set yet (`read` refuses)."""
        if not count:
            return None
        out = np.empty((count, 2), np.uint32)
        return out if read(self.t, out.ctypes.data) == VF_OK else None

    def close(self):
        if self.t:
            self.lib.vf_terrain_destroy(self.t)
            self.t = _vp()
        if self.ctx:
            if self._own_ctx:
                self.lib.vf_ctx_destroy(self.ctx)
            self.ctx = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def device_info(self):
        """dict of the vf_device_info of this handle's device (name, arch, ordinal, PCI bus / device id, ...)."""
        di = DeviceInfo()
        self._check(self.lib.vf_ctx_device_info(self.ctx, C.byref(di)))
        return {k: (getattr(di, k).decode() if isinstance(getattr(di, k), bytes) else getattr(di, k)) for k, _ in DeviceInfo._fields_}

    def stream_handle(self):
        """hipStream_t of the context's own stream (what stream=None means), e.g. for torch.cuda.ExternalStream."""
        h = _vp()
        self._check(self.lib.vf_ctx_stream(self.ctx, C.byref(h)))
        return h.value

    def set_uniforms(self, u):
        u = np.ascontiguousarray(u, dtype=np.float32).reshape(44)
        self._check(self.lib.vf_terrain_set_uniforms(self.t, u.ctypes.data))

    def set_height(self, h):
        h = np.ascontiguousarray(h, dtype=np.float32)
        self._check(self.lib.vf_terrain_set_height(self.t, h.ctypes.data, h.shape[1], h.shape[0]))

    def set_height_device(self, dptr, tw, th):
        self._check(self.lib.vf_terrain_set_height_device(self.t, _vp(dptr), tw, th))

    def set_shade_mode(self, mode):
        """0 = REFERENCE (terrain.wgsl as coded), 1 = SPEC_T32 (documented-only stage; oracle-validated)."""
        self._check(self.lib.vf_terrain_set_shade_mode(self.t, int(mode)))

    def set_shade_precision(self, precision):
        """0 = EXACT (IEEE binary32 in a fixed order: the oracle bit for bit), 1 = FAST (default; hardware rcp / rsq / sin / cos /
        log / exp, within 1 LSB of EXACT, visibility identical)."""
        self._check(self.lib.vf_terrain_set_shade_precision(self.t, int(precision)))

    def set_raster_groups(self, mode):
        """-1: the handle measures both line loops of the raster stage on its own frames and keeps the faster (default); 0 / 1: fixed."""
        self._check(self.lib.vf_terrain_set_raster_groups(self.t, int(mode)))

    def raster_groups(self):
        """(variant that drew the last frame, [tile-kernel ms without groups, with groups]; 0 = not measured in this view)"""
        use, ms = _i(), (C.c_float * 2)()
        self._check(self.lib.vf_terrain_raster_groups(self.t, C.byref(use), C.cast(ms, _vp)))
        return use.value, [float(ms[0]), float(ms[1])]

    def set_shard(self, rank, nranks, band_h=64):
        self._check(self.lib.vf_terrain_set_shard(self.t, rank, nranks, band_h))

    def set_tile_shard(self, rank, nranks, skew=3):
        """`skew`: the layout word skew | stripe_log2 << 16 (include/vf_hip.h, VF_TILE_LAYOUT)."""
        self._check(self.lib.vf_terrain_set_tile_shard(self.t, rank, nranks, skew))

    def add_points(self, xyz, size_px=5.0, rgba=(255, 255, 255, 255), shape=0, drape=False):
        """Point layer (include/vf_hip.h, overlays): xyz (N, 3); size_px a float or (N,); rgba a 4-tuple or (N, 4) uint8;
        shape 0 circle / 1 square.  Returns the layer id."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        sizes = None if np.isscalar(size_px) else np.ascontiguousarray(size_px, dtype=np.float32).reshape(n)
        cols = np.ascontiguousarray(rgba, dtype=np.uint8)
        per = cols.ndim == 2
        default = _rgba([255] * 4 if per else cols.reshape(4))
        layer = _u32()
        self._check(self.lib.vf_terrain_add_points(self.t, xyz.ctypes.data, n, None if sizes is None else sizes.ctypes.data,
                                                   cols.ctypes.data if per else None, float(size_px) if sizes is None else 0.0,
                                                   C.cast(default, _vp), int(shape), int(bool(drape)), C.byref(layer)))
        return layer.value

    def add_lines(self, coords, offsets, width_px=2.0, rgba=(255, 255, 255, 255), cap=2, drape=False):
        """Polyline layer: coords (M, 3), offsets (P + 1,) uint32 (vulkan_forge.pack_lines); cap 0 butt / 1 square / 2 round."""
        coords = np.ascontiguousarray(coords, dtype=np.float32).reshape(-1, 3)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        col = _rgba(rgba)
        layer = _u32()
        self._check(self.lib.vf_terrain_add_lines(self.t, coords.ctypes.data, offsets.ctypes.data, max(len(offsets) - 1, 0),
                                                  float(width_px), C.cast(col, _vp), int(cap), int(bool(drape)), C.byref(layer)))
        return layer.value

    def add_polygons(self, coords, ring_offsets, feature_offsets, fill_rgba=(255, 255, 255, 255), line_rgba=None, line_width_px=1.0,
                     drape=False):
        """Polygon layer: coords (M, 3), ring_offsets (R + 1,), feature_offsets (F + 1,) uint32 (vulkan_forge.pack_polygons);
        fill_rgba a 4-tuple, an (F, 4) uint8 array or None; line_rgba a 4-tuple or None.  Returns the layer id."""
        coords = np.ascontiguousarray(coords, dtype=np.float32).reshape(-1, 3)
        rings = np.ascontiguousarray(ring_offsets, dtype=np.uint32)
        feats = np.ascontiguousarray(feature_offsets, dtype=np.uint32)
        fills = None if fill_rgba is None else np.ascontiguousarray(fill_rgba, dtype=np.uint8)
        per = fills is not None and fills.ndim == 2
        default = None if fills is None or per else C.cast(_rgba(fills.reshape(4)), _vp)
        line = None if line_rgba is None else C.cast(_rgba(line_rgba), _vp)
        layer = _u32()
        self._check(self.lib.vf_terrain_add_polygons(self.t, coords.ctypes.data, rings.ctypes.data, max(len(rings) - 1, 0), feats.ctypes.data,
                                                     max(len(feats) - 1, 0), fills.ctypes.data if per else None, default, line,
                                                     float(line_width_px), int(bool(drape)), C.byref(layer)))
        return layer.value

    def set_layer_occlusion(self, layer, occlude, depth_bias=1e-2):
        """Hide a point / line layer's pixels behind the terrain; depth_bias >= 0, the default VF_OCCLUSION_DEPTH_BIAS."""
        self._check(self.lib.vf_terrain_set_layer_occlusion(self.t, int(layer), int(bool(occlude)), float(depth_bias)))

    def set_layer_haze(self, layer, on=True):
        """A point / line / contour layer takes the handle's atmospheric haze, or stops taking it."""
        self._check(self.lib.vf_terrain_set_layer_haze(self.t, int(layer), int(bool(on))))

    def layer_haze(self, layer):
        on = C.c_int()
        self._check(self.lib.vf_terrain_layer_haze(self.t, int(layer), C.byref(on)))
        return bool(on.value)

    def add_contours(self, levels, width_px=1.0, rgba=(0, 0, 0, 255), lift=0.0, join=0, occlude=False, depth_bias=1e-2):
        """Contour layer extracted on the device from the rendered surface: levels ascending float32; join 0 round /
        1 none.  Returns (layer id, number of segments)."""
        levels = np.ascontiguousarray(levels, dtype=np.float32).reshape(-1)
        col = _rgba(rgba)
        layer, nseg = _u32(), _u32()
        self._check(self.lib.vf_terrain_add_contours(self.t, levels.ctypes.data, len(levels), float(width_px), C.cast(col, _vp), float(lift),
                                                     int(join), int(bool(occlude)), float(depth_bias), C.byref(layer), C.byref(nseg)))
        return layer.value, nseg.value

    def height_bounds(self):
        """(lo, hi) of the rendered surface height h over the grid's vertices (non-finite heights left out)."""
        lo, hi = _f(), _f()
        self._check(self.lib.vf_terrain_height_bounds(self.t, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def layer_primitive_count(self, layer):
        return self._count(lambda t, n: self.lib.vf_terrain_layer_primitive_count(t, int(layer), n))

    def clear_overlays(self):
        self._check(self.lib.vf_terrain_clear_overlays(self.t))

    def tile_times(self):
        """ms the last frame spent on each local tile (storage order: vf_tile_layout's)."""
        n = _u32()
        self._check(self.lib.vf_terrain_tile_times(self.t, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        self._check(self.lib.vf_terrain_tile_times(self.t, out.ctypes.data, n.value, C.byref(n)))
        return out

    def local_tiles(self):
        return self._count(self.lib.vf_terrain_local_tiles)

    def read_tiles(self):
        """(local_tiles, 64, 64, 4) uint8, the tile-major buffer of a tile-sharded handle."""
        n = self.local_tiles()
        out = np.empty((n, 64, 64, 4), np.uint8)
        if n:
            self._check(self.lib.vf_terrain_read_tiles(self.t, out.ctypes.data, 0, n))
        return out

    def stitch_tiles(self, gathered_dptr, image_dptr, nranks, skew, stride_tiles, stream=None, height=None):
        """`height`: stitch a frame of that many rows instead of the handle's (a band of the frame: dist.BandStitchExchange)."""
        self._check(self.lib.vf_stitch_tiles_device(self.ctx, _vp(gathered_dptr), _vp(image_dptr), self.W, self.H if height is None else int(height),
                                                    nranks, skew, stride_tiles, _vp(stream or 0)))

    # ---- RCCL exchange through the C-ABI (include/vf_hip.h, "multi-GPU exchange over RCCL") ----
    def dist_unique_id(self):
        """128 bytes for vf_dist_comm_init: made on one rank, handed to all of them by the host."""
        buf = (C.c_uint8 * DIST_UNIQUE_ID_BYTES)()
        self._check(self.lib.vf_dist_unique_id(C.cast(buf, _vp)))
        return bytes(buf)

    def dist_comm_init(self, unique_id: bytes, rank: int, nranks: int):
        """ncclCommInitRank on this handle's device; returns the communicator (an integer handle = ncclComm_t)."""
        buf = (C.c_uint8 * DIST_UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        comm = _vp()
        self._check(self.lib.vf_dist_comm_init(self.ctx, C.cast(buf, _vp), int(rank), int(nranks), C.byref(comm)))
        return comm.value

    def dist_comm_destroy(self, comm):
        self.lib.vf_dist_comm_destroy(_vp(comm))

    def dist_gather_tiles(self, comm, root, gathered_dptr, stride_tiles, stream=None):
        self._check(self.lib.vf_dist_gather_tiles(self.t, _vp(comm), int(root), _vp(gathered_dptr or 0), int(stride_tiles), _vp(stream or 0)))

    def dist_gather_bands(self, comm, root, image_dptr, stream=None):
        self._check(self.lib.vf_dist_gather_bands(self.t, _vp(comm), int(root), _vp(image_dptr or 0), _vp(stream or 0)))

    def dist_exchange_bands(self, comm, root, image_dptr, stream=None):
        """Column-stripe tile shards -> the frame on `root`: all-to-all + one band stitched per rank + bands gathered in place."""
        self._check(self.lib.vf_dist_exchange_bands(self.t, _vp(comm), int(root), _vp(image_dptr or 0), _vp(stream or 0)))

    def dist_version(self):
        v = _i()
        self._check(self.lib.vf_dist_version(C.byref(v)))
        return v.value

    def fragment_stage(self, repeats=10):
        """The fragment stage as a launch of its own (diagnostics): dict(resolve_ms, covered_pixels, repeats, equal_to_frame)."""
        ft = FragmentTiming()
        self._check(self.lib.vf_terrain_debug_fragment_stage(self.t, int(repeats), C.byref(ft)))
        return {k: getattr(ft, k) for k, _ in FragmentTiming._fields_}

    def local_rows(self):
        return self._count(self.lib.vf_terrain_local_rows)

    def set_output_device(self, dptr):
        self._check(self.lib.vf_terrain_set_output_device(self.t, _vp(dptr)))

    def render(self, stream=None):
        self._check(self.lib.vf_terrain_render(self.t, _vp(stream or 0)))

    def render_batch(self, uniforms, outputs=None, stream=None):
        """n poses back to back (BASELINE config 5): uniforms (n, 44) float32; outputs: n device pointers (frame k -> outputs[k]) or None."""
        u = np.ascontiguousarray(uniforms, np.float32).reshape(-1, 44)
        ptrs = None
        if outputs is not None:
            assert len(outputs) == len(u)
            ptrs = (_vp * len(u))(*[_vp(int(p)) for p in outputs])
        self._check(self.lib.vf_terrain_render_batch(self.t, u.ctypes.data, len(u), ptrs, _vp(stream or 0)))

    def render_batch_host(self, uniforms):
        """n poses, every frame read back: (n, H, W, 4) uint8 (pageable NumPy memory: the runtime stages the copies)."""
        u = np.ascontiguousarray(uniforms, np.float32).reshape(-1, 44)
        out = np.empty((len(u), self.H, self.W, 4), np.uint8)
        ptrs = (_vp * len(u))(*[_vp(out[k].ctypes.data) for k in range(len(u))])
        self._check(self.lib.vf_terrain_render_batch_host(self.t, u.ctypes.data, len(u), ptrs))
        return out

    def sync(self):
        self._check(self.lib.vf_terrain_sync(self.t))

    def read_rgba(self):
        rows = self.local_rows()
        out = np.empty((rows, self.W, 4), np.uint8)
        self._check(self.lib.vf_terrain_read_rgba(self.t, out.ctypes.data, 0, rows))
        return out

    def read_png_scanlines(self):
        """(H, 4W+1) uint8 copy of the handle's pinned PNG scanlines (filter byte + filtered row) of the last frame."""
        ptr, n = _vp(), C.c_size_t()
        self._check(self.lib.vf_terrain_read_png_scanlines(self.t, C.byref(ptr), C.byref(n)))
        buf = (C.c_uint8 * n.value).from_address(ptr.value)
        return np.frombuffer(buf, np.uint8).reshape(self.H, self.W * 4 + 1).copy()

    def read_visibility(self):
        out = np.empty((self.SH if self.ss > 1 else self.local_rows(), self.SW), np.uint32)      # (a supersampled handle: the samples' ids)
        self._check(self.lib.vf_terrain_read_visibility(self.t, out.ctypes.data))
        return out

    # ---- supersampling (include/vf_hip.h) ----
    def supersampling(self):
        """(factor, sample width, sample height) as the library holds them."""
        f, w, h = _u32(), _u32(), _u32()
        self._check(self.lib.vf_terrain_supersampling(self.t, C.byref(f), C.byref(w), C.byref(h)))
        return f.value, w.value, h.value

    def read_samples(self):
        """The samples of the frame rendered last, before the resolve: (f H, f W, 4) uint8, terrain and passes, no overlays."""
        out = np.empty((self.SH, self.SW, 4), np.uint8)
        self._check(self.lib.vf_terrain_read_samples(self.t, out.ctypes.data))
        return out

    def samples_device(self, dev_dst, stream=None):
        """The same into device memory (a torch tensor's data_ptr(), f H x f W x 4 bytes); the copy is asynchronous on `stream`."""
        self._to_device(self.lib.vf_terrain_samples_device, dev_dst, stream)

    def resolve_stage(self, repeats=50):
        """The resolve kernel as timed launches of its own (diagnostics): average ms of `repeats` launches."""
        return self._stage(self.lib.vf_terrain_debug_resolve_stage, repeats)

    # ---- atmospheric haze (include/vf_hip.h) ----
    def set_haze(self, density, *, rgba=(200, 215, 235, 255), start=0.0, falloff=None, base=0.0, max_opacity=1.0, background=False, enabled=True):
        """Atmospheric haze: blend `rgba` over the terrain by view depth beyond `start`; falloff (world units of y): the
        density falls off exponentially with height above `base`, None: uniform haze; background: pixels without terrain take
        max_opacity.  Every parameter is stored by every call, also one that disables, and steers haze_opacity() too."""
        from ._haze import haze_args
        en, dens, col, st, fo, ba, mo, bg = haze_args(density, rgba, start, falloff, base, max_opacity, background, enabled)
        self._check(self.lib.vf_terrain_set_haze(self.t, en, dens, _rgba(col), st, fo, ba, mo, bg))

    def clear_haze(self):
        """Haze off, its parameters the defaults again, its opacity plane freed."""
        self._check(self.lib.vf_terrain_clear_haze(self.t))

    def haze_info(self):
        """The haze settings as stored and eye_y of the live uniforms (None before uniforms are set): a dict."""
        from ._haze import haze_info
        v = HazeInfo()
        self._check(self.lib.vf_terrain_haze_info(self.t, C.byref(v)))
        return haze_info(v.enabled, v.background, v.density, v.start, v.falloff, v.base, v.max_opacity, tuple(v.rgba), v.has_eye, v.eye_y)

    def haze_opacity(self):
        """The haze opacity of every pixel of the frame rendered last, 0 where the pass leaves the pixel: (H, W) float32 of the raster
        size (the sample size on a supersampled handle)."""
        out = np.empty((self.SH, self.SW), np.float32)
        self._check(self.lib.vf_terrain_read_haze_opacity(self.t, out.ctypes.data))
        return out

    def haze_opacity_device(self, dev, stream=None):
        """The same into device memory (a torch tensor's data_ptr(), H x W floats) on `stream`."""
        self._to_device(self.lib.vf_terrain_haze_opacity_device, dev, stream)

    def haze_stage(self, repeats=20):
        """The haze pass alone as timed launches (diagnostics): average ms of `repeats` launches."""
        return self._stage(self.lib.vf_terrain_debug_haze_stage, repeats)

    def set_flood(self, level, seeds=None, *, enabled=True, shallow_rgba=(96, 176, 224, 128), deep_rgba=(16, 64, 160, 224), depth_full=0.1):
        """Flood analysis: the ground below `level` (units of h before exaggeration, as contour levels) that water reaches
        from its sources, as a water tint of the frame.  seeds: None -- every vertex below the level; "edges" -- the water comes in over the
        border of the grid; (N, 2) points (x, z) of the overlays' world frame.  Every parameter is stored by every call, also one that
        disables, and steers flood_field() too."""
        from ._flood import flood_args
        en, lv, mode, xz, sh, dp, full = flood_args(level, seeds, enabled, shallow_rgba, deep_rgba, depth_full)
        self._check(self.lib.vf_terrain_set_flood(self.t, en, lv, mode, None if xz is None else xz.ctypes.data, 0 if xz is None else xz.shape[0],
                                                  _rgba(sh), _rgba(dp), full))

    def clear_flood(self):
        """The flood is off, its parameters are the defaults again and its buffers are freed."""
        self._check(self.lib.vf_terrain_clear_flood(self.t))

    def flood_field(self):
        """The depth field for the current heights, uniforms, level and sources: (grid, grid) float32, level - h where flooded, else 0."""
        return self._grid_field(self.lib.vf_terrain_read_flood_field)

    def flood_field_device(self, dev_depth, stream=None):
        """The same into device memory (a torch tensor's data_ptr()); the copy is asynchronous on `stream`."""
        self._to_device(self.lib.vf_terrain_flood_field_device, dev_depth, stream)

    def flood_info(self):
        """dict: the settings, vertices ((N, 2) uint32 of a seed list, else None) and, of the last computation, flooded_vertices,
        wettable_vertices, passes; scans and the group size."""
        from ._flood import flood_info
        v = FloodInfo()
        self._check(self.lib.vf_terrain_flood_info(self.t, C.byref(v)))
        return flood_info(v.enabled, v.has_flood, v.mode, v.count, self._vertices(v.count, self.lib.vf_terrain_read_flood_seeds), v.level, v.depth_full,
                          tuple(v.shallow_rgba), tuple(v.deep_rgba), v.flooded_vertices, v.wettable_vertices, v.passes, v.scans, v.group)

    def flood_scans(self):
        """How many times the handle has computed its flood field."""
        return self._count(self.lib.vf_terrain_debug_flood_scans)

    def flood_group(self, group=0):
        """Force the number of propagation passes queued per read-back (diagnostics); 0: the default again."""
        self._check(self.lib.vf_terrain_debug_flood_group(self.t, int(group)))

    def flood_stage(self, repeats=5):
        """(ms of one computation of the field, ms of the tint pass) as timed launches of their own on the frame rendered last
        (diagnostics); it needs the flood enabled."""
        return self._stage(self.lib.vf_terrain_debug_flood_stage, repeats, 2)

    def set_spill(self, seeds="edges", *, enabled=True, shallow_rgba=(96, 176, 224, 128), deep_rgba=(16, 64, 160, 224), depth_full=0.1):
        """Spill analysis: the level the water must reach at the sources before a vertex gets wet, and a tint of the
        closed basins by their depth spill - h.  seeds: "edges" -- the border of the grid (the depression-filled surface); (N, 2) points
        (x, z) of the overlays' world frame.  Every parameter is stored by every call, also one that disables, and steers the field
        calls too."""
        from ._spill import spill_args
        en, mode, xz, sh, dp, full = spill_args(seeds, enabled, shallow_rgba, deep_rgba, depth_full)
        self._check(self.lib.vf_terrain_set_spill(self.t, en, mode, None if xz is None else xz.ctypes.data, 0 if xz is None else xz.shape[0],
                                                  _rgba(sh), _rgba(dp), full))

    def clear_spill(self):
        """The spill is off, its parameters are the defaults again and its buffers are freed."""
        self._check(self.lib.vf_terrain_clear_spill(self.t))

    def spill_field(self):
        """The spill field for the current heights, uniforms and sources: (grid, grid) float32, +inf where no path arrives."""
        return self._grid_field(self.lib.vf_terrain_read_spill_field)

    def spill_field_device(self, dev_spill, stream=None):
        """The same into device memory (a torch tensor's data_ptr()); the copy is asynchronous on `stream`."""
        self._to_device(self.lib.vf_terrain_spill_field_device, dev_spill, stream)

    def sink_depth_field(self):
        """(grid, grid) float32: spill - h where that is finite, 0 elsewhere."""
        return self._grid_field(self.lib.vf_terrain_read_sink_depth)

    def spill_info(self):
        """dict: the settings, vertices ((N, 2) uint32 of a seed list, else None) and, of the last computation, reached_vertices,
        sink_vertices, passes, tile_runs; scans and the group size."""
        from ._spill import spill_info
        v = SpillInfo()
        self._check(self.lib.vf_terrain_spill_info(self.t, C.byref(v)))
        return spill_info(v.enabled, v.has_spill, v.mode, v.count, self._vertices(v.count, self.lib.vf_terrain_read_spill_seeds), v.depth_full,
                          tuple(v.shallow_rgba), tuple(v.deep_rgba), v.reached_vertices, v.sink_vertices, v.passes, v.scans, v.group, v.tile_runs)

    def spill_scans(self):
        """How many times the handle has computed its spill field."""
        return self._count(self.lib.vf_terrain_debug_spill_scans)

    def spill_group(self, group=0, flags=True):
        """Force the number of relaxation passes queued per read-back (diagnostics); 0: the default again.  flags=False: the activity
        flags are ignored, every tile runs in every pass."""
        self._check(self.lib.vf_terrain_debug_spill_group(self.t, int(group) | (0 if flags else 0x80000000)))

    def spill_stage(self, repeats=5):
        """(ms of one computation of the field, ms of the tint pass) as timed launches of their own on the frame rendered last
        (diagnostics); it needs the spill enabled."""
        return self._stage(self.lib.vf_terrain_debug_spill_stage, repeats, 2)

    def read_gbuffer(self, planes=("depth", "position", "normal", "primitive")):
        """Geometry buffers of the frame rendered last: dict plane name -> array."""
        from ._gbuffer import PLANES, plane_args
        names = plane_args(planes)
        out = {k: np.empty((self.SH, self.SW) + PLANES[k][1], PLANES[k][0]) for k in names}
        ptr = [out[k].ctypes.data if k in out else None for k in PLANES]
        self._check(self.lib.vf_terrain_read_gbuffer(self.t, *ptr))
        return out

    def gbuffer_device(self, depth=None, position=None, normal=None, primitive=None, stream=None):
        """The same into device memory: each argument a device address (a torch tensor's data_ptr()) or None; asynchronous on `stream`."""
        self._check(self.lib.vf_terrain_gbuffer_device(self.t, depth, position, normal, primitive, stream))

    def pick(self, pixels):
        """What is under the pixels (N, 2) of (x, y) of the frame rendered last: dict depth (N,), position (N, 3), normal (N, 3), primitive (N,)."""
        from ._gbuffer import pick_result, pixel_args
        px = pixel_args(pixels, self.W, self.H)
        out = np.zeros((len(px), 8), np.uint32)
        self._check(self.lib.vf_terrain_pick(self.t, px.ctypes.data, len(px), out.ctypes.data))
        return pick_result(out)

    def gbuffer_stage(self, planes=("depth",), repeats=50):
        """The geometry-buffer kernel as timed launches of its own (diagnostics): average ms of `repeats` launches."""
        from ._gbuffer import PLANES, plane_args
        mask = sum(1 << list(PLANES).index(k) for k in plane_args(planes))
        return self._stage(lambda t, reps, ms: self.lib.vf_terrain_debug_gbuffer_stage(t, mask, reps, ms), repeats)

    def set_shadows(self, enabled=True, *, strength=0.7, softness=0.02, bias=0.002):
        """Cast sun shadows on the terrain.  The three parameters are stored by every call, also one that disables, and
        steer shadow_field() too: set_shadows(False) without them puts the defaults back."""
        from ._shadows import shadow_args
        self._check(self.lib.vf_terrain_set_shadows(self.t, *shadow_args(enabled, strength, softness, bias)))

    def shadow_field(self):
        """The shadow field for the current heights, uniforms and parameters: (grid, grid) float32, lit in [0, 1]."""
        return self._grid_field(self.lib.vf_terrain_read_shadow_field)

    def shadow_field_device(self, dev_lit, stream=None):
        """The same into device memory (a torch tensor's data_ptr()); the copy is asynchronous on `stream`."""
        self._to_device(self.lib.vf_terrain_shadow_field_device, dev_lit, stream)

    def shadow_stage(self, repeats=20):
        """(scan ms, shade-pass ms) of the frame rendered last, as timed launches of their own (diagnostics)."""
        return self._stage(self.lib.vf_terrain_debug_shadow_stage, repeats, 2)

    def shadow_scans(self):
        """How many times the handle has computed its shadow field."""
        return self._count(self.lib.vf_terrain_debug_shadow_scans)

    def set_ambient_occlusion(self, enabled=True, *, strength=0.6, reach=64.0, directions=16):
        """Ambient occlusion from a sky-view scan of the height field.  `directions`: how many of the default set, or
        a (D, 2) array of (ux, uz).  The parameters are stored by every call, also one that disables, and steer sky_view_field()
        too: set_ambient_occlusion(False) without them puts the defaults back."""
        from ._ambient import ambient_args
        enable, strength, reach, D, dirs = ambient_args(enabled, strength, reach, directions)
        self._check(self.lib.vf_terrain_set_ambient(self.t, enable, strength, reach, D, dirs.ctypes.data))

    def sky_view_field(self):
        """The sky-view field for the current heights, uniforms and parameters: (grid, grid) float32, sky in [0, 1], 1 = open sky."""
        return self._grid_field(self.lib.vf_terrain_read_sky_view_field)

    def sky_view_field_device(self, dev_sky, stream=None):
        """The same into device memory (a torch tensor's data_ptr()); the copy is asynchronous on `stream`."""
        self._to_device(self.lib.vf_terrain_sky_view_field_device, dev_sky, stream)

    def ambient_stage(self, repeats=20):
        """(field ms, shade-pass ms) of the frame rendered last, as timed launches of their own (diagnostics)."""
        return self._stage(self.lib.vf_terrain_debug_ambient_stage, repeats, 2)

    def ambient_scans(self):
        """How many times the handle has computed its sky-view field."""
        return self._count(self.lib.vf_terrain_debug_ambient_scans)

    def set_viewshed(self, observer, *, enabled=True, eye_height=0.05, target_height=0.0, radius=None, visible_rgba=(64, 255, 96, 96),
                     hidden_rgba=(0, 0, 0, 0), softness=0.02, bias=0.002):
        """Viewshed analysis: what the observer at (x, z) of the overlays' world frame sees, as a tint of the frame.
        Every parameter is stored by every call, also one that disables, and steers viewshed_field() too."""
        from ._viewshed import viewshed_args
        en, x, z, eye, tgt, rad, vis, hid, soft, bias = viewshed_args(observer, enabled, eye_height, target_height, radius, visible_rgba, hidden_rgba,
                                                                      softness, bias)
        self._check(self.lib.vf_terrain_set_viewshed(self.t, en, (_f * 2)(x, z), eye, tgt, rad, _rgba(vis), _rgba(hid), soft, bias))

    def clear_viewshed(self):
        """Forget the observer: the viewshed is off, its parameters are the defaults again and its buffers are freed."""
        self._check(self.lib.vf_terrain_set_viewshed(self.t, 0, None, 0.0, 0.0, 0.0, None, None, 1.0, 0.0))

    def viewshed_field(self):
        """The viewshed field for the current heights, uniforms, observer and parameters: (grid, grid) float32, 1 = seen, 0 = hidden."""
        return self._grid_field(self.lib.vf_terrain_read_viewshed_field)

    def viewshed_field_device(self, dev_seen, stream=None):
        """The same into device memory (a torch tensor's data_ptr()); the copy is asynchronous on `stream`."""
        self._to_device(self.lib.vf_terrain_viewshed_field_device, dev_seen, stream)

    def viewshed_info(self):
        """dict: enabled, vertex (i, j), observer_xyz (world), eye_y, and the parameters."""
        from ._viewshed import viewshed_info
        v = ViewshedInfo()
        self._check(self.lib.vf_terrain_viewshed_info(self.t, C.byref(v)))
        return viewshed_info(v.enabled, v.has_observer, tuple(v.vertex), tuple(v.observer_xyz), v.eye_y, v.eye_height, v.target_height, v.radius,
                             v.softness, v.bias, tuple(v.visible_rgba), tuple(v.hidden_rgba))

    def viewshed_stage(self, repeats=20):
        """(scan ms, tint-pass ms) of the frame rendered last, as timed launches of their own (diagnostics)."""
        return self._stage(self.lib.vf_terrain_debug_viewshed_stage, repeats, 2)

    def viewshed_scans(self):
        """How many times the handle has computed its viewshed field."""
        return self._count(self.lib.vf_terrain_debug_viewshed_scans)

    def set_cumulative_viewshed(self, observers, *, enabled=True, eye_height=0.05, target_height=0.0, radius=None, high_rgba=(64, 255, 96, 160),
                                low_rgba=(0, 0, 0, 0), softness=0.02, bias=0.002):
        """Cumulative viewshed: how many of the observers, (N, 2) points (x, z) of the overlays' world frame, see each
        vertex, as a tint of the frame.  Every parameter is stored by every call, also one that disables, and steers
        cumulative_viewshed_field() too."""
        from ._cumulative_viewshed import cumulative_viewshed_args
        en, obs, eye, tgt, rad, high, low, soft, bias = cumulative_viewshed_args(observers, enabled, eye_height, target_height, radius, high_rgba,
                                                                                 low_rgba, softness, bias)
        self._check(self.lib.vf_terrain_set_cumulative_viewshed(self.t, en, obs.ctypes.data, obs.shape[0], eye, tgt, rad, _rgba(high), _rgba(low),
                                                                soft, bias))

    def clear_cumulative_viewshed(self):
        """Forget the observers: the cumulative viewshed is off, its parameters are the defaults again and its buffers are freed."""
        self._check(self.lib.vf_terrain_set_cumulative_viewshed(self.t, 0, None, 0, 0.0, 0.0, 0.0, None, None, 1.0, 0.0))

    def cumulative_viewshed_field(self):
        """The count field for the current heights, uniforms, observers and parameters: (grid, grid) float32 in [0, N]."""
        return self._grid_field(self.lib.vf_terrain_read_cumulative_viewshed_field)

    def cumulative_viewshed_field_device(self, dev_count, stream=None):
        """The same into device memory (a torch tensor's data_ptr()); the copy is asynchronous on `stream`."""
        self._to_device(self.lib.vf_terrain_cumulative_viewshed_field_device, dev_count, stream)

    def cumulative_viewshed_info(self):
        """dict: enabled, observers (N), batch, vertices ((N, 2) uint32, None before observers and uniforms are set), and the parameters."""
        from ._cumulative_viewshed import cumulative_viewshed_info
        v = CumulativeViewshedInfo()
        self._check(self.lib.vf_terrain_cumulative_viewshed_info(self.t, C.byref(v)))
        vertices = self._vertices(v.count, self.lib.vf_terrain_read_cumulative_viewshed_vertices)
        return cumulative_viewshed_info(v.enabled, v.count, v.batch, vertices, v.eye_height, v.target_height, v.radius, v.softness, v.bias,
                                        tuple(v.high_rgba), tuple(v.low_rgba))

    def cumulative_viewshed_batch(self, batch=0):
        """Force the number of observers a launch takes (diagnostics); 0: from the memory budget again."""
        self._check(self.lib.vf_terrain_debug_cumulative_viewshed_batch(self.t, int(batch)))

    def cumulative_viewshed_scans(self):
        """How many times the handle has computed its cumulative viewshed field."""
        return self._count(self.lib.vf_terrain_debug_cumulative_viewshed_scans)

    def cumulative_viewshed_stage(self, repeats=5):
        """ms of one computation of the field, as timed launches of their own (diagnostics)."""
        return self._stage(self.lib.vf_terrain_debug_cumulative_viewshed_stage, repeats)

    def set_sun_exposure(self, suns, *, weights=None, incidence=False, enabled=True, softness=0.02, bias=0.002, high_rgba=(255, 208, 64, 160),
                         low_rgba=(0, 0, 0, 0)):
        """Sun exposure: the weighted sum of the shadow fields of the suns, (N, 3) direction vectors, as a tint of the
        frame.  The C call takes vectors: the angle form (N, 2) is the extension's, which shares set_sun's own arithmetic.  Every
        parameter is stored by every call, also one that disables, and steers sun_exposure_field() too."""
        from ._sun_exposure import sun_exposure_args
        en, s, w, inc, soft, bias, high, low = sun_exposure_args(suns, weights, incidence, enabled, softness, bias, high_rgba, low_rgba)
        if s.shape[1] != 3:
            raise ValueError("the C ABI takes suns as (N, 3) direction vectors")
        self._check(self.lib.vf_terrain_set_sun_exposure(self.t, en, s.ctypes.data, w.ctypes.data, s.shape[0], inc, soft, bias, _rgba(high), _rgba(low)))

    def clear_sun_exposure(self):
        """Forget the suns: sun exposure is off, its parameters are the defaults again and its buffers are freed."""
        self._check(self.lib.vf_terrain_clear_sun_exposure(self.t))

    def sun_exposure_field(self):
        """The exposure field for the current heights, uniforms, suns and parameters: (grid, grid) float32 in [0, sum of weights]."""
        return self._grid_field(self.lib.vf_terrain_read_sun_exposure_field)

    def sun_exposure_field_device(self, dev_exposure, stream=None):
        """The same into device memory (a torch tensor's data_ptr()); the copy is asynchronous on `stream`."""
        self._to_device(self.lib.vf_terrain_sun_exposure_field_device, dev_exposure, stream)

    def sun_exposure_info(self):
        """dict: enabled, suns (N), counted, weight_total, incidence, batch, softness, bias and the colours."""
        from ._sun_exposure import sun_exposure_info
        v = SunExposureInfo()
        self._check(self.lib.vf_terrain_sun_exposure_info(self.t, C.byref(v)))
        return sun_exposure_info(v.enabled, v.count, v.counted, v.weight_total, v.incidence, v.batch, v.softness, v.bias, tuple(v.high_rgba),
                                 tuple(v.low_rgba))

    def sun_exposure_batch(self, batch=0):
        """Force the number of suns a launch takes (diagnostics); 0: from the memory budget again."""
        self._check(self.lib.vf_terrain_debug_sun_exposure_batch(self.t, int(batch)))

    def sun_exposure_scans(self):
        """How many times the handle has computed its sun exposure field."""
        return self._count(self.lib.vf_terrain_debug_sun_exposure_scans)

    def sun_exposure_stage(self, repeats=5):
        """ms of one computation of the field, as timed launches of their own (diagnostics)."""
        return self._stage(self.lib.vf_terrain_debug_sun_exposure_stage, repeats)

    def set_drape(self, image, *, extent=None, opacity=1.0, filter="linear"):
        """Drape an image on the terrain as its albedo.  image: (ih, iw, 4) or (ih, iw, 3) uint8, sRGB bytes with
        straight alpha, row 0 at the extent's z0 and column 0 at its x0; extent: (x0, z0, x1, z1) in the world plane of the grid
        (vertices at -1.5 ... 1.5), None: the whole grid.  The handle keeps a copy made at the call; a second call replaces it."""
        from ._drape import drape_args
        img, iw, ih, ch, ext, opacity, code = drape_args(image, extent, opacity, filter)
        self._check(self.lib.vf_terrain_set_drape(self.t, img.ctypes.data, iw, ih, ch, ext.ctypes.data_as(C.POINTER(_f)), opacity, code))

    def set_drape_device(self, dev_rgba, width, height, *, extent=None, opacity=1.0, filter="linear", stream=None):
        """The same from device memory (a torch tensor's data_ptr(): width * height * 4 bytes, RGBA); the copy is device to device and
        asynchronous on `stream`, and later frames of the handle are ordered behind it."""
        from ._drape import drape_params, drape_size
        iw, ih = drape_size(width, height)
        ext, opacity, code = drape_params(extent, opacity, filter)
        self._check(self.lib.vf_terrain_set_drape_device(self.t, dev_rgba, iw, ih, ext.ctypes.data_as(C.POINTER(_f)), opacity, code, stream))

    def clear_drape(self):
        """Drop the draped image and free its copy: the handle draws as before."""
        self._check(self.lib.vf_terrain_clear_drape(self.t))

    def drape_info(self):
        """None, or dict(width, height, extent, opacity, filter) of the drape as set."""
        from ._drape import drape_info
        iw, ih, op, code, ext = _u32(), _u32(), _f(), _i(), (_f * 4)()
        self._check(self.lib.vf_terrain_drape_info(self.t, C.byref(iw), C.byref(ih), ext, C.byref(op), C.byref(code)))
        return drape_info(iw.value, ih.value, tuple(ext), op.value, code.value)

    def drape_stage(self, repeats=20):
        """Shade-pass ms of the drape for the frame rendered last, as timed launches of their own (diagnostics)."""
        return self._stage(self.lib.vf_terrain_debug_drape_stage, repeats)

    def set_drape_mipmaps(self, enabled=True, *, bias=0.0):
        """Sample the draped image through a mip pyramid at the level of detail of each pixel's footprint.  bias is
        added to the level, a finite number in [-16, 16].  A setting of the handle, off by default, that survives set_drape and
        clear_drape; the pyramid exists while a drape is held and mipmaps are on."""
        from ._drape import mip_params
        on, bias = mip_params(enabled, bias)
        self._check(self.lib.vf_terrain_set_drape_mips(self.t, on, bias))

    def drape_mip_info(self):
        """None while mipmaps are off, else dict(levels, sizes=[(w, h), ...], bias, bytes, builds); levels 0 without a drape."""
        from ._drape import mip_info
        on, levels, bias, nbytes, builds, iw, ih = _i(), _u32(), _f(), C.c_uint64(), _u32(), _u32(), _u32()
        self._check(self.lib.vf_terrain_drape_mip_info(self.t, C.byref(on), C.byref(levels), C.byref(bias), C.byref(nbytes), C.byref(builds)))
        self._check(self.lib.vf_terrain_drape_info(self.t, C.byref(iw), C.byref(ih), None, None, None))
        return mip_info(on.value != 0, levels.value, bias.value, nbytes.value, builds.value, iw.value, ih.value)

    def drape_mip_builds(self):
        """How often the pyramid has been built over the handle's life; unlike drape_mip_info(), also while mipmaps are off."""
        builds = _u32()
        self._check(self.lib.vf_terrain_drape_mip_info(self.t, None, None, None, None, C.byref(builds)))
        return int(builds.value)

    def read_drape_level(self, level):
        """Level 1 <= level < levels of the pyramid as (h, w, 4) float16: premultiplied linear (r, g, b, a).  Builds it if stale."""
        from ._drape import mip_level
        levels, w, h = _u32(), _u32(), _u32()
        self._check(self.lib.vf_terrain_drape_mip_info(self.t, None, C.byref(levels), None, None, None))
        k = mip_level(level, levels.value)
        self._check(self.lib.vf_terrain_read_drape_level(self.t, k, None, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 4), np.float16)
        self._check(self.lib.vf_terrain_read_drape_level(self.t, k, out.ctypes.data, None, None))
        return out

    def drape_mip_build_stage(self, repeats=20):
        """Build ms of the whole mip pyramid of the drape held, as timed launches of their own (diagnostics)."""
        return self._stage(self.lib.vf_terrain_debug_drape_mip_build, repeats)

    def set_drape_anisotropy(self, max_anisotropy=1):
        """Anisotropic filtering of the mip sampling: up to max_anisotropy (1, 2, 4, 8 or 16) samples along the longer
        axis of a pixel's footprint, at the level of detail of the shorter.  A setting of the handle, 1 by default, that survives
        set_drape, clear_drape and mipmaps off / on; it has no effect while mipmaps are off."""
        from ._drape import aniso_params
        self._check(self.lib.vf_terrain_set_drape_anisotropy(self.t, aniso_params(max_anisotropy)))

    def drape_anisotropy(self):
        """The largest anisotropy as set (1: off)."""
        return self._count(self.lib.vf_terrain_drape_anisotropy)

    def enable_timing(self, on=True, stats=True, sampled=False):
        """stats=False: HIP events only, the kernels run exactly as untimed (no per-item statistics; blocks_* read 0);
        sampled=True (with stats=False): events on every fourth frame only."""
        self._check(self.lib.vf_terrain_enable_timing(self.t, (1 if stats else (3 if sampled else 2)) if on else 0))

    def item_stats(self):
        """(items, 4) u32 per work item of the last frame: code (local tile | strip << 20 | log2 strips << 24), candidate
        blocks, raster ticks, raster+fragment ticks (10 ns)."""
        cap = self.timings()["tiles"] + 2048
        out = np.zeros((cap, 4), np.uint32)
        n = _u32()
        self._check(self.lib.vf_terrain_debug_item_stats(self.t, out.ctypes.data, cap, C.byref(n)))
        return out[:n.value]

    def band_masks(self):
        """Debug / tests (band masks): the set-up pass's output in the plan state the last frame was drawn from, per block
        of the grid (row-major): dict(box (n, 4) int16 {x0, y0, x1, y1}, flags (n,), count (n,), alive_even (n,) u64, alive_odd (n,) u64,
        masks (n, 8, 2) u64 [block, slot, even / odd], xy (n, 81, 2) int32 snapped vertices)."""
        nb = (self.grid - 1 + 7) // 8
        n = nb * nb
        recs, masks, xy = np.zeros((n, 8), np.uint32), np.zeros((n, 8, 2), np.uint64), np.zeros((n, 81, 2), np.int32)
        got = _u32()
        self._check(self.lib.vf_terrain_debug_band_masks(self.t, recs.ctypes.data, masks.ctypes.data, xy.ctypes.data, n, C.byref(got)))
        assert got.value == n
        wide = recs[:, 4:8].copy().view(np.uint64)
        return dict(box=recs[:, 0:2].copy().view(np.int16), flags=recs[:, 2].copy(), count=recs[:, 3].copy(),
                    alive_even=wide[:, 0].copy(), alive_odd=wide[:, 1].copy(), masks=masks, xy=xy)

    def set_plan_feedback(self, tile_ticks, strips_log2=None, piece_ticks=None):
        """Debug / tests: the scheduling feedback the next frame's plan reads.  Per local tile: tile_ticks (n,) u32,
        strips_log2 (n,) 0 .. 4 (None: 0), piece_ticks (n, 64) u32 (None: 0).  Refused on a handle's first two frames."""
        ticks = np.ascontiguousarray(tile_ticks, dtype=np.uint32).reshape(-1)
        n = len(ticks)
        lg = np.zeros(n, np.uint8) if strips_log2 is None else np.ascontiguousarray(strips_log2, dtype=np.uint8).reshape(n)
        pieces = None if piece_ticks is None else np.ascontiguousarray(piece_ticks, dtype=np.uint32).reshape(n, 64)
        self._check(self.lib.vf_terrain_debug_set_plan_feedback(self.t, ticks.ctypes.data, lg.ctypes.data,
                                                                None if pieces is None else pieces.ctypes.data, n))

    def plan_mode(self, geometry=False):
        """VF_PLAN_* bits: how the frame rendered last was planned.  Whether the plan state's geometry was rebuilt or reused changes nothing
        in the plan, so VF_PLAN_GEOMETRY_REUSED is reported only on request (geometry=True: the word as the library gives it)."""
        m = self._count(self.lib.vf_terrain_debug_plan_mode)
        return m if geometry else m & ~(VF_PLAN_GEOMETRY_REUSED | VF_PLAN_TILE_LISTS)

    def tile_lists(self):
        """Debug / tests: the per-tile candidate lists of the plan state the last frame was drawn from, as a dict:
        built, used (bools), tiles_listed, tiles_fallback, entries, capacity, units_asked.  Waits for the builder."""
        w = (_u32 * 8)()
        self._check(self.lib.vf_terrain_debug_tile_lists(self.t, C.addressof(w)))
        names = ("built", "used", "tiles_listed", "tiles_fallback", "entries", "capacity", "units_asked")
        d = dict(zip(names, (int(v) for v in w)))
        d["built"], d["used"] = bool(d["built"]), bool(d["used"])
        return d

    def set_tile_list_capacity(self, units=0xFFFFFFFF):
        """Debug / tests: the capacity (16-byte units) the next list builders get; both plan states build theirs again."""
        self._check(self.lib.vf_terrain_debug_set_tile_list_capacity(self.t, units))

    def geometry_reused(self):
        """Did the frame rendered last reuse its plan state's block boxes and set-up records (VF_PLAN_GEOMETRY_REUSED)?"""
        return bool(self.plan_mode(geometry=True) & VF_PLAN_GEOMETRY_REUSED)

    def tile_stats(self):
        """(ntiles, 3) u32 per local tile: candidate blocks (sum over strips), raster ticks, raster+fragment ticks (max)."""
        it = self.item_stats()
        out = np.zeros((self.timings()["tiles"], 3), np.uint32)
        tile = it[:, 0] & 0xFFFFF
        np.add.at(out[:, 0], tile, it[:, 1])
        np.maximum.at(out[:, 1], tile, it[:, 2])
        np.maximum.at(out[:, 2], tile, it[:, 3])
        return out

    def phase_cycles(self):
        """(40,) u64: [0:8] shader-clock cycles per phase summed over waves, [8:16] event counts, [16:24] parts of the set-up phase, [24:30] wave-level executions of the line loop's parts, [30:34] parts of the vertex phase
        (libraries built with -DVF_PHASE_PROF only)."""
        out = np.zeros(40, np.uint64)
        self._check(self.lib.vf_terrain_debug_phase_cycles(self.t, out.ctypes.data, 40))
        return out

    def frame_times(self):
        """(tile_ms, period_ms) per timed frame, oldest first (at most the last 64); period_ms[0] is 0."""
        tile, period, n = np.zeros(64, np.float32), np.zeros(64, np.float32), _u32(0)
        self._check(self.lib.vf_terrain_frame_times(self.t, tile.ctypes.data, period.ctypes.data, 64, C.byref(n)))
        return tile[:n.value].copy(), period[:n.value].copy()

    def timings(self):
        tm = Timings()
        self._check(self.lib.vf_terrain_timings(self.t, C.byref(tm)))
        return {k: getattr(tm, k) for k, _ in Timings._fields_}


class Dem:
    """Thin RAII wrapper over vf_ctx + vf_dem: the Renderer DEM path (heights resident on the device, statistics, normalisation,
    the R32F texture round trip) for callers that want the entry points themselves, vf_dem_percentile_range among them."""

    def __init__(self, device=0, lib=None):
        self.lib = lib or load()
        self.ctx, self.d = _vp(), _vp()
        self._check(self.lib.vf_ctx_create(int(device), C.byref(self.ctx)))
        self._check(self.lib.vf_dem_create(self.ctx, C.byref(self.d)))

    def _check(self, rc):
        if rc != VF_OK:
            msg = self.lib.vf_last_error().decode()
            raise VfError("No suitable GPU adapter" if rc == VF_ERR_NO_DEVICE else msg)

    def close(self):
        if self.d:
            self.lib.vf_dem_destroy(self.d)
            self.d = _vp()
        if self.ctx:
            self.lib.vf_ctx_destroy(self.ctx)
            self.ctx = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def set_heights(self, heights, exaggeration=1.0):
        """(h, w) float32 or float64, C-contiguous: heights = (f32)src * exaggeration on the device."""
        a = np.asarray(heights)
        if a.ndim != 2 or a.dtype not in (np.float32, np.float64) or not a.flags.c_contiguous:
            raise TypeError("heights must be a C-contiguous 2-D array of float32 or float64")
        fn = self.lib.vf_dem_set_heights_f32 if a.dtype == np.float32 else self.lib.vf_dem_set_heights_f64
        self._check(fn(self.d, a.ctypes.data, a.shape[1], a.shape[0], float(exaggeration)))

    def stats(self):
        """(min, max, mean, std) as float32 scalars."""
        out = np.zeros(4, np.float32)
        self._check(self.lib.vf_dem_stats(self.d, out.ctypes.data))
        return tuple(out)

    def percentile_range(self):
        """(p1, p99) as float32 scalars."""
        p1, p99 = _f(), _f()
        self._check(self.lib.vf_dem_percentile_range(self.d, C.byref(p1), C.byref(p99)))
        return np.float32(p1.value), np.float32(p99.value)

    def normalize(self, mode, lo=0.0, hi=1.0, eps=1e-8):
        """mode "minmax" (to [lo, hi]) or "zscore", in place on the device."""
        self._check(self.lib.vf_dem_normalize(self.d, {"minmax": 0, "zscore": 1}[mode], float(lo), float(hi), float(eps)))

    def upload(self):
        self._check(self.lib.vf_dem_upload_height(self.d))

    def texture_size(self):
        w, h = _u32(), _u32()
        self._check(self.lib.vf_dem_texture_size(self.d, C.byref(w), C.byref(h)))
        return w.value, h.value

    def read_patch(self, x=0, y=0, w=None, h=None):
        """(h, w) float32 of the uploaded texture; the whole texture by default."""
        tw, th = self.texture_size()
        x, y = int(x), int(y)
        w, h = (tw - x if w is None else int(w)), (th - y if h is None else int(h))
        if x < 0 or y < 0 or w <= 0 or h <= 0:
            raise ValueError(f"patch origin must be >= 0 and patch dimensions > 0 (x={x}, y={y}, w={w}, h={h}; texture {tw} x {th})")
        out = np.empty((h, w), np.float32)
        self._check(self.lib.vf_dem_read_patch(self.d, x, y, w, h, out.ctypes.data))
        return out
