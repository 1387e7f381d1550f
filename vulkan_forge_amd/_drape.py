"""Argument rules of the draped-image methods (Scene / TerrainSpike .set_drape / .clear_drape / .drape_info).

The extension and cabi.Terrain call these before they hand the values to the C-ABI (include/vf_hip.h, a draped image layer); they
need no device.
"""
from __future__ import annotations

import numpy as np

from ._shadows import _number

SIZE_MAX = 16384                                          # VF_DRAPE_SIZE_MAX
NEAREST, LINEAR = 0, 1                                    # VF_DRAPE_NEAREST, VF_DRAPE_LINEAR
FILTERS = {"nearest": NEAREST, "linear": LINEAR}
FULL_EXTENT = (-1.5, -1.5, 1.5, 1.5)                      # the grid's vertices lie at -1.5 ... 1.5 in x and z
DEFAULTS = {"extent": None, "opacity": 1.0, "filter": "linear"}


def drape_params(extent, opacity, filter):
    """-> ((4,) float32 extent (x0, z0, x1, z1), opacity, filter code) as the C calls take them"""
    if extent is None:
        extent = FULL_EXTENT
    try:
        ext = np.ascontiguousarray(extent, np.float32)
    except (TypeError, ValueError):
        raise TypeError(f"extent must be four numbers (x0, z0, x1, z1), got {type(extent).__name__}") from None
    if ext.shape != (4,):
        raise ValueError(f"extent must be four numbers (x0, z0, x1, z1), got shape {ext.shape}")
    if not np.isfinite(ext).all():
        raise ValueError("extent must be finite")
    if not (ext[2] > ext[0] and ext[3] > ext[1]):
        raise ValueError(f"extent (x0, z0, x1, z1) needs x1 > x0 and z1 > z0, got {tuple(float(v) for v in ext)}")
    opacity = _number("opacity", opacity)
    if not 0.0 <= opacity <= 1.0:
        raise ValueError(f"opacity must lie in [0, 1], got {opacity}")
    if not isinstance(filter, str):
        raise TypeError(f"filter must be 'linear' or 'nearest', got {type(filter).__name__}")
    if filter not in FILTERS:
        raise ValueError(f"filter must be 'linear' or 'nearest', got {filter!r}")
    return ext, opacity, FILTERS[filter]


def drape_args(image, extent=None, opacity=1.0, filter="linear"):
    """-> (contiguous (ih, iw, channels) uint8 array, iw, ih, channels, (4,) float32 extent, opacity, filter code)"""
    if image is None or isinstance(image, (str, bytes)):
        raise TypeError(f"image must be an (ih, iw, 4) or (ih, iw, 3) uint8 array, got {type(image).__name__}")
    try:
        img = np.asarray(image)
    except (TypeError, ValueError):
        raise TypeError(f"image must be an (ih, iw, 4) or (ih, iw, 3) uint8 array, got {type(image).__name__}") from None
    if img.dtype != np.uint8:
        raise TypeError(f"image must be uint8 (sRGB bytes, straight alpha), got {img.dtype}")
    if img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError(f"image must be (ih, iw, 4) or (ih, iw, 3), got shape {img.shape}")
    ih, iw, ch = img.shape
    if not (1 <= iw <= SIZE_MAX and 1 <= ih <= SIZE_MAX):
        raise ValueError(f"image width and height must lie in [1, {SIZE_MAX}], got {iw} x {ih}")
    ext, opacity, code = drape_params(extent, opacity, filter)
    return np.ascontiguousarray(img), int(iw), int(ih), int(ch), ext, opacity, code


def drape_size(iw, ih):
    """the size rule alone (set_drape_device: the image is in device memory)"""
    for name, v in (("width", iw), ("height", ih)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"image {name} must be an int, got {type(v).__name__}")
    if not (1 <= iw <= SIZE_MAX and 1 <= ih <= SIZE_MAX):
        raise ValueError(f"image width and height must lie in [1, {SIZE_MAX}], got {iw} x {ih}")
    return int(iw), int(ih)


def drape_info(iw, ih, extent, opacity, code):
    """what drape_info() returns: None without a drape"""
    if not iw:
        return None
    return {"width": int(iw), "height": int(ih), "extent": tuple(float(v) for v in extent), "opacity": float(opacity),
            "filter": "linear" if code == LINEAR else "nearest"}


# ---- the mip pyramid (set_drape_mipmaps / drape_mip_info / read_drape_level) ----

MIP_BIAS_MAX = 16.0                                       # VF_DRAPE_MIP_BIAS_MAX
MIP_LEVELS_MAX = 15                                       # VF_DRAPE_MIP_LEVELS_MAX
MIP_DEFAULTS = {"enabled": True, "bias": 0.0}


def mip_params(enabled=True, bias=0.0):
    """-> (enabled as 0 | 1, bias) as vf_terrain_set_drape_mips takes them"""
    if isinstance(enabled, (str, bytes)) or not isinstance(enabled, (bool, int, np.bool_, np.integer)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    bias = _number("bias", bias)
    if not -MIP_BIAS_MAX <= bias <= MIP_BIAS_MAX:
        raise ValueError(f"bias must lie in [-16, 16], got {bias}")
    return int(bool(enabled)), bias


ANISOTROPY_MAX = 16                                       # VF_DRAPE_ANISOTROPY_MAX
ANISOTROPIES = (1, 2, 4, 8, 16)


def aniso_params(max_anisotropy=1):
    """-> the largest anisotropy as vf_terrain_set_drape_anisotropy takes it (set_drape_anisotropy)"""
    if isinstance(max_anisotropy, (bool, np.bool_)) or not isinstance(max_anisotropy, (int, np.integer)):
        raise TypeError(f"max_anisotropy must be an int, got {type(max_anisotropy).__name__}")
    if max_anisotropy not in ANISOTROPIES:
        raise ValueError(f"max_anisotropy must be 1, 2, 4, 8 or 16, got {max_anisotropy}")
    return int(max_anisotropy)


def mip_sizes(iw, ih):
    """[(w, h)] of levels 0, 1, ...: each max(1, (size + 1) >> 1) of the level above, down to 1 x 1"""
    sizes = [(int(iw), int(ih))]
    while sizes[-1] != (1, 1):
        w, h = sizes[-1]
        sizes.append((max(1, (w + 1) >> 1), max(1, (h + 1) >> 1)))
    return sizes


def mip_level(level, levels):
    """the level rule of read_drape_level: 1 <= level < levels (level 0 is the uploaded bytes)"""
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
        raise TypeError(f"level must be an int, got {type(level).__name__}")
    if not 1 <= level < levels:
        raise ValueError(f"level must lie in [1, {levels}), got {level}" if levels > 1 else f"the pyramid has no level to read (levels = {levels})")
    return int(level)


def mip_info(enabled, levels, bias, nbytes, builds, iw, ih):
    """what drape_mip_info() returns: None while mipmaps are off; levels 0 and no sizes while they are on without a drape"""
    if not enabled:
        return None
    sizes = mip_sizes(iw, ih) if levels else []
    assert len(sizes) == levels
    return {"levels": int(levels), "sizes": sizes, "bias": float(bias), "bytes": int(nbytes), "builds": int(builds)}
