"""The CPU model of supersampled terrain frames: numpy over the existing models.

    out = ssm.resolve(samples, f)                  # (f H, f W, 4) uint8 -> (H, W, 4) uint8: the contract of the resolve kernel
    out = ssm.chain(rgba, vis, uniforms, height, grid, lut, **features)            # the passes over a terrain frame, in the library's order
    s, vis = ssm.samples(W, H, f, uniforms, height, grid, lut, **features)         # the oracle's frame at (f W, f H), then the chain
    out = ssm.frame(W, H, f, uniforms, height, grid, lut, layers=None, **features) # samples -> resolve -> the overlay models at (W, H)
    p = ssm.representative(plane, f)               # plane[f // 2::f, f // 2::f]: the sample pick() answers for

The resolve, per output pixel and colour channel: the f f sample bytes decoded through the 256-entry sRGB8 -> linear table; added in
binary32, rows outer, columns inner, starting from the first sample; times the binary32 1 / (f f); encoded over the threshold table
(byte = the number of thresholds T[1..255] the value reaches).  Alpha: the integer mean of the f f alpha bytes, half up.  The tables are
the oracle's (oracle.srgb_tables); tests/test_supersample_model.py holds them to the overlay model's decode / encode, which the tint
models use, over all 256 bytes.

features (all optional, each as the public setters take them):
    shade_mode   0 / 1
    shadows      dict(strength, softness, bias)
    ambient      dict(directions (D, 2), reach, strength)
    drape        dict(image, extent, opacity, filter, mips=False, bias=0.0, max_anisotropy=1)
    flood        dict(level, seeds (None, "edges" or world (x, z) pairs), shallow_rgba, deep_rgba, depth_full)
    spill        dict(seeds ("edges" or world (x, z) pairs), shallow_rgba, deep_rgba, depth_full)
    exposure     dict(suns, weights, incidence, softness, bias, high_rgba, low_rgba)
    cumulative   dict(observers, radius, eye_height, target_height, softness, bias, high_rgba, low_rgba)
    viewshed     dict(observer, radius, eye_height, target_height, softness, bias, visible_rgba, hidden_rgba)
    haze         dict(density, rgba, start, falloff, base, max_opacity, background)
and in `drape`, with mips, max_anisotropy=1.
"""
from __future__ import annotations

import numpy as np

import model_support as ms

F32 = np.float32
FACTORS = (1, 2, 3, 4)
_tables = None


def tables():
    """(decode (256,) float32, thresholds (256,) float32): the context's tables"""
    global _tables
    if _tables is None:
        import oracle
        d, t = oracle.srgb_tables()
        _tables = (np.ascontiguousarray(d, F32), np.ascontiguousarray(t, F32))
    return _tables


def encode(c):
    """float32 array -> uint8: the number of k in 1..255 with c >= T[k] (what srgb_encode stores)"""
    c = np.ascontiguousarray(c, F32)
    return np.searchsorted(tables()[1][1:], c, side="right").astype(np.uint8)


def resolve(samples, f, order=None):
    """(f H, f W, 4) uint8 -> (H, W, 4) uint8.  `order`: another sequence of the (sy, sx) pairs than the contract's, for the test that
    pins the order."""
    s = np.ascontiguousarray(samples, np.uint8)
    f = int(f)
    assert f in FACTORS and s.ndim == 3 and s.shape[2] == 4 and s.shape[0] % f == 0 and s.shape[1] % f == 0
    if f == 1:
        return s.copy()
    H, W = s.shape[0] // f, s.shape[1] // f
    b = s.reshape(H, f, W, f, 4)
    lin = tables()[0][b[..., :3]]                              # (H, f, W, f, 3) float32
    pairs = [(sy, sx) for sy in range(f) for sx in range(f)] if order is None else list(order)
    assert sorted(pairs) == [(sy, sx) for sy in range(f) for sx in range(f)]
    acc = lin[:, pairs[0][0], :, pairs[0][1], :].astype(F32)
    for sy, sx in pairs[1:]:
        acc = (acc + lin[:, sy, :, sx, :]).astype(F32)
    inv = F32(1.0) / F32(f * f)
    out = np.empty((H, W, 4), np.uint8)
    out[..., :3] = encode((acc * inv).astype(F32))
    a = b[..., 3].astype(np.uint32).sum(axis=(1, 3))
    out[..., 3] = ((a + (f * f) // 2) // (f * f)).astype(np.uint8)
    return out


def representative(plane, f):
    f = int(f)
    return np.asarray(plane)[f // 2::f, f // 2::f]


def _memo(memo, key, make):
    """make() once per key of `memo` (a dict, or None: no memory)"""
    if memo is None:
        return make()
    if key not in memo:
        memo[key] = make()
    return memo[key]


def _key(v):
    """a hashable form of a feature's parameters (arrays by their bytes)"""
    if isinstance(v, dict):
        return tuple((k, _key(v[k])) for k in sorted(v))
    if isinstance(v, (list, tuple)):
        return tuple(_key(x) for x in v)
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, v.tobytes())
    return v


def _sources(seeds, u, grid):
    """what a flood or spill field sees of its sources: the mode, or the seeds' vertices at the uniforms' spacing"""
    import contour_model as cm
    import flood_model as fdm
    if seeds is None or isinstance(seeds, str):
        return seeds
    return _key(fdm.seed_vertices(seeds, cm.spacing_of(u), max(int(grid), 2)))


def chain(rgba, vis, uniforms, height, grid, lut, shade_mode=0, shadows=None, ambient=None, drape=None, flood=None, spill=None, exposure=None,
          cumulative=None, viewshed=None, haze=None, stages=None, memo=None):
    """THE statement of the library's order of passes over a terrain frame `rgba` (H, W, 4) with visibility `vis`, at whatever size
    they have: the ambient / shadow relight -> the draped image (through its mips, and their anisotropic taps, if asked) -> the
    flood's water -> the spill's sink tint -> the sun-exposure, cumulative and viewshed tints -> the haze.  -> the frame behind the
    last pass.  `stages` (a dict) receives what lies between: lit, sky; shaded, mask; draped, drape_mask, drape_sample (mips on: the
    mip / anisotropy model's sample planes); flood_field and spill_field (the models' Field tuples), flood_frame, spill_frame; per late
    pass `<name>_frame` (the frame behind it) and `<name>_field`; haze_opacity.  `memo` (a dict) keeps the vertex fields, which do
    not depend on the camera or the size, for a caller that runs the chain more than once; the flood and spill fields are kept under
    a key without the exaggeration, which neither depends on (include/vf_hip.h): the heights, the grid, the level and the sources,
    a seed list as its vertices at the uniforms' spacing."""
    import ambient_model as abm
    import cumulative_viewshed_model as cvm
    import drape_aniso_model as dam
    import drape_mip_model as dmm
    import drape_model as drm
    import flood_model as fdm
    import haze_model as hzm
    import shadow_model as shm
    import spill_model as spm
    import sun_exposure_model as sem
    import viewshed_model as vsm
    u = ms.u44(uniforms)
    h = np.ascontiguousarray(height, F32)
    vis = np.ascontiguousarray(vis, np.uint32)
    out = np.ascontiguousarray(rgba, np.uint8).reshape(vis.shape + (4,))
    st = {} if stages is None else stages
    surface = (float(u[36]), float(u[38]), h.shape, h.tobytes(), int(grid))      # what a vertex field sees of the uniforms and the heights
    lit = _memo(memo, ("lit", surface, u[32:35].tobytes(), _key(shadows)), lambda: shm.field(u, h, grid, **shadows)) if shadows is not None else None
    sky, strength = None, 0.0
    st["mask"] = np.zeros(vis.shape, bool)
    if ambient is not None:
        strength = ambient["strength"]
        sky = _memo(memo, ("sky", surface, _key(ambient["directions"]), ambient["reach"]), lambda: abm.field(u, h, grid, ambient["directions"], ambient["reach"]))
        out, st["mask"] = abm.frame(out, vis, u, h, grid, lut, sky, strength, lit=lit, shade_mode=shade_mode)
    elif shadows is not None:
        out, st["mask"] = shm.frame(out, vis, u, h, grid, lut, lit, shade_mode=shade_mode)
    st["lit"], st["sky"], st["shaded"] = lit, sky, out
    st["drape_mask"], st["drape_sample"] = np.zeros(vis.shape, bool), None
    if drape is not None:
        kw = dict(extent=drape.get("extent"), opacity=drape.get("opacity", 1.0), filter=drape.get("filter", "linear"), lit=lit, sky=sky,
                  strength=strength, shade_mode=shade_mode)
        if drape.get("mips") and drape.get("max_anisotropy", 1) > 1:
            out, st["drape_mask"], st["drape_sample"] = dam.frame(out, vis, u, h, grid, lut, drape["image"], bias=drape.get("bias", 0.0),
                                                                  max_anisotropy=drape["max_anisotropy"], want_sample=True, **kw)
        elif drape.get("mips"):
            out, st["drape_mask"], st["drape_sample"] = dmm.frame(out, vis, u, h, grid, lut, drape["image"], bias=drape.get("bias", 0.0), want_sample=True, **kw)
        else:
            out, st["drape_mask"] = drm.frame(out, vis, u, h, grid, lut, drape["image"], **kw)
    st["draped"] = out
    ground = (h.shape, h.tobytes(), int(grid))                 # what a flood or spill field sees of the heights: no exaggeration
    if flood is not None:
        tint = {k: flood[k] for k in ("shallow_rgba", "deep_rgba", "depth_full") if k in flood}
        level = float(F32(flood["level"]))
        F = _memo(memo, ("flood", ground, level, _sources(flood.get("seeds"), u, grid)), lambda: fdm.field(u, h, grid, level, flood.get("seeds")))
        out, _ = fdm.frame(out, vis, u, h, grid, F, **tint)
        st["flood_field"], st["flood_frame"] = F, out
    if spill is not None:
        tint = {k: spill[k] for k in ("shallow_rgba", "deep_rgba", "depth_full") if k in spill}
        S = _memo(memo, ("spill", ground, _sources(spill.get("seeds", "edges"), u, grid)), lambda: spm.field(u, h, grid, spill.get("seeds", "edges")))
        out, _ = spm.frame(out, vis, u, h, grid, S, **tint)
        st["spill_field"], st["spill_frame"] = S, out
    if exposure is not None:
        field = {k: exposure[k] for k in ("incidence", "softness", "bias") if k in exposure}
        tint = {k: exposure[k] for k in ("high_rgba", "low_rgba") if k in exposure}
        e = _memo(memo, ("exposure", surface, _key(exposure["suns"]), _key(exposure.get("weights")), _key(field)),
                  lambda: sem.field(u, h, grid, exposure["suns"], exposure.get("weights"), **field))
        out, _ = sem.frame(out, vis, u, h, grid, e, sem.weight_total(exposure["suns"], exposure.get("weights")), **tint)
        st["exposure_field"], st["exposure_frame"] = e, out
    if cumulative is not None:
        field = {k: cumulative[k] for k in ("radius", "eye_height", "target_height", "softness", "bias") if k in cumulative}
        tint = {k: cumulative[k] for k in ("high_rgba", "low_rgba") if k in cumulative}
        cnt = _memo(memo, ("cumulative", surface, _key(cumulative["observers"]), _key(field)), lambda: cvm.field(u, h, grid, cumulative["observers"], **field)[0])
        out, _ = cvm.frame(out, vis, u, h, grid, cnt, len(cumulative["observers"]), **tint)
        st["cumulative_field"], st["cumulative_frame"] = cnt, out
    if viewshed is not None:
        field = {k: viewshed[k] for k in ("eye_height", "target_height", "softness", "bias") if k in viewshed}
        tint = {k: viewshed[k] for k in ("radius", "visible_rgba", "hidden_rgba") if k in viewshed}
        seen, v = _memo(memo, ("viewshed", surface, _key(viewshed["observer"]), _key(field)), lambda: vsm.field(u, h, grid, viewshed["observer"], **field))
        out, _ = vsm.frame(out, vis, u, h, grid, seen, v, **tint)
        st["viewshed_field"], st["viewshed_vertex"], st["viewshed_frame"] = seen, v, out
    st["haze_opacity"] = np.zeros(vis.shape, F32)
    if haze is not None:
        out, st["haze_opacity"] = hzm.frame(out, vis, u, h, grid, **haze)
        st["haze_frame"] = out
    return np.ascontiguousarray(out, np.uint8)


def samples(W, H, f, uniforms, height, grid, lut, shade_mode=0, nthreads=8, stages=None, memo=None, **features):
    """The terrain and its passes at the sample size (f W, f H): the oracle's frame, then `chain` with the features.
    -> (samples (f H, f W, 4) uint8, vis (f H, f W) uint32)"""
    import oracle
    sw, sh = int(f) * int(W), int(f) * int(H)
    u = ms.u44(uniforms)
    h = np.ascontiguousarray(height, F32)
    rgba, vis = oracle.render_terrain(u, sw, sh, grid, h, lut, want_vis=True, nthreads=min(nthreads, oracle.max_threads()), shade_mode=shade_mode)
    return chain(rgba.reshape(sh, sw, 4), vis, u, h, grid, lut, shade_mode=shade_mode, stages=stages, memo=memo, **features), vis


def composite(frame, uniforms, height, grid, layers):
    """the overlay / polygon / contour models at the output size, over the resolved frame (no layer occludes: the visibility is not read)"""
    if layers is None:
        return frame
    import occlusion_model as ocm
    H, W = frame.shape[:2]
    return ocm.composite(frame, np.zeros((H, W), np.uint32), uniforms, height, grid, layers)


def frame(W, H, f, uniforms, height, grid, lut, layers=None, **features):
    """-> dict(samples, vis, resolved, frame): the samples and their visibility at (f H, f W), the resolved frame and the frame under
    its overlays at (H, W)"""
    s, vis = samples(W, H, f, uniforms, height, grid, lut, **features)
    resolved = resolve(s, f)
    return dict(samples=s, vis=vis, resolved=resolved, frame=composite(resolved, uniforms, height, grid, layers))
