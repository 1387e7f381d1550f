#!/usr/bin/env python3
"""Cost of anisotropic filtering of the drape's mip sampling (include/vf_hip.h vf_terrain_set_drape_anisotropy) at C4
(4096 x 4096, grid 4096).

The shade pass k_relight<., kDrapeAniso> at the largest anisotropy A = 2, 4, 8, 16 beside k_relight<., kDrapeMip> (A = 1) of the same
session, for opaque full-extent images of 4096^2 and 16384^2 texels, linear and nearest, under the default and the fill camera
(vf_terrain_debug_drape_stage times whichever pass the handle would run).  Kernel times are HIP events around `--launches`
back-to-back launches after a warm-up; the variants alternate within the process, `--reps` rounds, and the median is reported with
the spread (max - min) of the rounds.  Beside each time stands the mean tap count N of the frame's rewritten pixels, from the CPU
model (tests/drape_aniso_model) on a copy of the case reduced to a 512 x 512 frame over every (size / 512)-th height: the ratio of a
footprint's axes does not depend on the frame's size, so the reduced frame estimates the full one's mean.  Run it twice.

    python tools/exp_drape_aniso.py [--size 4096] [--grid 4096] [--images 4096,16384] [--launches 20] [--reps 5] [--out profiles/drape_aniso_cost_run1.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import model_support  # noqa: E402,F401  (the repository root and the model directories on sys.path)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_drape import CAMERAS, SUN, opaque_image  # noqa: E402

AS = (1, 2, 4, 8, 16)
SMALL = 512


def mean_taps(vf, cabi, bench, h, G, W, eye, img, filt):
    """{A: mean N over the rewritten pixels} of the case reduced to a SMALL x SMALL frame, from the CPU model on the handle's own frame"""
    import drape_aniso_model as dam
    step = max(1, W // SMALL)
    hs = np.ascontiguousarray(h[::step, ::step])
    g = max(2, G // step)
    lut = vf.colormap_rgba8("viridis")
    t = cabi.Terrain(SMALL, SMALL, g, lut)
    t.set_height(hs)
    t.set_shade_precision(0)
    u = np.array(bench.look_at_uniforms(SMALL, SMALL, eye), np.float32).reshape(44)
    u[32:35] = SUN
    t.set_uniforms(u)
    t.render()
    rgba, vis = t.read_rgba().copy(), t.read_visibility().copy()
    t.close()
    out = {}
    for A in AS[1:]:
        _, again, s = dam.frame(rgba, vis, u, hs, g, lut, img, filter=filt, max_anisotropy=A, want_sample=True)
        out[A] = float(s[..., 7][again].mean()) if again.any() else 0.0
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--images", default="4096,16384")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    W = H = a.size
    G = a.grid
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(20261017)
    h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    t = cabi.Terrain(W, H, G, vf.colormap_rgba8("viridis"))
    t.set_height(h)
    t.set_drape_mipmaps(True)
    sizes = [int(v) for v in a.images.split(",") if v]
    results = {"frame": [W, H], "grid": G, "launches": a.launches, "reps": a.reps, "mean_taps_frame": [SMALL, SMALL], "cameras": {}}
    for n in sizes:
        img = opaque_image(n)
        small = np.ascontiguousarray(img[::max(1, n // 1024), ::max(1, n // 1024)])    # (N does not depend on the texels: a thinned copy for the model)
        for cam, eye in CAMERAS.items():
            u = np.array(bench.look_at_uniforms(W, H, eye), np.float32).reshape(44)
            u[32:35] = SUN
            t.set_uniforms(u)
            samples = {(filt, A): [] for filt in ("linear", "nearest") for A in AS}
            for r in range(a.reps):
                for filt in (("linear", "nearest") if r % 2 == 0 else ("nearest", "linear")):
                    t.set_drape(img, filter=filt)
                    for A in (AS if r % 2 == 0 else AS[::-1]):
                        t.set_drape_anisotropy(A)
                        t.render()
                        samples[(filt, A)].append(t.drape_stage(a.launches))
            row = {}
            for filt in ("linear", "nearest"):
                taps = mean_taps(vf, cabi, bench, h, G, W, eye, small, filt)
                base = float(np.median(samples[(filt, 1)]))
                for A in AS:
                    v = samples[(filt, A)]
                    e = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
                    if A > 1:
                        e["multiple_of_mip"] = e["ms"] / base
                        e["mean_taps"] = taps[A]
                        e["ms_per_extra_tap"] = (e["ms"] - base) / max(taps[A] - 1.0, 1e-9)
                    row[f"{filt}_A{A}"] = e
                    extra = f", {e['multiple_of_mip']:.2f} x the mipped pass, mean N {e['mean_taps']:.2f}" if A > 1 else " (k_relight<., kDrapeMip>)"
                    print(f"{cam}, image {n}^2: {filt:8s} A = {A:2d} {e['ms']:.4f} ms (spread {e['spread_ms']:.4f}){extra}", flush=True)
            results["cameras"].setdefault(cam, {})[str(n)] = row
        t.clear_drape()
        del img
    t.close()
    line = json.dumps(results, default=float)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
