#!/usr/bin/env python3
"""Cost of the drape's mip pyramid (include/vf_hip.h vf_terrain_set_drape_mips) at C4 (4096 x 4096, grid 4096).

The pyramid build (k_drape_mips, vf_terrain_debug_drape_mip_build) for opaque full-extent images of 4096^2 and 16384^2 texels: ms,
the bytes it moves computed from the shapes (4 per image texel read, 8 per pyramid texel written, 8 per texel of the levels a later
launch reads again) and the share of the HBM peak that makes; and the mipped shade pass (k_relight<., kDrapeMip>), linear and
nearest, beside the unmipped one (k_relight<., kDrape>) of the same session under the default and the fill camera
(vf_terrain_debug_drape_stage times whichever the handle would run).  Kernel times are HIP events around `--launches` back-to-back
launches after a warm-up; the variants alternate within the process, `--reps` rounds, and the median is reported with the spread
(max - min) of the rounds.  Run it twice.

    python tools/exp_drape_mips.py [--size 4096] [--grid 4096] [--images 4096,16384] [--launches 20] [--reps 5] [--out profiles/drape_mips_cost_run1.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exp_drape import CAMERAS, SUN, opaque_image  # noqa: E402

HBM_PEAK_GBS = 8000.0                                     # MI355X: 8 TB/s


def build_bytes(n):
    """bytes the build moves for an n x n image: three levels per launch, each launch reads its source once"""
    from vulkan_forge_amd._drape import mip_sizes
    sz = mip_sizes(n, n)
    read = written = 0
    for k in range(0, len(sz) - 1, 3):
        w, h = sz[k]
        read += w * h * (4 if k == 0 else 8)
        written += sum(8 * a * b for a, b in sz[k + 1:k + 4])
    return read, written


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
    sizes = [int(v) for v in a.images.split(",") if v]
    results = {"frame": [W, H], "grid": G, "launches": a.launches, "reps": a.reps, "hbm_peak_GBs": HBM_PEAK_GBS, "build": {}, "cameras": {}}
    keys = [(mip, filt) for filt in ("linear", "nearest") for mip in (False, True)]
    for n in sizes:
        img = opaque_image(n)
        t.set_drape_mipmaps(True)
        t.set_drape(img)
        build = [t.drape_mip_build_stage(a.launches) for _ in range(a.reps)]
        rd, wr = build_bytes(n)
        ms = float(np.median(build))
        results["build"][str(n)] = {"ms": ms, "spread_ms": float(max(build) - min(build)), "samples_ms": build, "bytes_read": rd, "bytes_written": wr,
                                    "GBs": (rd + wr) / ms * 1e-6, "share_of_hbm_peak": (rd + wr) / ms * 1e-6 / HBM_PEAK_GBS,
                                    "pyramid_bytes": t.drape_mip_info()["bytes"]}
        print(f"image {n}^2: build {ms:.4f} ms (spread {max(build) - min(build):.4f}), {rd + wr} bytes, {(rd + wr) / ms * 1e-6:.0f} GB/s, "
              f"{100 * (rd + wr) / ms * 1e-6 / HBM_PEAK_GBS:.1f} % of the HBM peak", flush=True)
        for cam, eye in CAMERAS.items():
            u = np.array(bench.look_at_uniforms(W, H, eye), np.float32).reshape(44)
            u[32:35] = SUN
            t.set_uniforms(u)
            samples = {k: [] for k in keys}
            for r in range(a.reps):
                for k in (keys if r % 2 == 0 else keys[::-1]):
                    mip, filt = k
                    t.set_drape_mipmaps(mip)
                    t.set_drape(img, filter=filt)
                    t.render()
                    samples[k].append(t.drape_stage(a.launches))
            row = {}
            for (mip, filt), v in samples.items():
                row[("mip_" if mip else "flat_") + filt] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
            for filt in ("linear", "nearest"):
                row["mip_" + filt]["multiple_of_flat"] = row["mip_" + filt]["ms"] / row["flat_" + filt]["ms"]
            for k, v in row.items():
                extra = f", {v['multiple_of_flat']:.2f} x the unmipped pass" if "multiple_of_flat" in v else ""
                print(f"{cam}, image {n}^2: {k:13s} {v['ms']:.4f} ms (spread {v['spread_ms']:.4f}){extra}", flush=True)
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
