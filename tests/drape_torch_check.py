"""vf_terrain_set_drape_device from a torch tensor on a stream of the caller's draws the frame of the CPU model and of
vf_terrain_set_drape (run by tests/test_gpu_drape.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import drape_model as drm
    import vulkan_forge_amd
    from overlay_scenes import CAMERAS, GRID, heights
    from vulkan_forge_amd import cabi
    W, H = 257, 131
    h = heights()
    lut = vulkan_forge_amd.colormap_rgba8("viridis")
    t = cabi.Terrain(W, H, GRID, lut)
    t.set_height(h)
    t.set_shade_precision(0)
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)
    t.set_uniforms(u)
    t.render()
    plain = t.read_rgba().copy()
    vis = t.read_visibility()
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    # the tests' image, then one of another size in its place; the tensor is made on the side stream, right in front of the call
    for img, kw in ((drm.image(), dict(extent=drm.EXTENT, opacity=0.37, filter="linear")),
                    (drm.opaque_image((64, 5)), dict(extent=None, opacity=1.0, filter="nearest"))):
        host = torch.from_numpy(img).pin_memory()
        with torch.cuda.stream(stream):
            tensor = host.to(dev, non_blocking=True)
            t.set_drape_device(tensor.data_ptr(), img.shape[1], img.shape[0], stream=stream.cuda_stream, **kw)
            tensor.zero_()                                 # behind the copy on the same stream: the handle holds a snapshot
        t.render()                                         # on the context's stream: ordered behind the copy by the library
        got = t.read_rgba().copy()
        want, again = drm.frame(plain, vis, u, h, GRID, lut, img, **kw)
        assert again.any() and np.array_equal(got, want), int((got != want).any(axis=2).sum())
        info = t.drape_info()
        assert (info["width"], info["height"], info["filter"]) == (img.shape[1], img.shape[0], kw["filter"])
        t.set_drape(img, **kw)
        t.render()
        assert np.array_equal(t.read_rgba(), want)
    stream.synchronize()
    assert t.lib.vf_terrain_set_drape_device(t.t, None, 4, 4, None, 1.0, 1, None) == cabi.VF_ERR_INVALID
    t.clear_drape()
    t.render()
    assert np.array_equal(t.read_rgba(), plain) and t.drape_info() is None
    t.close()
    print("DRAPE TORCH OK")


if __name__ == "__main__":
    main()
