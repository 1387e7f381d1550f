"""vf_terrain_set_drape_device from a torch tensor on a stream of the caller's, with mipmaps on: the pyramid is built behind the copy
and the frame is the CPU model's (run by tests/test_gpu_drape_mips.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import drape_mip_model as dmm
    import vulkan_forge_amd
    from overlay_scenes import CAMERAS, GRID, heights
    from vulkan_forge_amd import cabi
    drm = dmm.drm
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
    t.set_drape_mipmaps(True, bias=0.5)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    builds = 0
    for img, kw in ((dmm.case_image(), dict(extent=dmm.CASE_EXTENT["default"], opacity=0.37, filter="linear")),
                    (drm.opaque_image((301, 77)), dict(extent=None, opacity=1.0, filter="nearest"))):
        host = torch.from_numpy(img).pin_memory()
        with torch.cuda.stream(stream):
            tensor = host.to(dev, non_blocking=True)
            t.set_drape_device(tensor.data_ptr(), img.shape[1], img.shape[0], stream=stream.cuda_stream, **kw)
            tensor.zero_()                                 # behind the copy on the same stream: the handle holds a snapshot
        t.render()                                         # on the context's stream: the build and the pass wait for the copy
        got = t.read_rgba().copy()
        want, again = dmm.frame(plain, vis, u, h, GRID, lut, img, bias=0.5, **kw)
        assert again.any() and np.array_equal(got, want), int((got != want).any(axis=2).sum())
        builds += 1
        assert t.drape_mip_info()["builds"] == builds
        levels = dmm.pyramid(img)
        for k in (1, len(levels) - 1):
            assert np.array_equal(t.read_drape_level(k).view(np.uint16), levels[k].view(np.uint16)), k
        assert t.drape_mip_info()["builds"] == builds
    stream.synchronize()
    # A frame drawn on a stream of the caller's, behind work of the caller's that takes a while: the pyramid is built on that stream
    # with the frame, and a level read right behind the call waits for it (the read copies on the context's stream).
    img = drm.opaque_image((1024, 512), seed=9)
    t.set_drape(img, filter="linear")
    busy = torch.ones(1 << 26, device=dev)
    with torch.cuda.stream(stream):
        for _ in range(40):
            busy.mul_(1.0001)
    t.render(stream=stream.cuda_stream)
    levels = dmm.pyramid(img)
    for k in (1, 4, len(levels) - 1):
        assert np.array_equal(t.read_drape_level(k).view(np.uint16), levels[k].view(np.uint16)), ("behind a frame on a side stream", k)
    assert t.drape_mip_info()["builds"] == builds + 1
    want, again = dmm.frame(plain, vis, u, h, GRID, lut, img, bias=0.5, filter="linear")
    assert again.any() and np.array_equal(t.read_rgba(), want)
    # an image of the same size in its place: the pyramid is built again, into the buffer held
    img2 = drm.opaque_image((1024, 512), seed=10)
    t.set_drape(img2, filter="linear")
    t.render(stream=stream.cuda_stream)
    assert np.array_equal(t.read_drape_level(2).view(np.uint16), dmm.pyramid(img2)[2].view(np.uint16))
    assert t.drape_mip_info()["builds"] == builds + 2
    stream.synchronize()
    t.close()
    print("DRAPE MIP TORCH OK")


if __name__ == "__main__":
    main()
