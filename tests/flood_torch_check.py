"""vf_terrain_flood_field_device into a torch tensor on a stream of the caller's equals vf_terrain_read_flood_field and the CPU model
(run by tests/test_gpu_flood.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import flood_model as fdm
    from overlay_scenes import CAMERAS, heights
    from vulkan_forge_amd import cabi
    for grid in (65, 203):                                 # a tile of one column and one row; 4 x 4 tiles, the last eleven vertices wide
        check(torch, oracle, fdm, cabi, CAMERAS, heights, grid)
    print("FLOOD TORCH OK")


def check(torch, oracle, fdm, cabi, CAMERAS, heights, grid):
    W, H = 320, 200
    tex = heights(**fdm.FIELD_TEXTURE)
    t = cabi.Terrain(W, H, grid, np.zeros(1024, np.uint8))
    t.set_height(tex)
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)
    t.set_uniforms(u)
    surface = fdm.cm.surface(tex, grid)
    level = fdm.field_level(surface)
    one, several = fdm.field_seed_lists(surface, level, grid)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    for seeds in (one, several, "edges", None):
        t.set_flood(level, seeds, enabled=False)
        depth = torch.full((grid, grid), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t.flood_field_device(depth.data_ptr(), stream.cuda_stream)
            deepest = depth.max()                          # consumed on the device, behind the copy
        stream.synchronize()
        got = depth.cpu().numpy()
        F = fdm.field(u, tex, grid, level, seeds)
        assert np.array_equal(got.view(np.uint32), F.depth.view(np.uint32)), seeds
        assert np.array_equal(t.flood_field().view(np.uint32), F.depth.view(np.uint32)), seeds
        assert float(deepest) == float(F.depth.max()) and F.flooded.any() and not F.flooded.all()
        info = t.flood_info()
        assert (info["flooded_vertices"], info["wettable_vertices"]) == (int(F.flooded.sum()), int(F.wet.sum()))
    assert t.lib.vf_terrain_flood_field_device(t.t, None, None) == cabi.VF_ERR_INVALID
    t.close()


if __name__ == "__main__":
    main()
