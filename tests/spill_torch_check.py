"""vf_terrain_spill_field_device into a torch tensor on a stream of the caller's equals vf_terrain_read_spill_field and the CPU model;
and on the device, for the same seeds, spill_field() < L is flood_field() > 0 (run by tests/test_gpu_spill.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import spill_model as spm
    from overlay_scenes import CAMERAS, heights
    from vulkan_forge_amd import cabi
    for grid in (65, 203):                                 # a tile of one column and one row; 4 x 4 tiles, the last eleven vertices wide
        check(torch, oracle, spm, cabi, CAMERAS, heights, grid)
    print("SPILL TORCH OK")


def check(torch, oracle, spm, cabi, CAMERAS, heights, grid):
    W, H = 320, 200
    fdm = spm.fdm
    tex = spm.dry_texture(heights(**spm.FIELD_TEXTURE))
    t = cabi.Terrain(W, H, grid, np.zeros(1024, np.uint8))
    t.set_height(tex)
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)
    t.set_uniforms(u)
    surface = spm.cm.surface(tex, grid)
    level = fdm.field_level(np.where(np.isfinite(surface), surface, 0.0).astype(np.float32))
    one, several = spm.field_seed_lists(surface, grid)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    for seeds in (one, several, "edges"):
        t.set_spill(seeds, enabled=False)
        spill = torch.full((grid, grid), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t.spill_field_device(spill.data_ptr(), stream.cuda_stream)
            lowest = spill.min()                           # consumed on the device, behind the copy
        stream.synchronize()
        got = spill.cpu().numpy()
        F = spm.field(u, tex, grid, seeds)
        assert np.array_equal(got.view(np.uint32), F.spill.view(np.uint32)), seeds
        assert np.array_equal(t.spill_field().view(np.uint32), F.spill.view(np.uint32)), seeds
        assert np.array_equal(t.sink_depth_field().view(np.uint32), F.sink.view(np.uint32)), seeds
        assert float(lowest) == float(F.spill.min()) and F.reached.any() and not F.reached.all()
        info = t.spill_info()
        assert (info["reached_vertices"], info["sink_vertices"]) == (int(F.reached.sum()), int((F.sink > 0).sum()))
        # the flood identity, on the device: the flood at a level from the same seeds is the set below the level
        t.set_flood(level, seeds, enabled=False)
        depth = torch.empty((grid, grid), dtype=torch.float32, device=dev)
        with torch.cuda.stream(stream):
            t.flood_field_device(depth.data_ptr(), stream.cuda_stream)
            same = bool(torch.equal(spill < level, depth > 0))
            flooded = int((depth > 0).sum())
        stream.synchronize()
        assert same and 0 < flooded < grid * grid, (seeds, flooded)
    assert t.lib.vf_terrain_spill_field_device(t.t, None, None) == cabi.VF_ERR_INVALID
    t.close()


if __name__ == "__main__":
    main()
