"""vf_terrain_viewshed_field_device into a torch tensor on a stream of the caller's equals vf_terrain_read_viewshed_field and the CPU
model (run by tests/test_gpu_viewshed.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import viewshed_model as vsm
    from overlay_scenes import CAMERAS, heights
    from vulkan_forge_amd import cabi
    W, H, grid = 320, 200, 257
    h = heights(3)
    t = cabi.Terrain(W, H, grid, np.zeros(1024, np.uint8))
    t.set_height(h)
    params = dict(eye_height=0.4, target_height=0.02, softness=0.05, bias=0.01)
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)
    t.set_uniforms(u)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    # a corner, an edge, an inner vertex, a position outside the grid
    for obs in ((-1.5, 1.5), (0.3, -1.5), (0.41, -0.87), (-4.0, 9.0)):
        t.set_viewshed(obs, enabled=False, **params)
        seen = torch.full((grid, grid), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t.viewshed_field_device(seen.data_ptr(), stream.cuda_stream)
            lowest = seen.min()                            # consumed on the device, behind the copy
        stream.synchronize()
        got = seen.cpu().numpy()
        want, v = vsm.field(u, h, grid, obs, **params)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), obs
        assert np.array_equal(t.viewshed_field().view(np.uint32), want.view(np.uint32)), obs
        assert float(lowest) == float(want.min()) and (want < 1).any()
    assert t.lib.vf_terrain_viewshed_field_device(t.t, None, None) == cabi.VF_ERR_INVALID
    t.close()
    print("VIEWSHED TORCH OK")


if __name__ == "__main__":
    main()
