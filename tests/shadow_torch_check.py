"""vf_terrain_shadow_field_device into a torch tensor on a stream of the caller's equals vf_terrain_read_shadow_field and the CPU
model (run by tests/test_gpu_shadows.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import shadow_model as shm
    from overlay_scenes import CAMERAS, GRID, heights
    from vulkan_forge_amd import cabi
    W, H = 320, 200
    h = heights(3)
    t = cabi.Terrain(W, H, GRID, np.zeros(1024, np.uint8))
    t.set_height(h)
    params = dict(strength=0.8, softness=0.05, bias=0.01)
    t.set_shadows(False, **params)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    # GRID = 1024: sixteen chunks per line; an x-major, a z-major and an exactly diagonal sun, straight up, below the horizon
    for sun in ((0.9, 0.5, 0.31), (-0.31, 0.4, 0.9), (-0.5, 0.4, 0.5), (0.0, 1.0, 0.0), (0.2, -0.3, 0.7)):
        u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)
        u[32:35] = sun
        t.set_uniforms(u)
        lit = torch.full((GRID, GRID), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t.shadow_field_device(lit.data_ptr(), stream.cuda_stream)
            darkest = lit.min()                            # consumed on the device, behind the copy
        stream.synchronize()
        got = lit.cpu().numpy()
        want = shm.field(u, h, GRID, **params)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), sun
        assert np.array_equal(t.shadow_field().view(np.uint32), want.view(np.uint32)), sun
        assert float(darkest) == float(want.min())
    assert t.lib.vf_terrain_shadow_field_device(t.t, None, None) == cabi.VF_ERR_INVALID
    t.close()
    print("SHADOW TORCH OK")


if __name__ == "__main__":
    main()
