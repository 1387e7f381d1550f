"""vf_terrain_sky_view_field_device into a torch tensor on a stream of the caller's equals vf_terrain_read_sky_view_field and the CPU
model (run by tests/test_gpu_ambient.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import ambient_model as abm
    from overlay_scenes import CAMERAS, heights
    from vulkan_forge_amd import cabi
    W, H, G = 96, 64, 203
    h = heights(4, (97, 131))
    t = cabi.Terrain(W, H, G, np.zeros(1024, np.uint8))
    t.set_height(h)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)
    u[38] = 0.6
    t.set_uniforms(u)
    for reach in (16.0, 70.0):
        t.set_ambient_occlusion(False, reach=reach, directions=abm.IRREGULAR)
        sky = torch.full((G, G), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t.sky_view_field_device(sky.data_ptr(), stream.cuda_stream)
            darkest = sky.min()                            # consumed on the device, behind the copy
        stream.synchronize()
        got = sky.cpu().numpy()
        want = abm.field(u, h, G, abm.IRREGULAR, reach)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), reach
        assert np.array_equal(t.sky_view_field().view(np.uint32), want.view(np.uint32)), reach
        assert float(darkest) == float(want.min())
    assert t.lib.vf_terrain_sky_view_field_device(t.t, None, None) == cabi.VF_ERR_INVALID
    t.close()
    print("AMBIENT TORCH OK")


if __name__ == "__main__":
    main()
