"""vf_terrain_sun_exposure_field_device into a torch tensor on a stream of the caller's equals vf_terrain_read_sun_exposure_field and the
CPU model (run by tests/test_gpu_sun_exposure.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import sun_exposure_model as sem
    from overlay_scenes import CAMERAS, heights
    from vulkan_forge_amd import cabi
    W, H, grid = 320, 200, 257
    h = heights(4, (97, 131))
    t = cabi.Terrain(W, H, grid, np.zeros(1024, np.uint8))
    t.set_height(h)
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)
    u[38] = 0.6
    t.set_uniforms(u)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    suns, weights = sem.SUNS[2:24], sem.WEIGHTS[2:24]         # the arc: x-major and z-major suns, one of weight 0, one below the horizon
    for incidence, batch in ((False, 0), (True, 3)):
        t.sun_exposure_batch(batch)
        t.set_sun_exposure(suns, weights=weights, incidence=incidence, enabled=False)
        field = torch.full((grid, grid), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            t.sun_exposure_field_device(field.data_ptr(), stream.cuda_stream)
            highest = field.max()                          # consumed on the device, behind the copy
        stream.synchronize()
        got = field.cpu().numpy()
        want = sem.field(u, h, grid, suns, weights, incidence=incidence)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), incidence
        assert np.array_equal(t.sun_exposure_field().view(np.uint32), want.view(np.uint32)), incidence
        assert float(highest) == float(want.max()) and (want == 0).any() and (want > 1).any()
    assert t.lib.vf_terrain_sun_exposure_field_device(t.t, None, None) == cabi.VF_ERR_INVALID
    t.close()
    print("SUN EXPOSURE TORCH OK")


if __name__ == "__main__":
    main()
