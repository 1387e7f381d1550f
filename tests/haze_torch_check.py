"""vf_terrain_haze_opacity_device into a torch tensor on a stream of the caller's equals vf_terrain_read_haze_opacity and the CPU
model (run by tests/test_gpu_haze.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import haze_model as hzm
    from overlay_scenes import CAMERAS, GRID, heights
    from vulkan_forge_amd import cabi
    W, H = 96, 64
    h = heights()
    lut = np.zeros(1024, np.uint8)
    t = cabi.Terrain(W, H, GRID, lut)
    t.set_height(h)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream()
    for cam in ("default", "near"):
        u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam]), np.float32).reshape(44)
        t.set_uniforms(u)
        t.render()
        rgba, vis = oracle.render_terrain(u, W, H, GRID, h, lut, want_vis=True, nthreads=8)
        for kw in (dict(hzm.SCENE_PARAMS[cam], falloff=0.3, base=hzm.SCENE_BASE), dict(hzm.SCENE_PARAMS[cam], max_opacity=0.8, background=True)):
            t.set_haze(**kw, enabled=False)                # the plane does not need haze enabled for drawing
            plane = torch.full((H, W), -1.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                t.haze_opacity_device(plane.data_ptr(), stream.cuda_stream)
                highest = plane.max()                      # consumed on the device, behind the pass
            stream.synchronize()
            got = plane.cpu().numpy()
            _, want = hzm.frame(rgba, vis, u, h, GRID, **kw)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cam, kw)
            assert np.array_equal(t.haze_opacity().view(np.uint32), want.view(np.uint32)), (cam, kw)
            assert float(highest) == float(want.max()) > 0.0
    assert t.lib.vf_terrain_haze_opacity_device(t.t, None, None) == cabi.VF_ERR_INVALID
    t.close()
    print("HAZE TORCH OK")


if __name__ == "__main__":
    main()
