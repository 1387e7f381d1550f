"""vf_terrain_gbuffer_device into torch tensors on a stream of the caller's equals vf_terrain_read_gbuffer (run by
tests/test_gpu_gbuffer.py in a process of its own)."""
import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    from overlay_scenes import CAMERAS, GRID, heights
    from vulkan_forge_amd import cabi
    W, H = 640, 360
    t = cabi.Terrain(W, H, GRID, np.zeros(1024, np.uint8))
    t.set_height(heights(3))
    t.set_uniforms(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["near"]))
    t.render()
    want = t.read_gbuffer()
    assert (want["primitive"] != 0).any() and (want["primitive"] == 0).any()
    dev = torch.device("cuda")
    depth = torch.full((H, W), -1.0, dtype=torch.float32, device=dev)
    position = torch.full((H, W, 3), -1.0, dtype=torch.float32, device=dev)
    normal = torch.full((H, W, 3), -1.0, dtype=torch.float32, device=dev)
    primitive = torch.full((H, W), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        t.gbuffer_device(depth.data_ptr(), position.data_ptr(), normal.data_ptr(), primitive.data_ptr(), stream.cuda_stream)
        nearest = depth.min()                              # consumed on the device, behind the kernel
    stream.synchronize()
    got = {"depth": depth.cpu().numpy(), "position": position.cpu().numpy(), "normal": normal.cpu().numpy(),
           "primitive": primitive.cpu().numpy().view(np.uint32)}
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert float(nearest) == float(want["depth"].min())
    # a subset: the planes not asked for are not touched
    depth.fill_(-2.0)
    normal.fill_(-2.0)
    torch.cuda.synchronize()
    t.gbuffer_device(depth=depth.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(bits(depth.cpu().numpy()), bits(want["depth"])) and bool((normal == -2.0).all())
    assert t.lib.vf_terrain_gbuffer_device(t.t, None, None, None, None, None) == cabi.VF_ERR_INVALID
    # frames after it are what they were before it
    before = t.read_rgba()
    t.render()
    assert np.array_equal(t.read_rgba(), before)
    t.close()
    print("GBUFFER TORCH OK")


if __name__ == "__main__":
    main()
