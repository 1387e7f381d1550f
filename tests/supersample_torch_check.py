"""A supersampled handle and device memory of the caller's (run by tests/test_gpu_supersample.py in a process of its own):
vf_terrain_set_output_device with a torch tensor of H x W x 4 receives the resolved frame, vf_terrain_samples_device fills a tensor
of f H x f W x 4 with what vf_terrain_read_samples returns, on a stream of the caller's, and vf_terrain_rgba_device names the frame."""
import ctypes

import numpy as np

import support  # noqa: F401  (the repository root and the model directories on sys.path)


def main():
    import torch                                           # before the library: one HIP runtime per process
    import oracle
    import supersample_model as ssm
    import vulkan_forge_amd
    from vulkan_forge_amd import cabi
    W, H, G = 71, 45, 33
    h = (np.random.default_rng(11).random((33, 33), dtype=np.float32) * 0.6 - 0.3).astype(np.float32)
    u = oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, (3.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0)
    dev = torch.device("cuda")
    for f in (2, 3, 4):
        t = cabi.Terrain(W, H, G, vulkan_forge_amd.colormap_rgba8("viridis"), supersample=f)
        t.set_height(h)
        t.set_uniforms(u)
        t.set_shade_precision(0)
        t.render()
        own = t.read_rgba()
        samples = t.read_samples()
        assert np.array_equal(own, ssm.resolve(samples, f))
        # the caller's output buffer: W x H x 4 bytes, one more row behind it that must stay untouched
        out = torch.full((H + 1, W, 4), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t.set_output_device(out.data_ptr())
        ptr = ctypes.c_void_p()
        assert t.lib.vf_terrain_rgba_device(t.t, ctypes.byref(ptr)) == 0 and ptr.value == out.data_ptr()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            t.render(stream.cuda_stream)
            dst = torch.full((f * H + 1, f * W, 4), 9, dtype=torch.uint8, device=dev)
            t.samples_device(dst.data_ptr(), stream.cuda_stream)
            total = dst[:f * H].sum(dtype=torch.int64)     # consumed on the device, behind the copy
        stream.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:H], own) and (got[H] == 7).all()
        assert np.array_equal(t.read_rgba(), own)          # (the host read-back follows the caller's buffer)
        got = dst.cpu().numpy()
        assert np.array_equal(got[:f * H], samples) and (got[f * H] == 9).all()
        assert int(total) == int(samples.astype(np.int64).sum())
        t.set_output_device(0)
        t.render()
        assert np.array_equal(t.read_rgba(), own)
        t.sync()
        t.close()
    print("SUPERSAMPLE TORCH OK")


if __name__ == "__main__":
    main()
