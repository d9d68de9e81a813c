"""Child process of tests/test_u16_gpu.py::test_group_render_under_fake_rccl_on_a_u16_volume.

Runs with VK_RCCL_LIB naming the single-process stand-in for RCCL (tests/fake_rccl.cpp): vk_group_render with n = 2 and 3 contexts, all on
GPU 0, every member holding the same R16_UNORM volume under the same transfer table -- every frame bitwise equal to vk_render's.
Prints one line per case and "u16_shim_group_check: OK"; any mismatch raises."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    shim = os.environ.get("VK_RCCL_LIB", "")
    assert shim and os.path.exists(shim), "VK_RCCL_LIB must name the fake RCCL library"
    import vokselis_amd as V
    from oracle import oracle as O

    import table_cases as TC

    O.build()
    L = V.native.lib()
    check = V.native.check
    W, H, ts, nvox, dt, B = 328, 200, 32, 32, 0.5, 4
    rng = np.random.default_rng(7)
    vol = np.ascontiguousarray(np.minimum(O.volume_standin_u8(nvox).astype(np.int64) * 257 + rng.integers(0, 256, (nvox,) * 3), 65535).astype(np.uint16))
    table = np.ascontiguousarray(TC.random_table(rng, 64), np.float32)
    cams = [V.Camera(1.0, 0.5 + 0.03 * j, 1.0 + 0.21 * j, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix() for j in range(B)]
    want = []
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    ctx.set_transfer_function(table)
    V.VolumeTexture(ctx, vol, fmt=V.FMT_R16_UNORM)
    for cam in cams:
        ctx.set_camera_blob(cam)
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=dt).record(ctx)
        want.append(ctx.read_backbuffer().copy())
    ctx.close()
    want = np.stack(want)
    assert want[..., :3].max() > 0
    for n in (2, 3):
        ords = (C.c_int * n)(*([0] * n))
        g = C.c_void_p()
        assert L.vk_group_create(n, ords, C.byref(g)) == 0, L.vk_last_error(None)
        try:
            for i in range(n):
                c = C.c_void_p(L.vk_group_ctx(g, i))
                check(c, L.vk_backbuffer_resize(c, W, H, V.OUT_RGBA32F))
                check(c, L.vk_set_transfer_function(c, table.ctypes.data_as(C.POINTER(C.c_float)), table.shape[0], 0.0, 1.0))
                check(c, L.vk_volume_upload(c, vol.ctypes.data, None, nvox, nvox, nvox, V.FMT_R16_UNORM, V.LAYOUT_AUTO))
            root = C.c_void_p(L.vk_group_ctx(g, 0))
            out = C.c_void_p()
            check(root, L.vk_device_alloc(root, B * W * H * 16, C.byref(out)))
            rc = L.vk_group_render(g, V.MODE_NAIVE_TRILINEAR, B, b"".join(cams), ts, dt, 0, out)
            assert rc == 0, L.vk_group_last_error(g)
            assert L.vk_group_sync(g) == 0
            got = np.empty((B, H, W, 4), np.float32)
            check(root, L.vk_device_download(root, got.ctypes.data, out, got.nbytes))
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), ("vk_group_render on a u16 volume", n)
            check(root, L.vk_device_free(root, out))
        finally:
            L.vk_group_destroy(g)
        print("vk_group_render n=%d on a u16 volume: %d frames bitwise" % (n, B))
    print("u16_shim_group_check: OK")


if __name__ == "__main__":
    main()
