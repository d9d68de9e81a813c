"""The isosurface's host surface without a GPU: the library exports vk_set_isosurface / vk_get_isosurface with the header's struct, the
Python binding mirrors it, and what the Python layer checks itself raises before any native call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_isosurface_calls(hip_built):
    from vokselis_amd import _native as N

    hdr = open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("vk_set_isosurface", "vk_get_isosurface"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in N.SYMBOLS and getattr(hip_built, name) is not None
    assert re.search(r"#define VK_ISO_MAX_REFINE 16\b", code) and N.ISO_MAX_REFINE == 16
    assert re.search(r"#define VK_ABI_VERSION 5\b", code) and hip_built.vk_abi_version() == 5  # additive: the ABI number stays
    # the struct: float iso; float rgb[3]; uint32_t refine -- 20 bytes, the binding field for field
    body = re.search(r"typedef struct vk_isosurface \{(.*?)\} vk_isosurface;", code, flags=re.S).group(1)
    assert re.findall(r"(float|uint32_t)\s+(\w+)(\[3\])?;", body) == [("float", "iso", ""), ("float", "rgb", "[3]"), ("uint32_t", "refine", "")]
    assert C.sizeof(N.VkIsosurface) == 20 and [f[0] for f in N.VkIsosurface._fields_] == ["iso", "rgb", "refine"]
    assert (N.VkIsosurface.iso.offset, N.VkIsosurface.rgb.offset, N.VkIsosurface.refine.offset) == (0, 4, 16)
    # the projection enum is what it was: the isosurface is no third projection
    assert re.search(r"enum vk_projection \{ VK_PROJ_COMPOSITE = 0, VK_PROJ_MAX = 1 \};", code)
    # a NULL context is an error code, never a crash
    s, on = N.VkIsosurface(), C.c_int(7)
    assert hip_built.vk_set_isosurface(None, C.byref(s)) == -1 and hip_built.vk_set_isosurface(None, None) == -1
    assert hip_built.vk_get_isosurface(None, C.byref(s), C.byref(on)) == -1 and on.value == 7


def test_python_surface_checks_its_arguments(hip_built):
    """Context.set_isosurface refuses what it can see itself -- a colour that is no triple, a refine that is no integer in [0, 16] --
    before the native call (the values the library refuses, and the round trip, need a context: tests/test_iso_gpu.py)."""
    import vokselis_amd as V

    assert V.ISO_MAX_REFINE == 16 and V.VkIsosurface is not None
    ctx = V.Context.__new__(V.Context)  # no device here: no native context either
    ctx._h = None
    for kw in (dict(colour=(1.0, 1.0)), dict(colour=(1.0, 1.0, 1.0, 1.0)), dict(refine=17), dict(refine=-1), dict(refine=2.5)):
        with pytest.raises(ValueError):
            ctx.set_isosurface(0.5, **kw)
    with pytest.raises(V.VokselisError):  # the call goes through to the library, which refuses a NULL context
        ctx.set_isosurface(0.5)
    with pytest.raises(V.VokselisError):
        ctx.set_isosurface(None)
    assert isinstance(V.Context.isosurface, property)

