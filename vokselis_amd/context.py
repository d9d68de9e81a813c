"""Headless host mirror of the reference's `Context` / `Demo` / `run` surface over the C-ABI.

Reference: src/context.rs (Context), src/context/global_ubo.rs (Uniform),
src/context/hdr_backbuffer.rs (HdrBackBuffer), src/context/volume_texture.rs (VolumeTexture),
src/lib.rs:37-49 (`trait Demo`, `run`).  Windowing, input, hot reload and the present pass are out
of scope (no display on a compute node); the call order of the frame loop is kept:
`Context.update()` -> `Demo.update()` -> `Demo.render()` (src/lib.rs:75-79,178-181).
"""
from __future__ import annotations

import ctypes as C
import struct
import time
from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from .camera import Camera


def dispatch_optimal(length: int, subgroup_size: int) -> int:
    """src/utils/mod.rs:15-18"""
    padded = (subgroup_size - length % subgroup_size) % subgroup_size
    return (length + padded) // subgroup_size


@dataclass
class ImageDimentions:
    """src/utils/mod.rs:91-118 (the reference's spelling)."""
    width: int
    height: int
    unpadded_bytes_per_row: int
    padded_bytes_per_row: int

    @classmethod
    def new(cls, width: int, height: int, align: int) -> "ImageDimentions":
        height = max(height - height % 2, 0)
        width = max(width - width % 2, 0)
        unpadded = width * 4
        row_padding = (align - unpadded % align) % align
        return cls(width, height, unpadded, unpadded + row_padding)

    def linear_size(self) -> int:
        return self.padded_bytes_per_row * self.height


@dataclass
class Uniform:
    """48-byte global uniform, src/context/global_ubo.rs:52-81."""
    pos: tuple = (0.0, 0.0, 0.0)
    frame: int = 0
    resolution: tuple = (1920.0, 780.0)
    mouse: tuple = (0.0, 0.0)
    mouse_pressed: int = 0
    time: float = 0.0
    time_delta: float = 1.0 / 60.0
    _padding: float = 0.0

    def to_bytes(self) -> bytes:
        b = struct.pack("<3fI2f2fI3f", *self.pos, self.frame, *self.resolution, *self.mouse, self.mouse_pressed,
                        self.time, self.time_delta, self._padding)
        assert len(b) == 48
        return b


@dataclass
class HdrBackBuffer:
    """src/context/hdr_backbuffer.rs:10-11 -- fixed 1280x720 rgba16float in the reference."""
    DEFAULT_RESOLUTION = (1280, 720)
    width: int = 1280
    height: int = 720
    format: int = N.OUT_RGBA16F


class FrameCounter:
    """src/utils/frame_counter.rs:1-40 (mean frame time)."""

    def __init__(self):
        self.frame_count = 0
        self.accum_time = 0.0
        self._last = time.perf_counter()
        self._delta = 1.0 / 60.0

    def time_delta(self) -> float:
        return self._delta

    def record(self) -> float:
        now = time.perf_counter()
        self._delta = now - self._last
        self._last = now
        self.accum_time += self._delta
        self.frame_count += 1
        return self._delta


@dataclass
class Hit:
    """One pixel's surface point from the geometry pass (Context.pick): the refined crossing `pos` in unit-cube coordinates, its distance
    `t` along the unit ray from the eye, the raw gradient `grad` (the kernel's scale, times the dimensions; not normalised), the filtered
    sample `value` there, and `normal` = -grad / |grad| in float64 (outward for a surface entered from below the threshold), None
    without a gradient (zero or non-finite)."""
    pos: tuple
    t: float
    grad: tuple
    value: float
    normal: tuple | None


class Context:
    """Device + per-frame uniform/camera upload + backbuffer (src/context.rs:38-67,225-249)."""

    def __init__(self, width: int = 1280, height: int = 720, camera: Camera | None = None, device: int = 0,
                 backbuffer: tuple | None = None, out_format: int = N.OUT_RGBA16F, stream=None):
        L = N.lib()
        self._h = C.c_void_p()
        rc = L.vk_ctx_create(device, C.byref(self._h))
        if rc != N.VK_OK:
            msg = L.vk_last_error(None)
            raise N.VokselisError(rc, msg.decode() if msg else "")
        self.stream_handle = None
        if stream is not None:
            N.check(self._h, L.vk_ctx_set_stream(self._h, C.c_void_p(stream)))
            self.stream_handle = stream
        self.width, self.height = width, height
        # Context::new: Camera::new(1., 0.5, 1., (0.,0.,0.), w/h) when none is given (src/context.rs:124-132)
        self.camera = camera if camera is not None else Camera(1.0, 0.5, 1.0, (0.0, 0.0, 0.0), width / height)
        self.camera_epoch = 0  # bumped whenever a camera blob is uploaded (per-camera caches key on it)
        self.camera_blob = None  # the 144 bytes last uploaded
        self.global_uniform = Uniform()
        bw, bh = backbuffer if backbuffer is not None else HdrBackBuffer.DEFAULT_RESOLUTION
        self.render_backbuffer = HdrBackBuffer(bw, bh, out_format)
        N.check(self._h, L.vk_backbuffer_resize(self._h, bw, bh, out_format))
        self._timeline = time.perf_counter()
        self._first_frame = True
        self.in_flight = 1
        # fuse_present: when the window has the backbuffer's size, RaycastPipeline.record presents from the pass's own epilogue
        # (VK_RENDER_PRESENT) and the render() that follows records nothing -- demo.render + context.render (src/lib.rs:178-182) in one launch
        self.fuse_present = False
        self._pass_presented = False

    # -- lifetime
    def close(self):
        if self._h:
            N.lib().vk_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def get_info(self) -> dict:
        """Context::get_info, src/context.rs:183-203."""
        name = C.create_string_buffer(256)
        cus, is950, mem = C.c_int(), C.c_int(), C.c_size_t()
        N.check(self._h, N.lib().vk_device_info(self._h, name, 256, C.byref(cus), C.byref(is950), C.byref(mem)))
        return {"device_name": name.value.decode(), "compute_units": cus.value, "gfx950": bool(is950.value),
                "total_mem_bytes": mem.value, "backend": "HIP"}

    # -- per frame
    def update(self, frame_counter: FrameCounter | None = None):
        """Context::update, src/context.rs:225-236.  The camera is uploaded unconditionally on the
        first frame (the reference's `updated` gate leaves frame 0 with an identity camera, F10)."""
        gu = self.global_uniform
        gu.time = time.perf_counter() - self._timeline
        if frame_counter is not None:
            gu.time_delta = frame_counter.time_delta()
            gu.frame = frame_counter.frame_count
        gu.resolution = (float(self.width), float(self.height))
        N.check(self._h, N.lib().vk_set_uniform(self._h, gu.to_bytes()))
        if self.camera.updated or self._first_frame:
            self.camera_blob = self.camera.get_proj_view_matrix()
            N.check(self._h, N.lib().vk_set_camera(self._h, self.camera_blob))
            self.camera.updated = False
            self._first_frame = False
            self.camera_epoch += 1

    def resize(self, width: int, height: int):
        """Context::resize, src/context.rs:238-249: the *window* size drives the camera aspect; the
        backbuffer keeps its own resolution (F6)."""
        self.width, self.height = width, height
        self.camera.set_aspect(width, height)

    def resize_backbuffer(self, width: int, height: int, out_format: int | None = None):
        fmt = self.render_backbuffer.format if out_format is None else out_format
        N.check(self._h, N.lib().vk_backbuffer_resize(self._h, width, height, fmt))
        self.render_backbuffer = HdrBackBuffer(width, height, fmt)

    def set_stream(self, hip_stream: int | None):
        """Run this context's work on a caller-owned HIP stream (None: the context's own)."""
        N.check(self._h, N.lib().vk_ctx_set_stream(self._h, C.c_void_p(hip_stream)))
        self.stream_handle = hip_stream

    def set_camera_blob(self, blob: bytes):
        if len(blob) != 144:  # the C side reads exactly one CameraUniform (src/camera.rs:5-11)
            raise ValueError("a camera blob is 144 bytes, got %d" % len(blob))
        N.check(self._h, N.lib().vk_set_camera(self._h, bytes(blob)))
        self.camera_blob = bytes(blob)
        self._first_frame = False
        self.camera_epoch += 1

    def sync(self):
        N.check(self._h, N.lib().vk_ctx_sync(self._h))

    def set_transfer_function(self, table, domain=(0.0, 1.0)):
        """Runtime transfer function of MODE_NAIVE_TRILINEAR (vk_set_transfer_function): `table` is an (n, 4) float32 array of RGBA
        entries (not premultiplied, alpha in [0, 1], 2 <= n <= 256) spread evenly over the sample values `domain` = (lo, hi) -- normalised
        values for R8 and R16_UNORM volumes, values for R16F.  It replaces the built-in transfer and palette (raycast_naive.wgsl:104-110) until
        `table` is None, which resets.  Drains the frames in flight and rebuilds the skip maps of the current volume."""
        L = N.lib()
        if table is None:
            N.check(self._h, L.vk_set_transfer_function(self._h, None, 0, 0.0, 1.0))
            return
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.ndim != 2 or t.shape[1] != 4:
            raise ValueError("transfer table: an (n, 4) array of RGBA entries")
        lo, hi = domain
        N.check(self._h, L.vk_set_transfer_function(self._h, t.ctypes.data_as(C.POINTER(C.c_float)), t.shape[0], float(lo), float(hi)))

    def set_projection(self, projection):
        """Projection of MODE_NAIVE_TRILINEAR (vk_set_projection): "max" for a maximum-intensity projection over the window of the
        table in force (without a table: a grey ramp over [0, 1]), None or "composite" for the front-to-back compositing (the default).
        Drains the frames in flight and rebuilds the skip maps of the current volume; lighting is ignored under "max"."""
        if projection in (None, "composite", N.PROJ_COMPOSITE):
            value = N.PROJ_COMPOSITE
        elif projection in ("max", N.PROJ_MAX):
            value = N.PROJ_MAX
        else:
            raise ValueError('set_projection: "max", "composite" or None')
        N.check(self._h, N.lib().vk_set_projection(self._h, value))

    @property
    def projection(self):
        """The projection in force: "max", or None for the compositing default (vk_get_projection)."""
        v = C.c_int(0)
        N.check(self._h, N.lib().vk_get_projection(self._h, C.byref(v)))
        return "max" if v.value == N.PROJ_MAX else None

    def set_isosurface(self, iso, colour=(1.0, 1.0, 1.0), refine=4):
        """First-hit isosurface rendering of MODE_NAIVE_TRILINEAR (vk_set_isosurface): a ray stops at its first sample at or above
        `iso` (in sample values: normalised for R8 and R16_UNORM volumes, values for R16F), the crossing is refined by `refine` bisection steps
        (0 .. 16) and the surface of linear colour `colour` is shaded by set_lighting's light, if one is set.  While set, the transfer
        table and the projection are ignored (they stay stored); None turns it off and brings them back.  Drains the frames in flight
        and rebuilds the skip maps of the current volume."""
        L = N.lib()
        if iso is None:
            N.check(self._h, L.vk_set_isosurface(self._h, None))
            return
        c = tuple(float(v) for v in colour)
        if len(c) != 3:
            raise ValueError("set_isosurface: colour needs three components")
        if int(refine) != refine or not 0 <= int(refine) <= N.ISO_MAX_REFINE:
            raise ValueError("set_isosurface: refine is an integer in [0, %d]" % N.ISO_MAX_REFINE)
        s = N.VkIsosurface()
        s.iso = float(iso)
        s.rgb[0], s.rgb[1], s.rgb[2] = c
        s.refine = int(refine)
        N.check(self._h, L.vk_set_isosurface(self._h, C.byref(s)))

    @property
    def isosurface(self):
        """The isosurface in force as (iso, (r, g, b), refine), or None (vk_get_isosurface)."""
        s, on = N.VkIsosurface(), C.c_int(0)
        N.check(self._h, N.lib().vk_get_isosurface(self._h, C.byref(s), C.byref(on)))
        return (s.iso, (s.rgb[0], s.rgb[1], s.rgb[2]), int(s.refine)) if on.value else None

    def set_lighting(self, direction=None, ambient=0.3, diffuse=0.7, specular=0.2, shininess=32.0):
        """Gradient lighting of the table march (vk_set_lighting): each sample's table colour is shaded by the gradient of the trilinear
        interpolant, two-sided Blinn-Phong, rgb' = c.rgb (ambient + diffuse |N.L|) + specular |N.H|^shininess; alpha is untouched.
        `direction`: (x, y, z) towards the light in world space, "headlight" for a light at the eye, or None to turn lighting off.
        Needs a transfer function (set_transfer_function) for NAIVE_TRILINEAR renders; takes effect from the next recorded render."""
        L = N.lib()
        if direction is None:
            N.check(self._h, L.vk_set_lighting(self._h, None))
            return
        li = N.VkLighting()
        if isinstance(direction, str):
            if direction != "headlight":
                raise ValueError('set_lighting: direction is None, (x, y, z) or "headlight"')
            li.headlight = 1
        else:
            d = tuple(float(v) for v in direction)
            if len(d) != 3:
                raise ValueError("set_lighting: direction needs three components")
            li.dir[0], li.dir[1], li.dir[2] = d
        li.ambient, li.diffuse, li.specular, li.shininess = float(ambient), float(diffuse), float(specular), float(shininess)
        N.check(self._h, L.vk_set_lighting(self._h, C.byref(li)))

    def set_shadows(self, strength=0.7, bias=2.0):
        """Light-direction shadows of the lit isosurface (vk_set_shadows): a ray that hit marches once more from the crossing towards
        the light, and a point whose shadow ray meets the surface again keeps 1 - strength of its diffuse and specular terms.  `bias`:
        the distance of the first shadow sample from the surface, in shadow steps (0 .. 1024; 0 shadows every hit).  set_shadows(None)
        turns them off.  They take effect only under set_isosurface with set_lighting and a light that is not "headlight"; every other
        render ignores them.  Host state like lighting: takes effect from the next recorded render, no drain."""
        L = N.lib()
        if strength is None:
            N.check(self._h, L.vk_set_shadows(self._h, None))
            return
        s = N.VkShadows()
        s.strength, s.bias = float(strength), float(bias)
        N.check(self._h, L.vk_set_shadows(self._h, C.byref(s)))

    @property
    def shadows(self):
        """The shadows in force as (strength, bias), or None (vk_get_shadows)."""
        s, on = N.VkShadows(), C.c_int(0)
        N.check(self._h, N.lib().vk_get_shadows(self._h, C.byref(s), C.byref(on)))
        return (s.strength, s.bias) if on.value else None

    def set_clip_box(self, lo, hi=None):
        """A clip box (cut-away) of the table, lit, MAX and isosurface marches (vk_set_clip_box): NAIVE_TRILINEAR rays march the box
        lo = (x0, y0, z0) .. hi = (x1, y1, z1), in unit-cube coordinates with 0 <= lo < hi <= 1 per axis, instead of the whole cube.
        set_clip_box(None) turns it off.  Host state like lighting: it takes effect from the next recorded render and needs no drain; the
        active tiles and the tile order follow it.  While it is set, NAIVE renders need a transfer function, the "max" projection or an
        isosurface (the built-in march has no clip kernels); the compute and procedural modes ignore it."""
        L = N.lib()
        if lo is None:
            if hi is not None:
                raise ValueError("set_clip_box: (lo, hi) or None")
            N.check(self._h, L.vk_set_clip_box(self._h, None))
            return
        if hi is None:
            raise ValueError("set_clip_box: (lo, hi) or None")
        b = N.clip_box(lo, hi)
        N.check(self._h, L.vk_set_clip_box(self._h, C.byref(b)))

    @property
    def clip_box(self):
        """The clip box in force as ((x0, y0, z0), (x1, y1, z1)), or None (vk_get_clip_box)."""
        b, on = N.VkClipBox(), C.c_int(0)
        N.check(self._h, N.lib().vk_get_clip_box(self._h, C.byref(b), C.byref(on)))
        return (tuple(b.lo), tuple(b.hi)) if on.value else None

    # -- frames in flight: the queue running ahead of the GPU (src/lib.rs:178-194), bounded by the swapchain (src/context.rs:118,252)
    def frames_in_flight(self, k: int):
        """vk_ctx_frames_in_flight: a ring of k frame surfaces, each on its own stream (1: one surface, the default)."""
        N.check(self._h, N.lib().vk_ctx_frames_in_flight(self._h, int(k)))
        self.in_flight = int(k)

    def frame_begin(self) -> int:
        """Surface::get_current_texture (src/context.rs:252): the next surface of the ring (blocks while the frame that used it k
        frames ago is still running); the render / present / read calls that follow address it.  Returns the frame's id."""
        fid = C.c_uint64()
        N.check(self._h, N.lib().vk_frame_begin(self._h, C.byref(fid)))
        return fid.value

    def frame_end(self):
        """queue.submit + frame.present() (src/context.rs:294-296)."""
        N.check(self._h, N.lib().vk_frame_end(self._h))

    def frame_wait(self, frame_id: int):
        N.check(self._h, N.lib().vk_frame_wait(self._h, frame_id))

    def read_frame(self, frame_id: int) -> np.ndarray:
        """vk_frame_readback: that frame's backbuffer (waits for that frame only), while its surface still holds it."""
        bb = self.render_backbuffer
        out = np.empty((bb.height, bb.width, 4), np.float32 if bb.format == N.OUT_RGBA32F else np.float16)
        N.check(self._h, N.lib().vk_frame_readback(self._h, frame_id, out.ctypes.data, out.strides[0]))
        return out

    def capture_frame_of(self, frame_id: int):
        """vk_frame_capture: capture_frame of that frame's presented Rgba8 image."""
        dims = ImageDimentions.new(self.width, self.height, 256)
        buf = np.zeros(dims.linear_size(), np.uint8)
        N.check(self._h, N.lib().vk_frame_capture(self._h, frame_id, buf.ctypes.data, buf.size, None, None, None))
        return buf.tobytes(), dims

    def frame_info(self, frame_id: int) -> dict:
        bb, r8, done = C.c_void_p(), C.c_void_p(), C.c_int()
        N.check(self._h, N.lib().vk_frame_info(self._h, frame_id, C.byref(bb), C.byref(r8), C.byref(done)))
        return {"backbuffer": bb.value, "rgba8": r8.value, "complete": bool(done.value)}

    # -- the geometry pass of the first-hit isosurface (vk_render_geometry: where the surface is)
    def render_geometry(self, dt_scale: float = 1.0, tile=None, flags: int = 0):
        """vk_render_geometry: per pixel of the tile (None: the frame) the refined crossing, its distance along the ray, the gradient and the
        sample there, into the current frame slot's geometry surface; asynchronous.  Needs an isosurface (set_isosurface); lighting,
        shadows, table and projection have no influence.  flags: RENDER_NO_SKIP, RENDER_SAFE, RENDER_FORCE_SKIP, RENDER_PROBE_ALWAYS."""
        bb = self.render_backbuffer
        tx, ty, tw, th = (0, 0, bb.width, bb.height) if tile is None else tile
        N.check(self._h, N.lib().vk_render_geometry(self._h, int(tx), int(ty), int(tw), int(th), float(dt_scale), int(flags)))

    def _split_geometry(self, rec):
        return rec[:, :, 0, :], rec[:, :, 1, :]

    def read_geometry(self):
        """vk_readback_geometry: (pos_t [H, W, 4] f32: the crossing and its distance t, +inf for a miss; grad_x [H, W, 4] f32: the raw
        gradient and the sample value).  np.isfinite(pos_t[..., 3]) is the hit mask.  Blocks."""
        bb = self.render_backbuffer
        rec = np.empty((bb.height, bb.width, 2, 4), np.float32)
        N.check(self._h, N.lib().vk_readback_geometry(self._h, rec.ctypes.data, rec.strides[0]))
        return self._split_geometry(rec)

    def frame_geometry(self, frame_id: int):
        """vk_frame_geometry: read_geometry of that frame's slot (waits for that frame only), while its surface still holds it."""
        bb = self.render_backbuffer
        rec = np.empty((bb.height, bb.width, 2, 4), np.float32)
        N.check(self._h, N.lib().vk_frame_geometry(self._h, frame_id, rec.ctypes.data, rec.strides[0]))
        return self._split_geometry(rec)

    def geometry_info(self) -> dict:
        """vk_geometry_info: the current slot's geometry surface (does not synchronise)."""
        w, h, p = C.c_uint32(), C.c_uint32(), C.c_void_p()
        N.check(self._h, N.lib().vk_geometry_info(self._h, C.byref(w), C.byref(h), C.byref(p)))
        return {"width": w.value, "height": h.value, "device_ptr": p.value}

    def pick(self, x: int, y: int, dt_scale: float = 1.0):
        """vk_pick: what the ray through pixel (x, y) hits -- a Hit, or None for a miss.  Blocks (one wave, one 32-byte download)."""
        if x < 0 or y < 0:
            raise ValueError("pick: negative pixel coordinates")
        h = N.VkHit()
        N.check(self._h, N.lib().vk_pick(self._h, int(x), int(y), float(dt_scale), C.byref(h)))
        if not h.hit:
            return None
        g = np.array(h.grad[:], np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            n = float(np.sqrt((g * g).sum()))
        normal = tuple(float(v) for v in -g / n) if np.isfinite(n) and n > 0.0 else None
        return Hit(tuple(h.pos[:]), float(h.t), tuple(h.grad[:]), float(h.value), normal)

    # -- the slice pass (vk_render_slice: a plane through the volume, thick slabs)
    def render_slice(self, slice, tile=None, values: bool = False):
        """vk_render_slice: the plane `slice` (a VkSlice: Slice.plane / axial / coronal / sagittal) into the tile (None: the frame) of the
        backbuffer -- the volume filtered at each pixel's position, or a slab of samples reduced by max / min / mean, mapped through the
        table in force like the maximum projection and stored as sRGB; asynchronous.  Needs no camera; of the context's state only the
        table and the clip box have influence.  values: also write the (x, weight) records into the slot's value surface."""
        bb = self.render_backbuffer
        tx, ty, tw, th = (0, 0, bb.width, bb.height) if tile is None else tile
        N.check(self._h, N.lib().vk_render_slice(self._h, C.byref(slice) if slice is not None else None, int(tx), int(ty), int(tw), int(th),
                                                 N.SLICE_VALUES if values else 0))

    def read_slice_values(self) -> np.ndarray:
        """vk_readback_slice_values: [H, W, 2] f32 -- per pixel the value x on the kernel's scale (R8: 0..255, R16_UNORM: 0..65535, R16F: the
        value) and the weight, 1 where the pixel's position lies in the box, 0 (with x = +0) elsewhere.  Blocks."""
        bb = self.render_backbuffer
        rec = np.empty((bb.height, bb.width, 2), np.float32)
        N.check(self._h, N.lib().vk_readback_slice_values(self._h, rec.ctypes.data, rec.strides[0]))
        return rec

    def frame_slice_values(self, frame_id: int) -> np.ndarray:
        """vk_frame_slice_values: read_slice_values of that frame's slot (waits for that frame only), while its surface still holds it."""
        bb = self.render_backbuffer
        rec = np.empty((bb.height, bb.width, 2), np.float32)
        N.check(self._h, N.lib().vk_frame_slice_values(self._h, frame_id, rec.ctypes.data, rec.strides[0]))
        return rec

    def slice_values_info(self) -> dict:
        """vk_slice_values_info: the current slot's value surface (does not synchronise)."""
        w, h, p = C.c_uint32(), C.c_uint32(), C.c_void_p()
        N.check(self._h, N.lib().vk_slice_values_info(self._h, C.byref(w), C.byref(h), C.byref(p)))
        return {"width": w.value, "height": h.value, "device_ptr": p.value}

    def slice_probe(self, slice, x: int, y: int) -> N.VkSliceSample:
        """vk_slice_probe: the value under pixel (x, y) of the plane -- a VkSliceSample (inside, pos, value).  Blocks (one wave, 8 bytes down)."""
        if x < 0 or y < 0:
            raise ValueError("slice_probe: negative pixel coordinates")
        out = N.VkSliceSample()
        N.check(self._h, N.lib().vk_slice_probe(self._h, C.byref(slice) if slice is not None else None, int(x), int(y), C.byref(out)))
        return out

    # -- the histogram and region statistics of the volume (vk_volume_histogram)
    def volume_histogram(self, bins: int = 256, domain=(0.0, 1.0), box=None):
        """vk_volume_histogram: the histogram of the stored texels over `domain` (sample values, like set_transfer_function's) in `bins` bins,
        and the statistics of the region, as a Histogram.  box: None -- the whole volume; "clip" -- the voxels whose centres lie in the clip
        box in force; ((x0, y0, z0), (x1, y1, z1)) -- the voxels [x0, x1) x [y0, y1) x [z0, z1).  Blocks; changes no state of the context."""
        from .histogram import Histogram
        from .label import voxel_box

        req = N.VkHistogram(float(domain[0]), float(domain[1]), int(bins), N.HIST_CLIP_BOX if isinstance(box, str) and box == "clip" else 0)
        vb = voxel_box(box)
        counts = np.zeros(max(int(bins), 0), np.uint64)
        stats = N.VkVolumeStats()
        N.check(self._h, N.lib().vk_volume_histogram(self._h, C.byref(req), C.byref(vb) if vb is not None else None,
                                                     counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(stats)))
        return Histogram(counts, (req.lo, req.hi), stats)

    # -- the isosurface as a triangle mesh (vk_extract_isosurface)
    def extract_isosurface(self, iso: float, box=None, max_triangles=None) -> np.ndarray:
        """vk_extract_isosurface: the surface `stored texel >= iso` (sample values, like set_isosurface's; independent of it) by marching
        tetrahedra, as a float32 array (n, 3, 3) of triangles in unit-cube coordinates, normals towards lower values.  box: None -- the whole
        volume; "clip" -- the voxels whose centres lie in the clip box in force; ((x0, y0, z0), (x1, y1, z1)).  max_triangles: at most that
        many, the first ones in order.  A count call, then a fill call; blocks; changes no state of the context.  See V.weld, V.write_stl
        and V.write_obj."""
        from .label import voxel_box

        req = N.VkMeshRequest(float(iso), N.MESH_CLIP_BOX if isinstance(box, str) and box == "clip" else 0)
        vb = voxel_box(box)
        if max_triangles is not None and int(max_triangles) < 0:
            raise ValueError("max_triangles: None or >= 0")
        bp = C.byref(vb) if vb is not None else None
        n = C.c_uint64(0)
        N.check(self._h, N.lib().vk_extract_isosurface(self._h, C.byref(req), bp, None, 0, C.byref(n)))
        m = int(n.value) if max_triangles is None else min(int(n.value), int(max_triangles))
        tris = np.zeros((m, 3, 3), np.float32)
        if m:
            N.check(self._h, N.lib().vk_extract_isosurface(self._h, C.byref(req), bp, tris.ctypes.data_as(C.POINTER(C.c_float)), m, C.byref(n)))
        return tris

    # -- the volume filter pass (vk_volume_filter: separable convolution, 3x3x3 median)
    def filter_volume(self, weights=None, op: str = "convolve", install: bool = True, out: bool = False):
        """vk_volume_filter: the stored volume through a separable convolution -- weights=(wx, wy, wz), each None (the axis is skipped) or
        2 r + 1 weights, r <= FILTER_MAX_RADIUS -- or, op="median3", the 3x3x3 median, into a volume of the same dimensions and format.
        install: the result replaces the context's volume in its layout, under the table / projection / isosurface in force (outside
        frame_begin / frame_end).  out: also return it as a dense array [nz, ny, nx] (uint8; uint16 for R16_UNORM; float16).  Blocks when
        out; needs install or out."""
        from .filter import filter_request

        req = filter_request(weights, op, install)
        dense = self._dense_out() if out else None
        N.check(self._h, N.lib().vk_volume_filter(self._h, C.byref(req), dense.ctypes.data if dense is not None else None))
        return dense

    def smooth_volume(self, sigma, radius=None, install: bool = True, out: bool = False):
        """filter_volume with Gaussian weights (V.gaussian_weights) of `sigma` voxels: one number, or (sx, sy, sz) with None or 0 for an
        axis to skip.  radius: None -- min(6, ceil(3 sigma)) per axis."""
        from .filter import gaussian_weights

        sig = tuple(sigma) if isinstance(sigma, (tuple, list, np.ndarray)) else (sigma, sigma, sigma)
        if len(sig) != 3:
            raise ValueError("sigma: one number or (sx, sy, sz)")
        return self.filter_volume(tuple(None if s is None or float(s) == 0.0 else gaussian_weights(s, radius) for s in sig), "convolve", install, out)

    def median_volume(self, install: bool = True, out: bool = False):
        """filter_volume(op="median3"): every texel becomes the median of its 3x3x3 neighbourhood -- lone speckles vanish, edges stay."""
        return self.filter_volume(None, "median3", install, out)

    # -- the resample pass (vk_volume_resample: crop, resize, convert the format)
    def resample_volume(self, dims=None, scale=None, box=None, mode: str = "linear", fmt=None, window=None, layout=None, install: bool = True, out: bool = False):
        """vk_volume_resample: the voxel box `box` (None: the whole volume; "clip": the clip box's voxels; ((x0, y0, z0), (x1, y1, z1)))
        of the stored volume resampled to dims = (nx, ny, nz) (None or 0 per axis keeps the box's extent) -- or to
        max(1, round(extent * scale)) per axis, scale one number or three -- by mode "nearest", "linear" or "area" (the area-weighted
        mean: the mode for shrinking, at most RESAMPLE_MAX_RATIO per axis).  fmt: None (the volume's format), "u8", "u16" or "f16";
        window = (lo, hi): sample values lo .. hi are mapped onto the whole range of the output format (16-bit data into u8).  install:
        the result replaces the context's volume, in `layout` (None: the current one, PACKED where that cannot hold the new format), under
        the table / projection / isosurface in force (outside frame_begin / frame_end); the clip box stays in force in unit-cube
        coordinates of the new volume.  Returns the VkResampleResult (dims, format, layout, box); with out=True (dense [nz, ny, nx],
        VkResampleResult).  Blocks; needs install or out."""
        from .label import voxel_box
        from .resample import DTYPE, resample_request

        vb = voxel_box(box)
        if scale is not None:
            if dims is not None:
                raise ValueError("resample: dims or scale, not both")
            sc = tuple(scale) if isinstance(scale, (tuple, list, np.ndarray)) else (scale, scale, scale)
            if len(sc) != 3 or not all(np.isfinite(float(s)) and float(s) > 0.0 for s in sc):
                raise ValueError("resample: scale is one finite number > 0, or three")
            dims = tuple(max(1, int(round(n * float(s)))) for n, s in zip(self._box_dims(box), sc))
        req = resample_request(dims, mode, fmt, window, layout, box, install, out)
        res = N.VkResampleResult()
        bp = C.byref(vb) if vb is not None else None
        dense = None
        if out:  # the library says what the call will write (vk_resample_output), or refuses as the call would
            N.check(self._h, N.lib().vk_resample_output(self._h, C.byref(req), bp, C.byref(res)))
            dense = np.zeros((res.dims[2], res.dims[1], res.dims[0]), DTYPE[res.format])
        N.check(self._h, N.lib().vk_volume_resample(self._h, C.byref(req), bp, dense.ctypes.data if dense is not None else None, C.byref(res)))
        return (dense, res) if out else res

    def _box_dims(self, box):
        """The extents (x, y, z) of a pass's voxel box (None: the volume; "clip": the clip box's voxels; two triples), from the library."""
        from .label import voxel_box
        from .resample import resample_request

        vb, res = voxel_box(box), N.VkResampleResult()
        req = resample_request(None, "nearest", box=box, install=False, out=True)
        N.check(self._h, N.lib().vk_resample_output(self._h, C.byref(req), C.byref(vb) if vb is not None else None, C.byref(res)))
        return tuple(int(v) for v in res.dims)

    def crop_volume(self, box, install: bool = True, out: bool = False):
        """resample_volume(mode="nearest") at the box's own extents: the voxels of `box` -- ((x0, y0, z0), (x1, y1, z1)) or "clip" --
        become the volume, bit for bit.  crop_volume("clip") turns the clip box off after a successful install: the crop is what it showed."""
        if box is None:
            raise ValueError('crop: box is "clip" or ((x0, y0, z0), (x1, y1, z1))')
        r = self.resample_volume(None, None, box, "nearest", None, None, None, install, out)
        if box == "clip" and install:
            self.set_clip_box(None)
        return r

    def downsample_volume(self, factor, box=None, install: bool = True, out: bool = False):
        """resample_volume(mode="area") to ceil(n / factor) voxels per axis (factor: one integer or three, at most RESAMPLE_MAX_RATIO):
        every output voxel is the mean of the voxels it covers."""
        from .resample import downsample_dims

        return self.resample_volume(downsample_dims(self._box_dims(box), factor), None, box, "area", None, None, None, install, out)

    def isotropic_volume(self, spacing, mode: str = "linear", install: bool = True, out: bool = False):
        """resample_volume to max(1, round(n_c * spacing_c / min(spacing))) voxels per axis: a scan whose voxels measure
        spacing = (sx, sy, sz) becomes one of cubic voxels of the finest of the three."""
        from .resample import isotropic_dims

        return self.resample_volume(isotropic_dims(self._box_dims(None), spacing), None, None, mode, None, None, None, install, out)

    # -- connected components of a value range (vk_label_components)
    def _volume_dtype(self):
        dims, fmt = (C.c_uint32 * 3)(), C.c_int()
        N.check(self._h, N.lib().vk_volume_info(self._h, dims, C.byref(fmt), None, None))
        return tuple(dims), {N.FMT_R8_UNORM: np.uint8, N.FMT_R16_UNORM: np.uint16, N.FMT_R16_FLOAT: np.float16}.get(fmt.value)

    def _dense_out(self):
        """A dense array [nz, ny, nx] of the volume's dtype for a pass to write; RGBA16F_PAIR: a stand-in, the library refuses before it writes."""
        dims, dtype = self._volume_dtype()
        return np.zeros((dims[2], dims[1], dims[0]) if dtype is not None else (1, 1, 1), dtype or np.uint8)

    def label_components(self, lo, hi=float("inf"), connectivity: int = 6, box=None, labels: bool = False):
        """vk_label_components: the connected components of the voxels whose stored texel lies in [lo, hi] (sample values, like
        set_isosurface's), as a Components -- .n, .sizes, .first, .boxes in id order (ids 1 .. n by first voxel in raster order),
        .n_foreground, and with labels=True .labels, uint32 [nz, ny, nx] (0: background).  connectivity: 6, 18 or 26.  box: None,
        "clip" or ((x0, y0, z0), (x1, y1, z1)).  One call with room for 4096 components, a second only when there are more; blocks; changes
        no state of the context."""
        from .label import Components, label_request, voxel_box

        req, vb = label_request(lo, hi, connectivity=connectivity, box=box), voxel_box(box)
        bp = C.byref(vb) if vb is not None else None
        res = N.VkLabelResult()
        lab = None
        if labels:
            dims, _ = self._volume_dtype()
            lab = np.zeros((dims[2], dims[1], dims[0]), np.uint32)
        room = 4096
        table = (N.VkComponent * room)()
        N.check(self._h, N.lib().vk_label_components(self._h, C.byref(req), bp, lab.ctypes.data if lab is not None else None, table, room, None, C.byref(res)))
        n = int(res.n_components)
        if n > room:  # more components than the table had room for: once more, for the table alone
            table = (N.VkComponent * n)()
            N.check(self._h, N.lib().vk_label_components(self._h, C.byref(req), bp, None, table, n, None, C.byref(res)))
        return Components(table, n, int(res.n_foreground), lab)

    def keep_components(self, lo, hi=float("inf"), keep: str = "largest", count: int = 1, seeds=(), invert: bool = False, fill: float = 0.0, connectivity: int = 6,
                        box=None, install: bool = True, out: bool = False):
        """vk_label_components with a selection: the components of [lo, hi] that are kept -- keep="largest" (the `count` largest),
        "min_size" (those of at least `count` voxels), "seeds" (those that hold one of the voxels `seeds`, (x, y, z) each: see
        V.voxel_of) or "all" -- keep their stored texels, every other voxel becomes `fill`; invert=True: the kept components become `fill`
        and everything else stays.  install: the result replaces the context's volume (outside frame_begin / frame_end).  out: also
        return it as a dense array [nz, ny, nx].  Returns (dense or None, VkLabelResult); needs install or out."""
        from .label import label_request, voxel_box

        req, vb = label_request(lo, hi, connectivity=connectivity, box=box, keep=keep, count=count, seeds=seeds, invert=invert, fill=fill, install=install), voxel_box(box)
        if not (install or out):
            raise ValueError("keep_components: needs install or out")
        dense = self._dense_out() if out else None
        res = N.VkLabelResult()
        N.check(self._h, N.lib().vk_label_components(self._h, C.byref(req), C.byref(vb) if vb is not None else None, None, None, 0,
                                                     dense.ctypes.data if dense is not None else None, C.byref(res)))
        return dense, res

    # -- exact Euclidean distance transform of a value range, morphology by a radius (vk_distance_transform)
    def distance_transform(self, lo, hi=float("inf"), which: str = "outside", spacing=(1, 1, 1), box=None):
        """vk_distance_transform, a distance op: the squared Euclidean distance of every voxel to the set S of voxels whose stored texel
        lies in [lo, hi] (which="outside": 0 on S) or to its complement (which="inside": 0 off S), over the integer voxel pitch `spacing`
        = (sx, sy, sz), as a uint32 array [nz, ny, nx]; DIST_INF where the target set is empty.  box: None, "clip" or
        ((x0, y0, z0), (x1, y1, z1)) restricts S only.  Blocks; changes no state of the context."""
        from .distance import distance_request
        from .label import voxel_box

        if which not in ("outside", "inside"):
            raise ValueError('which: "outside" or "inside"')
        req, vb = distance_request(lo, hi, op=which, spacing=spacing, box=box), voxel_box(box)
        dims, _ = self._volume_dtype()
        d2 = np.zeros((dims[2], dims[1], dims[0]), np.uint32)
        N.check(self._h, N.lib().vk_distance_transform(self._h, C.byref(req), C.byref(vb) if vb is not None else None, d2.ctypes.data, None, None))
        return d2

    def morph_volume(self, lo, hi=float("inf"), op: str = "close", radius: float = 1.0, spacing=(1, 1, 1), fill_in=None, fill_out: float = 0.0, install: bool = True,
                     out: bool = False, box=None):
        """vk_distance_transform, a morphology op: the set S of voxels whose stored texel lies in [lo, hi] is closed, opened, dilated or
        eroded (op) by a Euclidean ball of `radius`, in the units of the integer voxel pitch `spacing`.  A voxel that joins the set
        becomes fill_in (None: hi where it is finite, else max(lo, 1) -- a value of the range), one that leaves it fill_out; every other
        voxel keeps its bits.  install: the result replaces the context's volume (outside frame_begin / frame_end).  Returns the
        VkDistanceResult (n_foreground, n_result, n_added, n_removed); with out=True (dense [nz, ny, nx], VkDistanceResult)."""
        from .distance import MORPH_OPS, distance_request
        from .label import voxel_box

        if op not in MORPH_OPS:
            raise ValueError('op: "close", "open", "dilate" or "erode"')
        req, vb = distance_request(lo, hi, op=op, radius=radius, spacing=spacing, fill_in=fill_in, fill_out=fill_out, install=install, box=box), voxel_box(box)
        dense = self._dense_out() if out else None
        res = N.VkDistanceResult()
        N.check(self._h, N.lib().vk_distance_transform(self._h, C.byref(req), C.byref(vb) if vb is not None else None, None, dense.ctypes.data if dense is not None else None,
                                                       C.byref(res)))
        return (dense, res) if out else res

    # -- split touching objects: eroded markers grown back over the set, cut where regions meet (vk_split_components)
    def split_components(self, lo, hi=float("inf"), radius: float = 0.0, spacing=(1, 1, 1), connectivity: int = 6, box=None, labels: bool = False, fill_out: float = 0.0,
                         install: bool = False, out: bool = False):
        """vk_split_components: the set S of voxels whose stored texel lies in [lo, hi] is eroded by a Euclidean ball of `radius` (in the
        units of the integer voxel pitch `spacing`), the components of what survives grow back over S -- every voxel joins the marker that
        reaches it first, ties go to the smaller anchor -- and a voxel that touches a region of smaller id is cut: it becomes fill_out, which
        must lie outside [lo, hi].  Returns a Regions, shaped like label_components' result (.n, .sizes, .first -- a region's anchor --,
        .boxes, .largest(k), .labels with labels=True) plus .n_markers, .n_residue_regions, .n_cut, .rounds and, with out=True, .dense
        [nz, ny, nx].  install: the cut volume replaces the context's (outside frame_begin / frame_end); label_components and
        keep_components then see the regions as separate components.  One call with room for 4096 regions, a second only when there are
        more and nothing was installed: after an install the context holds the cut volume, a second call would split that one, so the
        table then stays at its first 4096 regions (.n) while .n_regions tells how many there are; blocks."""
        from .label import voxel_box
        from .split import Regions, split_request

        req, vb = split_request(lo, hi, radius=radius, spacing=spacing, connectivity=connectivity, box=box, fill_out=fill_out, install=install), voxel_box(box)
        bp = C.byref(vb) if vb is not None else None
        res = N.VkSplitResult()
        dims, _ = self._volume_dtype()
        lab = np.zeros((dims[2], dims[1], dims[0]), np.uint32) if labels else None
        dense = self._dense_out() if out else None
        room = 4096
        table = (N.VkComponent * room)()
        N.check(self._h, N.lib().vk_split_components(self._h, C.byref(req), bp, lab.ctypes.data if lab is not None else None, table, room,
                                                     dense.ctypes.data if dense is not None else None, C.byref(res)))
        n = int(res.n_regions)
        if n > room and not install:  # more regions than the table had room for: once more, for the table alone
            table = (N.VkComponent * n)()
            N.check(self._h, N.lib().vk_split_components(self._h, C.byref(req), bp, None, table, n, None, C.byref(res)))
        return Regions(table, res, lab, dense)

    # -- measure labelled regions: one exact integer record per region (vk_measure_components)
    def measure_components(self, lo=None, hi=float("inf"), connectivity: int = 6, box=None, labels=None, max_label=None):
        """vk_measure_components: a Measurements -- per region the voxel count, first voxel, box, centroid, covariance and principal axes,
        mean / std / min / max of the stored texels, and the exposed voxel faces.  labels None: the regions are label_components' components
        of [lo, hi] under `connectivity` inside `box` (after split_components(install=True): the split regions), and the label array never
        leaves the device.  labels: a uint32 array [nz, ny, nx] (label_components' or split_components' .labels, or your own; 0:
        background); the regions are 1 .. max_label (default labels.max()), and lo, hi, connectivity and box are not used.  One call with
        room for 4096 regions, a second only when there are more; blocks; changes no state of the context."""
        from .label import voxel_box
        from .measure import Measurements, measure_request

        dims, _ = self._volume_dtype()
        if labels is not None:
            labels = np.ascontiguousarray(labels, np.uint32)
            if labels.shape != (dims[2], dims[1], dims[0]):
                raise ValueError("labels: a uint32 array [nz, ny, nx] of the volume's dimensions")
            if max_label is None:
                max_label = max(int(labels.max()), 1) if labels.size else 1
            req, vb = measure_request(box=box, max_label=max_label), None
        else:
            if max_label is not None or lo is None:
                raise ValueError("measure_components: a range (lo, hi) without labels, max_label only with labels")
            req, vb = measure_request(lo, hi, connectivity=connectivity, box=box), voxel_box(box)
        bp = C.byref(vb) if vb is not None else None
        lp = labels.ctypes.data if labels is not None else None
        res = N.VkMeasureResult()
        room = 4096
        table = (N.VkRegion * room)()
        N.check(self._h, N.lib().vk_measure_components(self._h, C.byref(req), bp, lp, table, room, C.byref(res)))
        n = int(res.n_regions)
        if n > room:  # more regions than the table had room for: once more
            table = (N.VkRegion * n)()
            N.check(self._h, N.lib().vk_measure_components(self._h, C.byref(req), bp, lp, table, n, C.byref(res)))
        return Measurements(table, int(res.records_written), res, dims)

    # -- local thickness of a value range: the largest inscribed ball per voxel (vk_local_thickness)
    def local_thickness(self, lo, hi=float("inf"), max_radius: float = 16.0, spacing=(1, 1, 1), box=None, gain=None, fill_out: float = 0.0, install: bool = False,
                        out: bool = False, t2: bool = False):
        """vk_local_thickness: for every voxel of the set S of voxels whose stored texel lies in [lo, hi], the squared radius T2 of the
        largest ball that fits inside S and holds the voxel, over the integer voxel pitch `spacing`, capped at max_radius^2 (a thicker
        place reports the cap).  The dense map stores sqrt(T2) * gain on S (gain None: automatic, the thickest place stores full scale)
        and fill_out elsewhere; install: it replaces the context's volume (outside frame_begin / frame_end), so that the table march
        colours the set by thickness, volume_histogram gives the distribution and measure_components(labels=...) the mean per region.
        Returns a Thickness: n_foreground, max_t2, n_saturated, sum_t2, gain, max_thickness (2 sqrt(max_t2)), mean_t2, with t2=True .t2
        (uint32 [nz, ny, nx]) and with out=True .dense [nz, ny, nx].  Blocks."""
        from .label import voxel_box
        from .thickness import Thickness, thickness_request

        req, vb = thickness_request(lo, hi, max_radius=max_radius, spacing=spacing, box=box, gain=gain, fill_out=fill_out, install=install), voxel_box(box)
        dims, _ = self._volume_dtype()
        arr = np.zeros((dims[2], dims[1], dims[0]), np.uint32) if t2 else None
        dense = self._dense_out() if out else None
        res = N.VkThicknessResult()
        N.check(self._h, N.lib().vk_local_thickness(self._h, C.byref(req), C.byref(vb) if vb is not None else None, arr.ctypes.data if arr is not None else None,
                                                    dense.ctypes.data if dense is not None else None, C.byref(res)))
        return Thickness(res, arr, dense)

    # -- geodesic distance through a value range: sources, targets, tortuosity (vk_geodesic_distance)
    def geodesic_distance(self, lo, hi=float("inf"), sources=("x-",), seeds=(), targets=(), connectivity: int = 26, spacing=(1, 1, 1), gain: float = 0.0, fill_out: float = 0.0,
                          fill_unreached: float = 0.0, box=None, install: bool = True, out: bool = False, g: bool = False):
        """vk_geodesic_distance: for every voxel of the set S of voxels whose stored texel lies in [lo, hi] (inside box: None, "clip" or
        ((x0, y0, z0), (x1, y1, z1))), the length of the shortest path inside S from the source set -- the voxels of S on the box's faces
        `sources` ("x-", "x+", "y-", "y+", "z-", "z+") and the `seeds` (x, y, z) that lie in S -- in units of 1/256 of the integer voxel
        pitch `spacing`, over steps to the 6, 18 or 26 neighbours.  targets: the faces whose nearest reached voxel gives target_min.  The
        dense map stores g * gain on a reached voxel (gain 0: automatic, the farthest stores full scale), fill_unreached on the rest of S
        and fill_out elsewhere; install: it replaces the context's volume (outside frame_begin / frame_end), so that the table march
        colours the set by its distance from the inlet.  Returns a Geodesic: the totals, n_unreached, reached_fraction, percolates,
        max_distance, mean_distance, target_distance, tortuosity(axis), with g=True .g (uint32 [nz, ny, nx]) and .distance, with out=True
        .dense [nz, ny, nx].  Blocks."""
        from .geodesic import Geodesic, geodesic_request
        from .label import voxel_box

        req = geodesic_request(lo, hi, sources=sources, seeds=seeds, targets=targets, connectivity=connectivity, spacing=spacing, gain=gain, fill_out=fill_out,
                               fill_unreached=fill_unreached, box=box, install=install)
        vb = voxel_box(box)
        dims, _ = self._volume_dtype()
        extent = dims
        if vb is not None:
            extent = (vb.x1 - vb.x0, vb.y1 - vb.y0, vb.z1 - vb.z0)
        elif box == "clip" and self.clip_box is not None:  # the voxels whose centre lies in the clip box, as the library counts them
            cl, ch = self.clip_box
            extent = tuple(sum(1 for i in range(n) if float(np.float32(l)) <= (i + 0.5) / n <= float(np.float32(h))) for l, h, n in zip(cl, ch, dims))
        arr = np.zeros((dims[2], dims[1], dims[0]), np.uint32) if g else None
        dense = self._dense_out() if out else None
        res = N.VkGeodesicResult()
        N.check(self._h, N.lib().vk_geodesic_distance(self._h, C.byref(req), C.byref(vb) if vb is not None else None, arr.ctypes.data if arr is not None else None,
                                                      dense.ctypes.data if dense is not None else None, C.byref(res)))
        return Geodesic(res, spacing, extent, arr, dense)

    # -- steady-state diffusion through a value range: effective diffusivity, tortuosity factor (vk_steady_diffusion)
    def steady_diffusion(self, lo, hi=float("inf"), axis="z", spacing=(1, 1, 1), omega: float = 0.0, check_every: int = 32, delta_tol: float = 1e-5, flux_tol: float = 1e-3,
                         max_sweeps: int = 20000, gain: float = 0.0, fill_out: float = 0.0, box=None, install: bool = False, out: bool = False, c: bool = False):
        """vk_steady_diffusion: the Laplace equation on the set S of voxels whose stored texel lies in [lo, hi] (inside box: None, "clip" or
        ((x0, y0, z0), (x1, y1, z1))), with no-flux walls, concentration 1 on the box's first plane along `axis` ("x", "y", "z") and 0 on its
        last, by red-black over-relaxation in float32 with the integer voxel pitch `spacing`.  omega: 0 picks the factor from the extent
        along the axis; sweeps run in blocks of check_every until the largest change of a sweep is <= delta_tol and the fluxes through the
        two faces agree to flux_tol (relative), or until max_sweeps.  The dense map stores c * gain (gain 0: 1) on S and fill_out
        elsewhere; install (default False: the product is a number): it replaces the context's volume (outside frame_begin / frame_end).
        Returns a Diffusion: porosity, flux, flux_mismatch, effective_diffusivity (D_eff / D0), tortuosity_factor, mean_concentration,
        converged, sweeps and the raw totals, with c=True .c (float32 [nz, ny, nx], NaN off S), with out=True .dense [nz, ny, nx].
        Blocks."""
        from .diffusion import Diffusion, diffusion_request
        from .label import voxel_box

        req = diffusion_request(lo, hi, axis=axis, spacing=spacing, omega=omega, check_every=check_every, delta_tol=delta_tol, flux_tol=flux_tol, max_sweeps=max_sweeps, gain=gain,
                                fill_out=fill_out, box=box, install=install)
        vb = voxel_box(box)
        dims, _ = self._volume_dtype()
        extent = dims
        if vb is not None:
            extent = (vb.x1 - vb.x0, vb.y1 - vb.y0, vb.z1 - vb.z0)
        elif box == "clip" and self.clip_box is not None:  # the voxels whose centre lies in the clip box, as the library counts them
            cl, ch = self.clip_box
            extent = tuple(sum(1 for i in range(n) if float(np.float32(l)) <= (i + 0.5) / n <= float(np.float32(h))) for l, h, n in zip(cl, ch, dims))
        arr = np.zeros((dims[2], dims[1], dims[0]), np.float32) if c else None
        dense = self._dense_out() if out else None
        res = N.VkDiffusionResult()
        N.check(self._h, N.lib().vk_steady_diffusion(self._h, C.byref(req), C.byref(vb) if vb is not None else None, arr.ctypes.data if arr is not None else None,
                                                     dense.ctypes.data if dense is not None else None, C.byref(res)))
        return Diffusion(res, req.axis, extent, arr, dense)

    # -- skeleton of a value range: topology-preserving thinning to centre lines (vk_skeletonize)
    def skeletonize(self, lo, hi=float("inf"), mode: str = "curve", max_iterations: int = 0, fill_in=None, fill_out: float = 0.0, box=None, install: bool = True, classes: bool = False,
                    out: bool = False):
        """vk_skeletonize: the set S of voxels whose stored texel lies in [lo, hi] (inside box: None, "clip" or ((x0, y0, z0), (x1, y1, z1)))
        thinned to a one-voxel-wide skeleton with the same pieces, tunnels and cavities (the set 26-connected, the background 6-connected).
        mode: "curve" keeps line ends and gives centre lines, "kernel" thins to the ultimate homotopic kernel; max_iterations: 0 thins
        until nothing more can go.  The dense volume keeps the stored value on the skeleton (fill_in: a sample value stored there instead)
        and stores fill_out elsewhere; install: it replaces the context's volume (outside frame_begin / frame_end) -- after
        local_thickness(install=True) the skeleton carries the radius along each centre line.  Returns a Skeleton: n_foreground,
        n_skeleton, n_isolated, n_end, n_regular, n_junction, links, length(spacing), iterations, converged, with classes=True .classes
        (uint8 [nz, ny, nx]), with out=True .dense [nz, ny, nx].  Blocks."""
        from .label import voxel_box
        from .skeleton import Skeleton, skeleton_request

        req = skeleton_request(lo, hi, mode=mode, max_iterations=max_iterations, fill_in=fill_in, fill_out=fill_out, box=box, install=install)
        vb = voxel_box(box)
        dims, _ = self._volume_dtype()
        cls = np.zeros((dims[2], dims[1], dims[0]), np.uint8) if classes else None
        dense = self._dense_out() if out else None
        res = N.VkSkeletonResult()
        N.check(self._h, N.lib().vk_skeletonize(self._h, C.byref(req), C.byref(vb) if vb is not None else None, cls.ctypes.data if cls is not None else None,
                                                dense.ctypes.data if dense is not None else None, C.byref(res)))
        return Skeleton(res, cls, dense)

    def set_root_skip(self, k: int):
        """vk_partition_root_skip: rank 0 sits out every k-th round of the tile deal (0: never)."""
        N.check(self._h, N.lib().vk_partition_root_skip(self._h, int(k)))

    def set_wire(self, wire: int):
        """vk_partition_wire: what a pixel of this context's compact tiles holds (WIRE_RGBA: the backbuffer's pixel; WIRE_RGB:
        its three colour channels -- alpha is 1 in every pixel the path writes -- a quarter less to move between GPUs)."""
        N.check(self._h, N.lib().vk_partition_wire(self._h, int(wire)))

    @property
    def wire_pixel_bytes(self) -> int:
        n = C.c_uint32(0)
        N.check(self._h, N.lib().vk_wire_pixel_bytes(self._h, C.byref(n)))
        return int(n.value)

    def set_param(self, name: str, value: float):
        """Debug / tuning knob of the library (vk_debug_set_param)."""
        N.check(self._h, N.lib().vk_debug_set_param(self._h, name.encode(), float(value)))

    def march_path_fast(self, dt_scale: float = 1.0, flags: int = 0) -> bool:
        """Debug (vk_debug_march_path): whether a NAIVE_TRILINEAR render of the current volume from the current camera would launch the
        unclamped build of the cell march (False: the clamped one, RENDER_SAFE's).  The frame is the same either way."""
        fast = C.c_int(-1)
        N.check(self._h, N.lib().vk_debug_march_path(self._h, float(dt_scale), int(flags), C.byref(fast)))
        return bool(fast.value)

    def read_skip_maps(self):
        """Debug (vk_debug_read_skip_maps): (grid, maps) of the current volume -- grid = (cells in x, y, z), maps uint8 [n_maps, cells] as
        stored (bricked order); n_maps is 0 for a layout without maps, 1 for the isotropic map, 8 for the octant maps.  Blocks."""
        grid, n_maps, nbytes = (C.c_uint32 * 3)(), C.c_uint32(), C.c_size_t()
        N.check(self._h, N.lib().vk_debug_read_skip_maps(self._h, grid, C.byref(n_maps), C.byref(nbytes), None, 0))
        n_cells = int(grid[0]) * int(grid[1]) * int(grid[2])
        maps = np.zeros((n_maps.value, n_cells), np.uint8)
        assert maps.size == nbytes.value
        if maps.size:
            N.check(self._h, N.lib().vk_debug_read_skip_maps(self._h, grid, C.byref(n_maps), C.byref(nbytes), maps.ctypes.data, maps.size))
        return tuple(int(g) for g in grid), maps

    # -- results
    def read_backbuffer(self) -> np.ndarray:
        """The backbuffer as [H, W, 4] float32 (RGBA32F) or float16 (RGBA16F)."""
        bb = self.render_backbuffer
        dt = np.float32 if bb.format == N.OUT_RGBA32F else np.float16
        out = np.empty((bb.height, bb.width, 4), dt)
        N.check(self._h, N.lib().vk_readback(self._h, out.ctypes.data, out.strides[0]))
        return out

    def render(self):
        """Context::render (src/context.rs:251-297): the present pass -- backbuffer -> ACES + sRGB ->
        Rgba8 at the window size.  (No surface to present to on a compute node.)"""
        if self._pass_presented:  # the raycast pass has written the presented image itself (fuse_present)
            self._pass_presented = False
            return
        N.check(self._h, N.lib().vk_present(self._h, self.width, self.height, 0))

    def present_targets(self):
        """vk_present_info: the current slot's presented images as [h, w, 4] uint8 arrays, (Rgba8, Bgra8 or None).  Waits for the context's
        stream."""
        w, h, r8, b8 = C.c_uint32(), C.c_uint32(), C.c_void_p(), C.c_void_p()
        N.check(self._h, N.lib().vk_present_info(self._h, C.byref(w), C.byref(h), C.byref(r8), C.byref(b8)))
        out = []
        for p in (r8.value, b8.value):
            img = None
            if p:
                img = np.empty((h.value, w.value, 4), np.uint8)
                N.check(self._h, N.lib().vk_device_download(self._h, img.ctypes.data, p, img.size))
            out.append(img)
        return tuple(out)

    def capture_frame(self):
        """Context::capture_frame (src/context.rs:299-302, screenshot.rs:37-77): the presented Rgba8
        frame as padded rows + its ImageDimentions."""
        w, h, pitch = C.c_uint32(), C.c_uint32(), C.c_uint32()
        N.check(self._h, N.lib().vk_capture_frame(self._h, None, 0, C.byref(w), C.byref(h), C.byref(pitch)))
        dims = ImageDimentions.new(self.width, self.height, 256)
        assert (dims.width, dims.height, dims.padded_bytes_per_row) == (w.value, h.value, pitch.value)
        buf = np.zeros(dims.linear_size(), np.uint8)
        N.check(self._h, N.lib().vk_capture_frame(self._h, buf.ctypes.data, buf.size, None, None, None))
        return buf.tobytes(), dims

    def partition_active(self, tile_size: int, nranks: int = 1, mode: int = N.MODE_NAIVE_TRILINEAR):
        """(active tiles, active slots per rank): only those leading positions of the order are marched /
        gathered; the rest of the frame is clear colour."""
        a, b = C.c_uint32(), C.c_uint32()
        N.check(self._h, N.lib().vk_partition_active(self._h, mode, tile_size, nranks, C.byref(a), C.byref(b)))
        return a.value, b.value

    def partition_order(self, tile_size: int, mode: int = N.MODE_NAIVE_TRILINEAR) -> np.ndarray:
        """Heaviest-first tile order of the frame partition (position -> row-major tile id)."""
        bb = self.render_backbuffer
        n = ((bb.width + tile_size - 1) // tile_size) * ((bb.height + tile_size - 1) // tile_size)
        out = np.empty(n, np.uint32)
        N.check(self._h, N.lib().vk_partition_order(self._h, mode, tile_size, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out

    def step_counts(self):
        a, b = C.c_uint64(), C.c_uint64()
        N.check(self._h, N.lib().vk_step_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def simt_census(self) -> dict:
        out = (C.c_uint64 * 4)()
        N.check(self._h, N.lib().vk_simt_census(self._h, out))
        return {"wave_loop_iters": out[0], "wave_skip_iters": out[1], "wave_sample_execs": out[2], "lane_loop_iters": out[3]}

    def speckle_census(self) -> dict:
        out = (C.c_uint64 * 2)()
        N.check(self._h, N.lib().vk_speckle_census(self._h, out))
        return {"wave_zero_alpha_execs": out[0], "lane_proven_steps": out[1]}

    def reset_step_counts(self):
        N.check(self._h, N.lib().vk_step_counts_reset(self._h))

    def read_steps(self) -> np.ndarray:
        bb = self.render_backbuffer
        out = np.empty((bb.height, bb.width), np.uint32)
        N.check(self._h, N.lib().vk_readback_steps(self._h, out.ctypes.data))
        return out

    def timer_begin(self):
        N.check(self._h, N.lib().vk_timer_begin(self._h))

    def timer_end(self):
        N.check(self._h, N.lib().vk_timer_end(self._h))

    def timer_elapsed_ms(self) -> float:
        ms = C.c_float()
        N.check(self._h, N.lib().vk_timer_elapsed_ms(self._h, C.byref(ms)))
        return ms.value


def transfer_table(points, n: int = 256) -> np.ndarray:
    """A piecewise-linear (n, 4) float32 transfer table from control points (x, r, g, b, a), x in the table's domain mapped to
    [0, 1] (entry j sits at x = j / (n - 1)); constant beyond the first and last point."""
    p = np.asarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 5 or len(p) < 1:
        raise ValueError("transfer_table: control points are rows (x, r, g, b, a)")
    if not 2 <= n <= N.TF_MAX_ENTRIES:
        raise ValueError("transfer_table: 2 <= n <= %d entries" % N.TF_MAX_ENTRIES)
    p = p[np.argsort(p[:, 0], kind="stable")]
    x = np.arange(n, dtype=np.float64) / (n - 1)
    return np.stack([np.interp(x, p[:, 0], p[:, 1 + k]) for k in range(4)], axis=1).astype(np.float32)


class VolumeTexture:
    """src/context/volume_texture.rs:32-89: uploads the dense x-fastest volume ([nz,ny,nx]).

    fmt=None infers the format from the array: u8 -> R8_UNORM, f16 -> R16_FLOAT, and a uint16 array is taken as f16 BIT PATTERNS
    (R16_FLOAT), as it always was.  16-bit integer data (CT / MR scans) is uploaded with fmt=FMT_R16_UNORM, which takes a 3-D
    np.uint16 array and nothing else; any other explicit fmt must be the one the array would infer."""

    def __init__(self, ctx: Context, data: np.ndarray, data2: np.ndarray | None = None, layout: int = N.LAYOUT_AUTO, fmt: int | None = None):
        vol = np.ascontiguousarray(data)
        if vol.dtype == np.uint8 and vol.ndim == 3:
            inferred = N.FMT_R8_UNORM
        elif vol.dtype in (np.float16, np.uint16) and vol.ndim == 3:
            inferred = N.FMT_R16_FLOAT
        elif vol.dtype in (np.float16, np.uint16) and vol.ndim == 4 and vol.shape[3] == 4 and data2 is not None:
            inferred = N.FMT_RGBA16F_PAIR
        else:
            raise ValueError("volume must be u8[nz,ny,nx], f16[nz,ny,nx] or a pair of f16[nz,ny,nx,4]")
        if fmt == N.FMT_R16_UNORM:
            if vol.dtype != np.uint16 or vol.ndim != 3 or data2 is not None:
                raise ValueError("fmt=FMT_R16_UNORM takes one np.uint16 array [nz,ny,nx]")
        elif fmt is not None and fmt != inferred:
            raise ValueError("fmt=%r does not match the array (dtype %s, %d-D): pass fmt=None, or FMT_R16_UNORM with a uint16 array" % (fmt, vol.dtype, vol.ndim))
        else:
            fmt = inferred
        nz, ny, nx = vol.shape[:3]
        v2 = None
        if data2 is not None:
            v2 = np.ascontiguousarray(data2)
            if v2.shape != vol.shape or v2.dtype.itemsize != 2:
                raise ValueError("normals volume must match the density volume")
        N.check(ctx.handle, N.lib().vk_volume_upload(ctx.handle, vol.ctypes.data, v2.ctypes.data if v2 is not None else None,
                                                    nx, ny, nz, fmt, layout))
        self.dims = (nx, ny, nz)
        self.format = fmt

    @classmethod
    def from_raw(cls, ctx: Context, path: str, dims=(256, 256, 256), layout: int = N.LAYOUT_AUTO, dtype=np.uint8) -> "VolumeTexture":
        """Drop-in for the reference's `bonsai_256x256x256_uint8.raw` (absent from the checkout, F3).  dtype=np.uint16: a raw file of
        native-endian 16-bit integers, uploaded as R16_UNORM."""
        nx, ny, nz = dims
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise ValueError("from_raw: dtype is np.uint8 or np.uint16")
        raw = np.fromfile(path, dtype=dtype)
        if raw.size != nx * ny * nz:
            raise ValueError(f"{path}: expected {nx * ny * nz * dtype.itemsize} bytes, found {raw.size * dtype.itemsize}")
        return cls(ctx, raw.reshape(nz, ny, nx), layout=layout, fmt=N.FMT_R16_UNORM if dtype == np.uint16 else None)

    @classmethod
    def generate(cls, ctx: Context, kind: int, dims, fmt=N.FMT_R8_UNORM, seed=0x5EED0001, lo=20, span=12,
                 layout: int = N.LAYOUT_AUTO) -> "VolumeTexture":
        """Deterministic synthetic volume made on the device (GEN_FOG / GEN_BONSAI_STANDIN)."""
        nx, ny, nz = dims
        N.check(ctx.handle, N.lib().vk_volume_generate(ctx.handle, kind, nx, ny, nz, fmt, seed, lo, span, layout))
        self = cls.__new__(cls)
        self.dims, self.format = (nx, ny, nz), fmt
        return self

    @classmethod
    def generate_fog(cls, ctx: Context, dims, fmt=N.FMT_R8_UNORM, seed=0x5EED0002, lo=20, span=12,
                     layout: int = N.LAYOUT_AUTO, dense_core: bool = False) -> "VolumeTexture":
        """Fog (C2-fog, C4, C5); dense_core: with the dense ball at the centre (the configs' early-out variant)."""
        return cls.generate(ctx, N.GEN_FOG_DENSE_CORE if dense_core else N.GEN_FOG, dims, fmt, seed, lo, span, layout)

    @classmethod
    def generate_xor(cls, ctx: Context, dims=(256, 256, 256), time: float = 0.0) -> "VolumeTexture":
        """XorCompute (examples/xor/xor_compute.rs): shaders/xor.wgsl cs_main -> density + normals rgba16f."""
        nx, ny, nz = dims
        N.check(ctx.handle, N.lib().vk_volume_generate_xor(ctx.handle, nx, ny, nz, time))
        self = cls.__new__(cls)
        self.dims, self.format = (nx, ny, nz), N.FMT_RGBA16F_PAIR
        return self

    @classmethod
    def generate_standin(cls, ctx: Context, dims=(256, 256, 256), seed=0x5EED0001, layout: int = N.LAYOUT_AUTO) -> "VolumeTexture":
        return cls.generate(ctx, N.GEN_BONSAI_STANDIN, dims, N.FMT_R8_UNORM, seed, 0, 1, layout)


class RaycastPipeline:
    """examples/bonsai/raycast.rs (render pipeline) and examples/xor/raycast.rs (compute
    `single` / `tile`): records one raycast pass into the context's backbuffer."""

    def __init__(self, mode: int = N.MODE_NAIVE_TRILINEAR, dt_scale: float = 1.0, flags: int = 0):
        self.mode, self.dt_scale, self.flags = mode, dt_scale, flags

    def record(self, ctx: Context, tile=None):
        bb = ctx.render_backbuffer
        tx, ty, tw, th = (0, 0, bb.width, bb.height) if tile is None else tile
        flags = self.flags
        if ctx.fuse_present and (ctx.width, ctx.height) == (bb.width, bb.height) and not (flags & N.RENDER_COUNT):
            flags |= N.RENDER_PRESENT
            ctx._pass_presented = True
        N.check(ctx.handle, N.lib().vk_render(ctx.handle, self.mode, tx, ty, tw, th, self.dt_scale, flags))

    def record_partition(self, ctx: Context, tile_size: int, rank: int, nranks: int, compact_ptr: int):
        """March this rank's tiles of the current camera's frame into a compact buffer (several frames: render_batch)."""
        N.check(ctx.handle, N.lib().vk_render_partition(ctx.handle, self.mode, tile_size, rank, nranks, self.dt_scale,
                                                       self.flags, C.c_void_p(compact_ptr)))


def render_batch(ctx: Context, pipe: RaycastPipeline, cameras, out_ptr: int, *, tile_size: int = 64, rank: int = 0, nranks: int = 1,
                 compact: bool = False, slot_capacity: int = 0):
    """vk_render_batch: len(cameras) frames (144-byte blobs) in one launch.  Returns (batch_id, active slots per rank)."""
    if not cameras or any(len(c) != 144 for c in cameras):
        raise ValueError("render_batch: every camera is one 144-byte CameraUniform blob")
    blob = b"".join(cameras)
    n = len(blob) // 144
    bid, act = C.c_uint32(), C.c_uint32()
    N.check(ctx.handle, N.lib().vk_render_batch(ctx.handle, pipe.mode, n, blob, tile_size, rank, nranks, pipe.dt_scale, pipe.flags,
                                               C.c_void_p(out_ptr), 1 if compact else 0, slot_capacity, C.byref(bid), C.byref(act)))
    return bid.value, act.value


def untile_batch(ctx: Context, batch_id: int, gathered_ptr: int, n_slots: int, out_ptr: int, prev_batch_id: int = 0):
    """vk_untile_batch / vk_untile_batch_over: `prev_batch_id` names the batch whose un-tiled frames `out_ptr` still holds,
    untouched (0: unknown -- every inactive tile is cleared)."""
    N.check(ctx.handle, N.lib().vk_untile_batch_over(ctx.handle, batch_id, C.c_void_p(gathered_ptr), n_slots, C.c_void_p(out_ptr), int(prev_batch_id)))


def partition_slots(width: int, height: int, tile_size: int, nranks: int, root_skip: int = 0) -> int:
    n = C.c_uint32()
    rc = N.lib().vk_partition_slots_weighted(width, height, tile_size, nranks, root_skip, C.byref(n))
    if rc != N.VK_OK:
        raise N.VokselisError(rc, "vk_partition_slots: bad arguments")
    return n.value


class Demo:
    """`trait Demo` (src/lib.rs:37-43): init / update / render; resize and update_input are
    window-side and therefore absent."""

    @classmethod
    def init(cls, ctx: Context) -> "Demo":
        return cls()

    def update(self, ctx: Context):
        pass

    def render(self, ctx: Context):
        pass


def run_headless(demo_cls, frames: int = 1, camera: Camera | None = None, width: int = 1280, height: int = 720,
                 backbuffer: tuple | None = None, out_format: int = N.OUT_RGBA16F, device: int = 0, in_flight: int = 1, on_frame=None,
                 fuse_present: bool = False):
    """`run::<D>` (src/lib.rs:45-208) without the window: N frames of
    Context.update -> Demo.update -> Demo.render, then returns (ctx, demo).
    in_flight > 1: the loop runs up to that many frames ahead of the GPU, as the reference's queue does (src/lib.rs:178-194), every
    frame on a surface of its own; on_frame(ctx, frame_id), if given, is called after each frame has been submitted.
    fuse_present: the present pass rides in the raycast pass's epilogue when the window has the backbuffer's size (Context.fuse_present)."""
    ctx = Context(width, height, camera, device=device, backbuffer=backbuffer, out_format=out_format)
    if in_flight > 1:
        ctx.frames_in_flight(in_flight)
    ctx.fuse_present = bool(fuse_present)
    fc = FrameCounter()
    demo = demo_cls.init(ctx)
    for _ in range(frames):
        ctx.update(fc)
        demo.update(ctx)
        fc.record()
        fid = ctx.frame_begin()
        demo.render(ctx)
        ctx.render()  # src/lib.rs:178-182: demo.render, then context.render (present pass)
        ctx.frame_end()
        if on_frame is not None:
            on_frame(ctx, fid)
    ctx.sync()
    return ctx, demo
