"""The rows of the allocation-failure sweep: every entry point that allocates device memory for a context, with
the request it is swept on and the number of allocations it makes -- pinned here, so that a pass that gains a buffer changes this table
and a sweep cannot quietly go short.  vk_debug_set_param(ctx, "alloc_fail_at", k) makes the k-th allocation from then on fail; the sweep
(tests/test_alloc_failure_gpu.py) arms it at k = 1, 2, ... until the call returns VK_OK, and the call made count + 1 attempts.

Volumes and requests come from the passes' own case lists (the first case of a format on the whole volume that is neither constant nor
refused); their restatements (the *_helpers modules) give the outputs a successful call must reproduce bit for bit.  Nothing here needs a
GPU to import: the CPU test checks the table against the list of entry points.  Dimensions are (nx, ny, nz); arrays are [nz, ny, nx]."""
import collections
import ctypes as C

import numpy as np

VK_OK, VK_ERR_INVALID, VK_ERR_HIP, VK_ERR_OOM = 0, -1, -2, -4
FILL = 0xAB             # every byte of every output buffer before a call
OOM_TEXT = "out of memory"  # hipGetErrorString(hipErrorOutOfMemory): what every message of a failed allocation ends with
W = H = 64              # the frame that stands for "what the context renders"
LEAK_DIMS = (128, 64, 32)   # every per-voxel u32 array of a pass is 1 MiB
LEAK_CALLS = 40
LEAK_MARGIN = 8 << 20

# The entry points the sweep must cover; a row names the one it sweeps (its `entry`), and the CPU test holds that none is left out.
ENTRY_POINTS = (
    "vk_volume_upload", "vk_volume_upload_device", "vk_volume_generate", "vk_volume_generate_xor",
    "vk_set_transfer_function", "vk_set_projection", "vk_set_isosurface",
    "vk_volume_histogram", "vk_extract_isosurface", "vk_volume_filter", "vk_label_components", "vk_distance_transform", "vk_volume_resample",
    "vk_split_components", "vk_measure_components", "vk_local_thickness", "vk_geodesic_distance", "vk_skeletonize",
    "vk_render", "vk_render_geometry", "vk_render_slice", "vk_present", "vk_render_batch", "vk_backbuffer_resize", "vk_ctx_frames_in_flight",
    "vk_device_alloc",
)

# the five volumes of the passes and the setters: (format, layout)
VARIANTS = (("u8", "LINEAR"), ("u8", "PACKED"), ("u8", "PACKED_PAIRS"), ("u16", "PACKED"), ("f16", "PACKED"))

# What the messages of a build's failed allocations begin with (vk_volume.hip); each is followed by " allocation failed: <HIP's text>".
BUILD_BUFFERS = ("dense volume", "dense volume (normals)", "record array", "index table", "re-layout scratch", "staged brick copy",
                 "quad layout (4.5x the dense bytes; VK_LAYOUT_STAGED is 1x per copy)", "9^3 brick array", "cell array", "distance map", "cell-index table")
BUILD_MESSAGES = tuple(b + " allocation failed: " + OOM_TEXT for b in BUILD_BUFFERS)
# ... and what a pass's begin with (its documented prefix); "prefix: the <buffer>: <HIP's text>"
PASS_PREFIX = {"vk_volume_histogram": "vk_volume_histogram", "vk_extract_isosurface": "vk_extract_isosurface", "vk_volume_filter": "vk_volume_filter",
               "vk_label_components": "vk_label_components", "vk_distance_transform": "vk_distance_transform", "vk_volume_resample": "resample",
               "vk_split_components": "vk_split_components", "vk_measure_components": "vk_measure_components", "vk_local_thickness": "vk_local_thickness",
               "vk_geodesic_distance": "vk_geodesic_distance", "vk_skeletonize": "vk_skeletonize"}


def pass_message_ok(entry, msg, install):
    """prefix: the <buffer>: out of memory -- or, behind an INSTALL, a message of the build."""
    import re

    if re.fullmatch(re.escape(PASS_PREFIX[entry]) + r": the [a-z' ]+: " + OOM_TEXT, msg):
        return True
    return install and msg in BUILD_MESSAGES


# ---- output buffers ------------------------------------------------------------------------------------------------------------------
class Out:
    """One output buffer of a call: its bytes as the library sees them, and -- for a struct with padding -- its fields."""

    def __init__(self, name, obj):
        self.name, self.obj = name, obj
        self.raw = np.frombuffer(obj, np.uint8) if not isinstance(obj, np.ndarray) else obj.reshape(-1).view(np.uint8)

    def untouched(self):
        return bool((self.raw == FILL).all())

    def value(self):
        if isinstance(self.obj, C.Structure):
            return fields(self.obj)
        return self.raw.tobytes()


def fields(s):
    """A ctypes value as nested tuples of its fields (padding left out; a float as its hex, so that NaN equals NaN)."""
    if isinstance(s, C.Structure):
        return tuple(fields(getattr(s, f[0])) for f in s._fields_)
    if isinstance(s, C.Array):
        return tuple(fields(x) for x in s)
    return s.hex() if isinstance(s, float) else s


def filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.reshape(-1).view(np.uint8)[:] = FILL
    return a


def filled_struct(cls):
    s = cls()
    C.memset(C.byref(s), FILL, C.sizeof(s))
    return s


def outputs_against(outs, final):
    """A failing call's outputs against the successful call's: each wholly untouched or wholly the result.  In words; empty: fine."""
    bad = []
    for o, f in zip(outs, final):
        if not o.untouched() and o.value() != f.value():
            bad.append(f"{o.name}: neither untouched nor the result")
    return "; ".join(bad)


# ---- the passes: a case of the pass's own list as a call with every output, and the restatement's word on the successful call -------------
def pick(cases, kind, want=lambda c: True):
    for c in cases:
        whole = getattr(c, "box", None) is None or (hasattr(c, "dims") and tuple(c.box) == (0, 0, 0) + tuple(reversed(c.vol.shape)))
        if c.kind == kind and whole and getattr(c, "clip", None) is None and not getattr(c, "refused", None) and "constant" not in c.name and 2000 <= c.vol.size <= 70000 and want(c):
            return c
    raise LookupError(kind)


def _vbp(vb):
    return C.byref(vb) if vb is not None else None


class Pass:
    """entry: the C function; variant: a word for the request; install: whether the request has an INSTALL flag.  case(kind): the case
    swept for a format.  call(E, ctx, c, install) -> (rc, [Out]).  final(E, c, outs) -> differences from the restatement, in words.
    dense(E, c) -> (the restatement's dense output, its format word): what an install makes the volume."""

    def __init__(self, entry, variant, install, case, call, final, dense=None):
        self.entry, self.variant, self.install, self.case, self.call, self.final, self.dense = entry, variant, install, case, call, final, dense

    @property
    def name(self):
        return self.entry + (", " + self.variant if self.variant else "")


def _hist_case(kind):
    import hist_cases as HC

    return pick(HC.cases(), kind, lambda c: c.bins >= 16)


def _hist_call(E, ctx, c, install):
    N = E.N
    req = N.VkHistogram(float(c.domain[0]), float(c.domain[1]), int(c.bins), 0)
    counts, stats = filled(c.bins, np.uint64), filled_struct(N.VkVolumeStats)
    rc = N.lib().vk_volume_histogram(ctx.handle, C.byref(req), None, counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(stats))
    return rc, [Out("counts", counts), Out("stats", stats)]


def _hist_final(E, c, outs):
    import hist_helpers as HH
    import np_hist_reference as NH

    counts, s = outs[0].obj, outs[1].obj
    got = dict(counts=counts, n_voxels=s.n_voxels, n_nan=s.n_nan, n_below=s.n_below, n_above=s.n_above, n_finite=s.n_finite, min=np.float32(s.min), max=np.float32(s.max),
               sum=float(s.sum), sum_sq=float(s.sum_sq))
    bad = HH.integer_part_differences(got, HH.restate_case(E.restatement("hist"), c))
    bad += HH.sum_differences(got, NH.histogram(c.vol, c.kind, c.bins, c.domain), c.kind)
    return "; ".join(bad)


def _mesh_case(kind):
    import mesh_cases as MC

    return pick(MC.cases(), kind)


def _mesh_call(E, ctx, c, install):
    N = E.N
    want = E.expected(("mesh", c.name), lambda: __import__("mesh_helpers").restate_case(E.restatement("mesh"), c))
    req = N.VkMeshRequest(float(c.iso), 0)
    cap = len(want) + 3  # (room beyond the surface stays untouched)
    tris, n = filled((cap, 3, 3), np.float32), filled(1, np.uint64)
    rc = N.lib().vk_extract_isosurface(ctx.handle, C.byref(req), None, tris.ctypes.data_as(C.POINTER(C.c_float)), cap, n.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, [Out("triangles", tris), Out("n_triangles", n)]


def _mesh_final(E, c, outs):
    want = E.expected(("mesh", c.name), None)
    tris, n = outs[0].obj, int(outs[1].obj[0])
    if n != len(want) or n == 0:
        return f"{n} triangles, the restatement has {len(want)} (the case must have some)"
    if not (tris[:n].view(np.uint32) == want.view(np.uint32)).all():
        return "triangles differ from the restatement"
    return "" if (tris[n:].view(np.uint8) == FILL).all() else "wrote beyond n_triangles"


def _filter_case(op):
    def case(kind):
        import filter_cases as FC

        return pick(FC.cases(), kind, lambda c: c.op == op)
    return case


def _filter_call(E, ctx, c, install):
    import filter_helpers as FH

    req = FH.request(E.V, c, install)
    dense = filled(c.vol.shape, c.vol.dtype)
    return E.N.lib().vk_volume_filter(ctx.handle, C.byref(req), dense.ctypes.data), [Out("dense", dense)]


def _filter_dense(E, c):
    import filter_helpers as FH

    return E.expected(("filter", c.name), lambda: FH.restate_case(E.restatement("filter"), c)), c.kind


def _dense_final(dense_of):
    def final(E, c, outs):
        want, _ = dense_of(E, c)
        got = outs[0].obj
        return "" if got.shape == want.shape and got.tobytes() == want.tobytes() else "dense differs from the restatement"
    return final


def _label_case(kind):
    import label_cases as LC

    return pick(LC.cases(), kind, lambda c: c.keep == "largest" and not c.invert and c.count == 3)


def _label_call(E, ctx, c, install):
    import label_helpers as LH

    N = E.N
    req, vb = LH.request(c, install)
    room = c.vol.size
    lab, dense, comps, res = filled(c.vol.shape, np.uint32), filled(c.vol.shape, c.vol.dtype), filled_struct(N.VkComponent * room), filled_struct(N.VkLabelResult)
    rc = N.lib().vk_label_components(ctx.handle, C.byref(req), _vbp(vb), lab.ctypes.data, comps, room, dense.ctypes.data, C.byref(res))
    return rc, [Out("labels", lab), Out("table", comps), Out("result", res), Out("dense", dense)]


def _label_restated(E, c):
    import label_helpers as LH

    return E.expected(("label", c.name), lambda: LH.restate_case(E.restatement("label"), c))


def _label_final(E, c, outs):
    import label_helpers as LH

    lab, comps, res, dense = (o.obj for o in outs)
    got = (lab, LH.table_array(comps, min(int(res.n_components), c.vol.size)), np.array([res.n_components, res.n_foreground, res.n_kept_components, res.n_kept_voxels], np.uint64), dense)
    return LH.differences(got, _label_restated(E, c))


def _dist_case(morph):
    def case(kind):
        import dist_cases as DC

        return pick(DC.cases(), kind, lambda c: (c.op in DC.MORPH) == morph and (not morph or c.radius >= 1.0))
    return case


def _dist_call(E, ctx, c, install):
    import dist_cases as DC
    import dist_helpers as DH

    N = E.N
    req, vb = DH.request(c, install)
    morph = c.op in DC.MORPH
    d2 = None if morph else filled(c.vol.shape, np.uint32)
    dense = filled(c.vol.shape, c.vol.dtype) if morph else None
    res = filled_struct(N.VkDistanceResult)
    rc = N.lib().vk_distance_transform(ctx.handle, C.byref(req), _vbp(vb), d2.ctypes.data if d2 is not None else None, dense.ctypes.data if dense is not None else None, C.byref(res))
    return rc, [Out("dense", dense) if morph else Out("d2", d2), Out("result", res)]


def _dist_restated(E, c):
    import dist_helpers as DH

    return E.expected(("dist", c.name), lambda: DH.restate_case(E.restatement("dist"), c))


def _dist_final(E, c, outs):
    import dist_cases as DC
    import dist_helpers as DH

    morph = c.op in DC.MORPH
    got = (None if morph else outs[0].obj, outs[0].obj if morph else None, DH.result_array(outs[1].obj))
    ref = _dist_restated(E, c)
    return DH.differences(got, ref) if ref is not None else "the restatement refuses the case"


def _resample_case(kind):
    import resample_cases as RC

    return pick(RC.cases(), kind, lambda c: c.mode == "linear" and c.out == c.kind and c.window is None and min(c.dims) >= 5 and int(np.prod(c.dims)) <= 70000)


def _resample_call(E, ctx, c, install):
    import resample_cases as RC
    import resample_helpers as RH

    N = E.N
    req, vb = RH.request(E.V, c, install, True, None)
    dense, res = filled((c.dims[2], c.dims[1], c.dims[0]), RC.DTYPE[c.out]), filled_struct(N.VkResampleResult)
    rc = N.lib().vk_volume_resample(ctx.handle, C.byref(req), _vbp(vb), dense.ctypes.data, C.byref(res))
    return rc, [Out("dense", dense), Out("result", res)]


def _resample_dense(E, c):
    import resample_helpers as RH

    return E.expected(("resample", c.name), lambda: RH.restate_case(E.restatement("resample"), c)), c.out


def _resample_final(E, c, outs):
    bad = _dense_final(_resample_dense)(E, c, outs)
    res = outs[1].obj
    if tuple(res.dims) != tuple(c.dims) or fields(res.box) != tuple(c.box):
        bad += "; result: dims or box are not the request's"
    return bad


def _split_case(kind):
    import split_cases as SC

    return pick(SC.cases(), kind, lambda c: c.radius >= 1.0)


def _split_call(E, ctx, c, install):
    import split_helpers as SH

    N = E.N
    req, vb = SH.request(c, install)
    room = c.vol.size
    lab, dense, comps, res = filled(c.vol.shape, np.uint32), filled(c.vol.shape, c.vol.dtype), filled_struct(N.VkComponent * room), filled_struct(N.VkSplitResult)
    rc = N.lib().vk_split_components(ctx.handle, C.byref(req), _vbp(vb), lab.ctypes.data, comps, room, dense.ctypes.data, C.byref(res))
    return rc, [Out("labels", lab), Out("table", comps), Out("result", res), Out("dense", dense)]


def _split_restated(E, c):
    import split_helpers as SH

    return E.expected(("split", c.name), lambda: SH.restate_case(E.restatement("split"), c))


def _split_final(E, c, outs):
    import label_helpers as LH
    import split_helpers as SH

    lab, comps, res, dense = (o.obj for o in outs)
    got = (lab, LH.table_array(comps, min(int(res.n_regions), c.vol.size)), SH.result_array(res), dense)
    return LH.differences(got, _split_restated(E, c)[:4])


def _measure_case(labels_in):
    def case(kind):
        import measure_cases as MC

        return pick(MC.cases(), kind, lambda c: (c.labels is not None) == labels_in)
    return case


def _measure_call(E, ctx, c, install):
    import measure_helpers as MH

    N = E.N
    lab = np.ascontiguousarray(c.labels, np.uint32) if c.labels is not None else None
    req, vb = MH.request(c, labels_in=lab is not None)
    room = int(req.max_label) if lab is not None else min(c.vol.size, MH.ROOM)
    regions, res = filled_struct(N.VkRegion * max(room, 1)), filled_struct(N.VkMeasureResult)
    rc = N.lib().vk_measure_components(ctx.handle, C.byref(req), _vbp(vb), lab.ctypes.data if lab is not None else None, regions, room, C.byref(res))
    return rc, [Out("regions", regions), Out("result", res)]


def _measure_final(E, c, outs):
    import measure_helpers as MH

    regions, res = outs[0].obj, outs[1].obj
    want, fg = E.expected(("measure", c.name), lambda: MH.restate_case(E.restatement("measure"), E.restatement("label"), c))
    if int(res.records_written) != len(want) or int(res.n_regions) != len(want) or int(res.n_foreground) != fg or len(want) == 0:
        return f"result {fields(res)}: the restatement has {len(want)} regions (the case must have some) and {fg} foreground voxels"
    return MH.differences(MH.table_array(regions, len(want)), want)


def _three(module, restatement, helper, fn, buf_name, buf_dtype, pick_want=lambda c: True):
    """The passes whose outputs are (a per-voxel array, the dense volume, a result struct): thickness, geodesic, skeleton."""
    def case(kind):
        return pick(__import__(module).cases(), kind, pick_want)

    def call(E, ctx, c, install):
        Hp = __import__(helper)
        req, vb = Hp.request(c, install)
        arr, dense, res = filled(c.vol.shape, buf_dtype), filled(c.vol.shape, c.vol.dtype), filled_struct(type(Hp.fresh_result(E.N)) if hasattr(Hp, "fresh_result") else E.N.VkThicknessResult)
        rc = getattr(E.N.lib(), fn)(ctx.handle, C.byref(req), _vbp(vb), arr.ctypes.data, dense.ctypes.data, C.byref(res))
        return rc, [Out(buf_name, arr), Out("dense", dense), Out("result", res)]

    def restated(E, c):
        Hp = __import__(helper)
        return E.expected((restatement, c.name), lambda: Hp.restate_case(E.restatement(restatement), c))

    def final(E, c, outs):
        Hp = __import__(helper)
        ref = restated(E, c)
        if ref is None:
            return "the restatement refuses the case"
        return Hp.differences((outs[0].obj, outs[1].obj, Hp.result_array(outs[2].obj)), ref)

    def dense(E, c):
        return restated(E, c)[1], c.kind

    return case, call, final, dense


_thick = _three("thick_cases", "thick", "thick_helpers", "vk_local_thickness", "t2", np.uint32)
_geo = _three("geo_cases", "geo", "geo_helpers", "vk_geodesic_distance", "g", np.uint32)
_skel = _three("skel_cases", "skel", "skel_helpers", "vk_skeletonize", "classes", np.uint8)

PASSES = (
    Pass("vk_volume_histogram", "", False, _hist_case, _hist_call, _hist_final),
    Pass("vk_extract_isosurface", "", False, _mesh_case, _mesh_call, _mesh_final),
    Pass("vk_volume_filter", "convolve", True, _filter_case("convolve"), _filter_call, _dense_final(_filter_dense), _filter_dense),
    Pass("vk_volume_filter", "median", True, _filter_case("median3"), _filter_call, _dense_final(_filter_dense), _filter_dense),
    Pass("vk_label_components", "", True, _label_case, _label_call, _label_final, lambda E, c: (_label_restated(E, c)[3], c.kind)),
    Pass("vk_distance_transform", "distance", False, _dist_case(False), _dist_call, _dist_final),
    Pass("vk_distance_transform", "morphology", True, _dist_case(True), _dist_call, _dist_final, lambda E, c: (_dist_restated(E, c)[1], c.kind)),
    Pass("vk_volume_resample", "", True, _resample_case, _resample_call, _resample_final, _resample_dense),
    Pass("vk_split_components", "", True, _split_case, _split_call, _split_final, lambda E, c: (_split_restated(E, c)[3], c.kind)),
    Pass("vk_measure_components", "range", False, _measure_case(False), _measure_call, _measure_final),
    Pass("vk_measure_components", "labels_in", False, _measure_case(True), _measure_call, _measure_final),
    Pass("vk_local_thickness", "", True, *_thick),
    Pass("vk_geodesic_distance", "", True, *_geo),
    Pass("vk_skeletonize", "", True, *_skel),
)


# ---- the rows ------------------------------------------------------------------------------------------------------------------------
# id: what pytest shows; entry: the entry point of ENTRY_POINTS; what: the words that tell the test what to do with it
Row = collections.namedtuple("Row", "id entry group what")


def _rows():
    out = []
    # volume builds, each from "no volume" and over an existing volume
    builds = [("upload", "u8", lay) for lay in ("LINEAR", "PACKED", "PACKED_PAIRS", "BRICKED", "QUADS", "STAGED")]
    builds += [("upload", "u8 sparse", "PACKED"), ("upload", "u16", "PACKED"), ("upload", "f16", "PACKED"), ("upload", "pair", "LINEAR"), ("upload", "pair", "PACKED")]
    builds += [("upload_device", "u8", "LINEAR"), ("upload_device", "u8", "PACKED"), ("upload_device", "pair", "LINEAR")]
    builds += [("generate", "u8", "PACKED_PAIRS"), ("generate", "f16", "PACKED"), ("generate_xor", "pair", "AUTO")]
    for how, vol, lay in builds:
        for over in (False, True):
            out.append(Row(f"vk_volume_{how} {vol} {lay}, {'over a volume' if over else 'from no volume'}", "vk_volume_" + how, "build", (how, vol, lay, over)))
    # setters that rebuild the maps
    for vol, lay in (("u8 sparse", "PACKED"), ("u8", "PACKED_PAIRS")):
        for entry, step in (("vk_set_transfer_function", "set"), ("vk_set_transfer_function", "clear"), ("vk_set_projection", "set"), ("vk_set_isosurface", "set"),
                            ("vk_set_isosurface", "change of threshold"), ("vk_set_isosurface", "clear")):
            out.append(Row(f"{entry} {step}, {vol} {lay}", entry, "setter", (entry, step, vol, lay)))
    # passes, with all of their outputs, and again with INSTALL
    for p in PASSES:
        for kind, lay in VARIANTS:
            for install in ((False, True) if p.install else (False,)):
                out.append(Row(f"{p.name}{', INSTALL' if install else ''}, {kind} {lay}", p.entry, "pass", (p, kind, lay, install)))
    # surfaces
    for rid, entry in (("vk_render first, counted, the order on the device", "vk_render"), ("vk_render_geometry first", "vk_render_geometry"),
                       ("vk_render_slice first with VK_SLICE_VALUES", "vk_render_slice"), ("vk_present first", "vk_present"), ("vk_present first, with the Bgra8 target", "vk_present"),
                       ("vk_render_batch first", "vk_render_batch"), ("vk_backbuffer_resize, one slot", "vk_backbuffer_resize"), ("vk_backbuffer_resize, three slots", "vk_backbuffer_resize"),
                       ("vk_ctx_frames_in_flight 1 -> 3", "vk_ctx_frames_in_flight"), ("vk_device_alloc", "vk_device_alloc")):
        out.append(Row(rid, entry, "surface", rid))
    assert len({r.id for r in out}) == len(out)
    return out


ROWS = _rows()


def _count(row):
    """The allocations of a row's call, from the code (DESIGN.md section 23.1 has the sites)."""
    # builds of a dense device array (build_from_dense): by layout
    build = {"LINEAR": 0, "PACKED": 7, "PACKED_PAIRS": 7, "BRICKED": 1, "QUADS": 1, "STAGED": 3}  # cells: the array, 4 scratch, the maps, the tables
    if row.group == "build":
        how, vol, lay, _ = row.what
        if vol == "pair":
            layout = 5 if lay in ("PACKED", "AUTO") else 0  # records: the array, the table, 3 scratch
            return {"upload": 2 + layout, "upload_device": 2, "generate_xor": 2 + layout}[how]  # (upload_device to LINEAR copies both arrays)
        return {"upload": 1 + build[lay], "upload_device": build[lay] + (1 if lay == "LINEAR" else 0), "generate": 1 + build[lay]}[how]
    if row.group == "setter":
        entry, step, _, _ = row.what
        return 5 + (1 if (entry, step) == ("vk_set_transfer_function", "set") else 0)  # 4 scratch, the maps; the table
    if row.group == "pass":
        p, kind, lay, install = row.what
        own = {"vk_volume_histogram": 1, "vk_extract_isosurface": 2, "vk_volume_filter, convolve": 1, "vk_volume_filter, median": 1, "vk_label_components": 10,
               "vk_distance_transform, distance": 4, "vk_distance_transform, morphology": 5, "vk_volume_resample": 2, "vk_split_components": 12, "vk_measure_components, range": 9,
               "vk_measure_components, labels_in": 3, "vk_local_thickness": 6, "vk_geodesic_distance": 7, "vk_skeletonize": 7}[p.name]
        return own + (build[lay] if install else 0)
    return {"vk_render first, counted, the order on the device": 3, "vk_render_geometry first": 1, "vk_render_slice first with VK_SLICE_VALUES": 1, "vk_present first": 1,
            "vk_present first, with the Bgra8 target": 2, "vk_render_batch first": 2, "vk_backbuffer_resize, one slot": 1, "vk_backbuffer_resize, three slots": 3,
            "vk_ctx_frames_in_flight 1 -> 3": 2, "vk_device_alloc": 1}[row.what]


COUNTS = {r.id: _count(r) for r in ROWS}
