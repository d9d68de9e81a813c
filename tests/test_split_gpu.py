"""vk_split_components on the MI355X beyond the case list: VK_SPLIT_INSTALL leaves the table, the projection, the
isosurface, the lighting and the clip box in force -- the frames after it are bit for bit those of a fresh context that set the same
state and uploaded the restatement's cut volume --; the C++ host: bonsai --split 6 --keep-pick on the fixed case written as a raw file."""
import math
import os
import subprocess

import numpy as np
import pytest

import label_helpers as LH
import split_cases as SC
import split_helpers as SH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 64, 64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("split_gpu"))


@pytest.fixture(scope="module")
def label_lib(tmp_path_factory):
    return LH.build_restatement(tmp_path_factory.mktemp("split_gpu_label"))


def _ctx(V):  # noqa: F811
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    return V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)


def _table(V):  # noqa: F811
    return V.transfer_table([(0.0, 0.0, 0.0, 0.0, 0.0), (0.3, 0.1, 0.2, 0.9, 0.0), (0.5, 1.0, 0.5, 0.1, 0.4), (1.0, 1.0, 1.0, 1.0, 0.9)], 64)


STATES = {
    "table": lambda V, c: c.set_transfer_function(_table(V), (0.0, 1.0)),
    "table, lit": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_lighting((0.3, 0.8, 0.5))),
    "table, max projection": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_projection("max")),
    "isosurface": lambda V, c: c.set_isosurface(0.35, (0.9, 0.8, 0.7), 4),
    "table, clip box": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_clip_box((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))),
}


def _frame(V, ctx):  # noqa: F811
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
    return ctx.read_backbuffer().copy()


@pytest.mark.parametrize("state", sorted(STATES))
def test_install_keeps_the_state_in_force(V, lib, state):  # noqa: F811
    c = next(c for c in SC.cases() if "fixed" in c.name and c.radius == 6.0)
    want = SH.restate_case(lib, c)
    assert int(want[2][6]) > 0
    for layout in ("LINEAR", "PACKED"):
        a, b = _ctx(V), _ctx(V)
        try:
            for ctx in (a, b):
                STATES[state](V, ctx)
            LH.upload(V, a, c.vol, c.kind, layout)
            LH.upload(V, b, want[3], c.kind, layout)
            a.update()
            b.update()
            assert np.abs(_frame(V, a)[..., :3]).sum() > 0
            rc, got = SH.run(V, a, c, install=True)
            assert rc == 0, V.native.lib().vk_last_error(a.handle)
            assert LH.differences(got, want[:4]) == "", (state, layout)
            after, fresh = _frame(V, a), _frame(V, b)
            assert np.abs(fresh[..., :3]).sum() > 0 and (after.view(np.uint32) == fresh.view(np.uint32)).all(), (state, layout)
        finally:
            a.close()
            b.close()


def test_bonsai_split_then_keep_pick_isolates_the_grain_under_the_pixel(V, lib, label_lib, tmp_path):  # noqa: F811
    """bonsai --iso 0.5 --split 6 --keep-pick: the printed totals and regions are the restatement's; the saved volume is the restatement's cut
    volume with only the component under the picked voxel kept, and that component lies inside one region of the split."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(LH.ROOT, "vokselis_amd", "_lib", "bonsai")
    c = next(c for c in SC.cases() if "fixed" in c.name and c.radius == 6.0)
    labels, table, result, dense, _ = SH.restate_case(lib, c)
    d = SC.FIXED_DIMS
    src, dst = tmp_path / "fixed.raw", tmp_path / "grain.raw"
    np.ascontiguousarray(c.vol).tofile(src)
    args = [exe, "--raw", str(src), "--dims"] + [str(v) for v in d] + ["--iso", "0.5", "--iso-refine", "16", "--size", "64x64", "--split", "6", "--keep-pick", "32", "32",
                                                                      "--save-raw", str(dst), "--frames", "1"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    lines = r.stdout.splitlines()
    n = [int(v) for v in result]
    assert ("split: [0.5, inf] radius 6 connectivity 6: %d regions (%d markers of %d voxels, %d unreached regions of %d voxels), %d foreground voxels, %d cut, %d rounds"
            % (n[0], n[2], n[3], n[4], n[5], n[1], n[6], n[7])) in lines, lines[:12]
    order = np.lexsort((table[:, 1].astype(np.int64), -table[:, 0].astype(np.int64)))
    assert [line for line in lines if line.startswith("region ")] == ["region %d: %d voxels, anchor %d, box %d %d %d .. %d %d %d" % ((k + 1,) + tuple(int(v) for v in table[k])) for k in order[:10]]
    picked = next(line for line in lines if line.startswith("keep-pick (32, 32): voxel "))
    seed = tuple(int(v) for v in picked.split("voxel ")[1].split())
    want = LH.restate(label_lib, dense, "u8", 0.5, math.inf, 6, keep="seeds", seeds=[seed])
    got = np.fromfile(dst, np.uint8).reshape(c.vol.shape)
    assert LH.differences((None, None, None, got), (None, None, None, want[3])) == ""
    kept = got != 0
    assert kept.any() and len(np.unique(labels[kept])) == 1 and int(kept.sum()) < int(result[1]) - 1000   # one grain, not both
