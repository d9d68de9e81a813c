"""Every allocation of vk_steady_diffusion, made to fail (DESIGN.md sections 23.1 and 32): vk_debug_set_param(ctx, "alloc_fail_at", k) fails
the k-th allocation a context makes, and the call is swept over k = 1, 2, ... until it returns VK_OK.  After every failing call:
VK_ERR_OOM, "vk_steady_diffusion: the <buffer>: out of memory" (or, behind an INSTALL, a message of the build), the context's volume,
maps and 64 x 64 frame as before the call, every output buffer wholly untouched or wholly the result; after the last: the outputs are the
restatement's bit for bit, and an INSTALL has left what a fresh context holds after uploading the restatement's field.  The number of
allocations is pinned, and so is the number of failing calls: an empty loop cannot pass.  The helpers are tests/alloc_failure_cases.py's
and tests/diff_alloc_helpers.py's."""
import ctypes as C
import re

import numpy as np
import pytest

import alloc_failure_cases as AC
import diff_cases as DFC
import diff_helpers as DH
import label_helpers as LH
from alloc_failure_cases import VK_ERR_OOM, VK_OK
from gpu_helpers import V  # noqa: F401
from diff_alloc_helpers import Env, arm, last_error, new_ctx, state, state_differences

pytestmark = pytest.mark.gpu

ENTRY = "vk_steady_diffusion"
OWN = 7  # the state array, the tile words, the rounds' counts, the done word, two rows of partial totals, the output buffer
BUILD = {"LINEAR": 0, "PACKED": 7, "PACKED_PAIRS": 7}  # what an install's build of the volume allocates (alloc_failure_cases._count)
OWN_BUFFERS = ("the state array", "the tile words", "the rounds' counts", "the done word", "the partial totals", "the partial totals", "the output buffer")


@pytest.fixture(scope="module")
def E(V, tmp_path_factory):  # noqa: F811
    env = Env(V)
    env.lib = DH.build_restatement(tmp_path_factory.mktemp("diff_alloc_failure"))
    return env


def _case(kind):
    return AC.pick(DFC.cases(), kind, lambda c: "full" not in c.name and "empty" not in c.name)


def _call(E, ctx, c, install):
    req, vb = DH.request(c, install)
    arr, dense, res = AC.filled(c.vol.shape, np.float32), AC.filled(c.vol.shape, c.vol.dtype), AC.filled_struct(E.N.VkDiffusionResult)
    rc = E.N.lib().vk_steady_diffusion(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, arr.ctypes.data, dense.ctypes.data, C.byref(res))
    return rc, [AC.Out("c", arr), AC.Out("dense", dense), AC.Out("result", res)]


def _message_ok(msg, install):
    if re.fullmatch(re.escape(ENTRY) + r": the [a-z' ]+: " + AC.OOM_TEXT, msg):
        return True
    return install and msg in AC.BUILD_MESSAGES


@pytest.mark.parametrize("kind, lay", AC.VARIANTS)
@pytest.mark.parametrize("install", (False, True), ids=("", "INSTALL"))
def test_a_failed_call_leaves_the_context_and_whole_outputs(E, kind, lay, install):
    V = E.V  # noqa: F811
    c = _case(kind)
    want = E.expected(("diff", c.name), lambda: DH.restate_case(E.lib, c))
    assert int(want[2][DH.R["n_foreground"]]) > 0
    ctx = new_ctx(E)
    try:
        LH.upload(V, ctx, c.vol, kind, lay)
        start = state(E, ctx)
        fails, final = [], None
        for k in range(1, 66):
            arm(ctx, k)
            rc, outs = _call(E, ctx, c, install)
            msg = last_error(E, ctx)
            arm(ctx, 0)
            if rc == VK_OK:
                final = outs
                break
            assert rc == VK_ERR_OOM and msg.endswith(": " + AC.OOM_TEXT) and _message_ok(msg, install), (k, rc, msg)
            assert state_differences(state(E, ctx), start) == "", (k, msg)
            fails.append((k, msg, outs))
        assert final is not None, "still failing at k = 65"
        n = OWN + (BUILD[lay] if install else 0)
        assert len(fails) == n and [f[0] for f in fails] == list(range(1, n + 1)), [f[1] for f in fails]                # the count of allocations, pinned
        assert [f[1] for f in fails[:OWN]] == [f"{ENTRY}: {b}: {AC.OOM_TEXT}" for b in OWN_BUFFERS]
        got = (final[0].obj, final[1].obj, DH.result_array(final[2].obj))
        assert DH.differences(got, want) == "", c.name
        for k, msg, outs in fails:
            assert AC.outputs_against(outs, final) == "", (k, msg)
        assert all(o.untouched() for _, _, outs in fails[:OWN] for o in outs), "the pass's own allocations all come before anything is written"
        if not install:
            rc, again = _call(E, ctx, c, False)
            assert rc == VK_OK and AC.outputs_against(again, final) == "" and not any(o.untouched() for o in again)
            assert state_differences(state(E, ctx), start) == ""
            return
        ref = new_ctx(E)
        try:
            LH.upload(V, ref, np.ascontiguousarray(want[1]), kind, lay)
            assert state_differences(state(E, ctx), state(E, ref)) == ""
        finally:
            ref.close()
    finally:
        ctx.close()


def test_failing_calls_lose_no_device_memory(E):
    """40 failing calls at every k, with INSTALL so that the build's allocations are among them, on a u8 PACKED volume of 128 x 64 x 32
    whose state array is 1 MiB: less than the margin of the suite's other leak tests."""
    import torch

    V = E.V  # noqa: F811
    vol = E.expected(("volume", "leak"), lambda: V.volumes.bonsai_standin(AC.LEAK_DIMS))
    c = _case("u8")._replace(vol=vol, name="the leak volume", max_sweeps=32, check_every=32)

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    ctx = new_ctx(E)
    try:
        LH.upload(V, ctx, vol, "u8", "PACKED")
        n = OWN + BUILD["PACKED"]

        def failing(k):
            arm(ctx, k)
            rc = _call(E, ctx, c, True)[0]
            arm(ctx, 0)
            assert rc == VK_ERR_OOM, (k, rc, last_error(E, ctx))

        for k in range(1, n + 1):
            failing(k)
        before = free_bytes()
        made = 0
        for k in range(1, n + 1):
            for _ in range(AC.LEAK_CALLS):
                failing(k)
                made += 1
        lost = before - free_bytes()
        assert made == AC.LEAK_CALLS * n and lost < AC.LEAK_MARGIN, f"{lost / 2**20:.1f} MiB of device memory lost over {made} failing calls"
    finally:
        ctx.close()
