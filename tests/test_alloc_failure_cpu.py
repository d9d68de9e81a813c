"""The allocation-failure hook without a GPU: the counter's arithmetic under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/alloc_hook_check.cpp), that no allocation of the library can bypass the hook, and that the sweep's table
of pinned allocation counts (tests/alloc_failure_cases.py) has a row for every entry point that allocates."""
import os
import re
import subprocess

import alloc_failure_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vokselis_amd", "csrc")


def test_hook_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "alloc_hook_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "alloc_hook_check.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    n = int(re.search(r"hook: (\d+) calls", r.stdout).group(1))
    assert n > 100000, n


def _code(text):
    """Source text without its comments (a comment may speak of an allocation)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return "\n".join(line.split("//")[0] for line in text.splitlines())


def test_every_allocation_goes_through_the_hook():
    """Any HIP allocation call in vokselis_amd/csrc stands in ctx_alloc / ctx_alloc_host (vk_ctx.hpp), in vk_ctx_create's counters -- made
    before there is a context to arm -- or in vk_comm.hip, whose group buffers belong to no context."""
    alloc = re.compile(r"\bhip\w*(?:Malloc|HostAlloc|MemPoolCreate|HostRegister)\w*\s*\(")
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".h", ".cpp")):
            lines = [l.strip() for l in _code(open(os.path.join(CSRC, name)).read()).splitlines() if alloc.search(l)]
            if lines:
                found[name] = lines
    assert set(found) == {"vk_ctx.hpp", "vk_context.hip", "vk_comm.hip"}, found
    assert len(found["vk_ctx.hpp"]) == 2 and all("ctx->alloc_fail.fires() ? kAllocRefused : bytes" in l for l in found["vk_ctx.hpp"]), found["vk_ctx.hpp"]
    assert found["vk_context.hip"] == [l for l in found["vk_context.hip"] if "&ctx->counters" in l] and len(found["vk_context.hip"]) == 1, found["vk_context.hip"]
    assert len(found["vk_comm.hip"]) == 2 and all("g->send[i]" in l or "g->recv" in l for l in found["vk_comm.hip"]), found["vk_comm.hip"]
    # the two functions clear HIP's sticky error and hand the pointer back as NULL
    hpp = _code(open(os.path.join(CSRC, "vk_ctx.hpp")).read())
    for fn in ("ctx_alloc", "ctx_alloc_host"):
        body = hpp[hpp.index("inline hipError_t %s(" % fn):]
        body = body[:body.index("\n}") + 2]
        assert "(void)hipGetLastError();" in body and "*p = nullptr;" in body and "return e;" in body, body


def test_the_parameter_is_documented_and_set():
    header = open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    context = open(os.path.join(CSRC, "vk_context.hip")).read()
    assert '"alloc_fail_at"' in header and "`alloc_fail_at`" in design and 'n == "alloc_fail_at"' in context


def test_the_table_has_a_row_for_every_entry_point():
    swept = {r.entry for r in AC.ROWS}
    assert swept == set(AC.ENTRY_POINTS), (sorted(set(AC.ENTRY_POINTS) - swept), sorted(swept - set(AC.ENTRY_POINTS)))
    assert set(AC.COUNTS) == {r.id for r in AC.ROWS}
    for rid, n in AC.COUNTS.items():
        assert isinstance(n, int) and 1 <= n <= 64, (rid, n)
    ids = [r.id for r in AC.ROWS]
    # the builds: six layouts, the pair on two, each from no volume and over one; both generators; the device upload
    for lay in ("LINEAR", "PACKED", "PACKED_PAIRS", "BRICKED", "QUADS", "STAGED"):
        for how in ("from no volume", "over a volume"):
            assert f"vk_volume_upload u8 {lay}, {how}" in ids
    for lay in ("LINEAR", "PACKED"):
        assert f"vk_volume_upload pair {lay}, from no volume" in ids and f"vk_volume_upload pair {lay}, over a volume" in ids
    # the passes: every request on every volume, with INSTALL where the request has the flag
    for p in AC.PASSES:
        for kind, lay in AC.VARIANTS:
            assert f"{p.name}, {kind} {lay}" in ids
            assert (f"{p.name}, INSTALL, {kind} {lay}" in ids) == p.install
    assert {p.entry for p in AC.PASSES} == set(AC.PASS_PREFIX)
    # the setters on both cell layouts, in every step
    for lay in ("PACKED", "PACKED_PAIRS"):
        steps = {r.what[1] for r in AC.ROWS if r.group == "setter" and r.what[3] == lay and r.entry == "vk_set_isosurface"}
        assert steps == {"set", "change of threshold", "clear"}
        assert {r.what[1] for r in AC.ROWS if r.group == "setter" and r.what[3] == lay and r.entry == "vk_set_transfer_function"} == {"set", "clear"}


def test_every_pass_has_a_case_on_every_format():
    """The cases the sweep takes from the passes' lists exist, are whole-volume requests and stay below the suite's volume sizes."""
    for p in AC.PASSES:
        for kind in ("u8", "u16", "f16"):
            c = p.case(kind)
            assert c.kind == kind and c.vol.size <= 70000, (p.name, c.name)
    assert AC.LEAK_DIMS[0] * AC.LEAK_DIMS[1] * AC.LEAK_DIMS[2] == 256 * 1024
