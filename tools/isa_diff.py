"""Compare the device code of two trees, kernel by kernel, and say for every kernel symbol whether it is identical (A), identical up
to register names (B) or different (C): tools/isa_diff.py OLD_TREE NEW_TREE [unit ...] (unit: vk_launch_cells or vk_launch_cells.hip;
default: every vk_launch_*.hip that both trees have).

Each named vk_launch_*.hip of both trees is compiled with the product's flags plus -S --cuda-device-only, the assembly is split per
kernel symbol, debug directives and comments are stripped, block labels lose their function's number in the unit (.LBB7_3 -> .LBB_3: a
function added to the unit shifts it), and every symbol lands in one class:
    A  instruction text and resource footer identical
    B  identical once every register token (vN, sN, aN, v[N:M], s[N:M], a[N:M]) is a placeholder, footers identical: renaming only
    C  anything else
Per unit the counts are printed, then every B and C symbol with both instruction counts and both footers.  A comparison of two
builds and nothing else.  The assembly of a tree is kept in tools/_isa/ keyed on the content of its csrc: an unchanged tree (the
parent, while a branch is worked on) is compiled once."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

FOOTER = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "Occupancy", "LDSByteSize", "codeLenInByte")
REG = re.compile(r"\b[vsa](?:\d+|\[\d+:\d+\])")


def launch_units(tree):
    return {os.path.splitext(f)[0] for f in os.listdir(os.path.join(tree, "vokselis_amd", "csrc")) if f.startswith("vk_launch_") and f.endswith(".hip")}


def assembly(tree, unit):
    csrc = os.path.join(tree, "vokselis_amd", "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc)) + [os.path.join(tree, "include", "vokselis_hip.h")]
    key = g._digest(files, g.HIPCC_FLAGS)
    out = os.path.join(ROOT, "tools", "_isa", "%s-%s.s" % (unit, key))
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        r = subprocess.run([hipcc] + g.HIPCC_FLAGS + ["-S", "--cuda-device-only", "-o", out + ".tmp", os.path.join(csrc, unit + ".hip")],
                           capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(r.stderr)
        os.replace(out + ".tmp", out)
    with open(out) as f:
        return f.read()


def kernels(text):
    """symbol -> (instruction lines, footer dict).  A kernel runs from its `sym:` label to its .Lfunc_end; its footer is the
    block of `; Name: value` comments that follows."""
    out, cur, in_body = {}, None, False
    for line in text.splitlines():
        m = re.match(r"^\t\.type\t(\w+),@function", line)
        if m:
            cur, in_body = ([], {}), False
            out[m.group(1)] = cur
            sym = m.group(1)
            continue
        if cur is None:
            continue
        if not in_body and not cur[0] and line.startswith(sym + ":"):
            in_body = True
        elif in_body:
            s = re.sub(r"\s+", " ", line.split(";")[0].strip())
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)  # a block's label carries its function's number in the unit: an added function renumbers the others
            if s.startswith(".Lfunc_end") or s.startswith(".section"):
                in_body = False
            elif s and (not s.startswith(".") or s.endswith(":")):  # instructions and branch targets; no .loc / .p2align / ...
                cur[0].append(s)
        else:
            m = re.match(r"^; (\w+)\s*[:=] (\S+)", line)
            if m and m.group(1) in FOOTER:
                cur[1][m.group(1)] = m.group(2)
    return {k: v for k, v in out.items() if "NumVgprs" in v[1]}


def n_instr(body):
    return sum(1 for s in body if not s.endswith(":"))


def classify(old, new):
    if old[1] != new[1]:
        return "C"
    if old[0] == new[0]:
        return "A"
    strip = lambda b: [REG.sub("R", x) for x in b]
    return "B" if strip(old[0]) == strip(new[0]) else "C"


def fmt(foot):
    return " ".join("%s=%s" % (k, foot.get(k, "?")) for k in FOOTER)


def main(argv):
    old_tree, new_tree = os.path.abspath(argv[0]), os.path.abspath(argv[1])
    units = [os.path.splitext(u)[0] for u in argv[2:]] or sorted(launch_units(old_tree) & launch_units(new_tree))
    with ThreadPoolExecutor(max_workers=7) as ex:
        asm = list(ex.map(lambda j: assembly(*j), [(t, u) for u in units for t in (old_tree, new_tree)]))
    for i, u in enumerate(units):
        ko, kn = kernels(asm[2 * i]), kernels(asm[2 * i + 1])
        cls = {s: classify(ko[s], kn[s]) for s in ko if s in kn}
        n = {c: sum(1 for v in cls.values() if v == c) for c in "ABC"}
        only_old, only_new = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
        print("%s: %d symbols  A %d  B %d  C %d%s" % (u, len(ko), n["A"], n["B"], n["C"],
              "  SYMBOLS DIFFER: -%d +%d" % (len(only_old), len(only_new)) if only_old or only_new else ""))
        for s in only_old:
            print("  only old: " + s)
        for s in only_new:
            print("  only new: " + s)
        for s in sorted(cls):
            if cls[s] != "A":
                print("  %s %s\n      old %5d instr  %s\n      new %5d instr  %s" % (cls[s], s, n_instr(ko[s][0]), fmt(ko[s][1]), n_instr(kn[s][0]), fmt(kn[s][1])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
