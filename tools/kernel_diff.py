"""Which gfx950 kernels of two builds of the C-ABI library differ (CPU only: nothing is run, nothing is changed).

   python tools/kernel_diff.py <old libmi_rast.so> <new libmi_rast.so>

Extracts the gfx950 code objects of both libraries (one per host file of csrc/), disassembles them, and compares function by
function, matched on the mangled name: the instruction stream and the registers, LDS and scratch the kernel descriptor asks
for.  Prints the functions that differ or exist on one side only; the exit status is 1 if there are any."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def tool(name, *args, cwd=None):
    exe = shutil.which(name) or os.path.join(LLVM, name)
    return subprocess.run([exe] + list(args), cwd=cwd, check=True, capture_output=True, text=True).stdout


def functions(lib):
    """{mangled name: (instruction texts, resources)} over every gfx950 code object of `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = shutil.copy(lib, tmp)   # (the code objects are written next to the file)
        tool("llvm-objdump", "--offloading", copy, cwd=tmp)
        for obj in sorted(f for f in os.listdir(tmp) if f.endswith("gfx950")):
            res, cur = {}, {}
            for line in tool("llvm-readelf", "--notes", os.path.join(tmp, obj)).splitlines():
                m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(\S+)", line)
                if not m:
                    continue
                if line.lstrip().startswith("- ") and line.index("-") <= 4:   # the next entry of amdhsa.kernels
                    cur = {}
                cur[m.group(1)] = m.group(2)
                if m.group(1) == ".symbol":
                    res[m.group(2)[:-3] if m.group(2).endswith(".kd") else m.group(2)] = cur
            name = None
            for line in tool("llvm-objdump", "-d", os.path.join(tmp, obj)).splitlines():
                m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    name = m.group(1)
                    r = tuple(res.get(name, {}).get(k) for k in RESOURCES)
                    if name in out and out[name][1] != r:
                        out[name][0].append("<another code object defines it with other resources>")
                    elif name not in out:
                        out[name] = ([], r)
                elif name and line.startswith("\t"):
                    # without the address and the encoding: they move with the kernel's place in its code object
                    out[name][0].append(re.sub(r"<[^>]*>", "", line.split("//")[0]).strip())
    for code, _ in out.values():   # the padding between one function's end and the next one's start, or the code object's end
        while code and code[-1] in ("s_nop 0", "s_code_end", "..."):
            code.pop()
    return out


def main(old, new):
    a, b = functions(old), functions(new)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in", old if name in a else new, ":", name)
        elif a[name][0] != b[name][0]:
            first = next((k for k, (x, y) in enumerate(zip(a[name][0], b[name][0])) if x != y), min(len(a[name][0]), len(b[name][0])))
            print(f"code differs: {name} ({len(a[name][0])} / {len(b[name][0])} instructions, first at {first})")
        elif a[name][1] != b[name][1]:
            print(f"resources differ: {name} {dict(zip(RESOURCES, a[name][1]))} / {dict(zip(RESOURCES, b[name][1]))}")
        else:
            continue
        bad += 1
    print(f"{len(a)} / {len(b)} functions, {sum(1 for v in b.values() if v[1][0] is not None)} kernels in the new library, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
