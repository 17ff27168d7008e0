"""Code size and digest of every kernel of one host file of csrc/ (--file=NAME, default mi_rast.hip) in the gfx950 code object hipcc
makes of it: one line `name size sha1(code) sha1(kernel descriptor)` per kernel, sorted, so that two trees are compared with diff.
The code object is linked with --emit-relocs and every relocated field is zeroed before hashing (the descriptor's offset to its code,
a kernel's pc-relative distance to a __device__ variable): what is hashed does not depend on the order the kernels were emitted in.
   python tools/kdigest.py [substring] [--file=mi_knn.hip] [-DMI_RAST_PROFILING]"""
import hashlib, os, struct, subprocess, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
flt = [a for a in sys.argv[1:] if not a.startswith("-")]
extra = [a for a in sys.argv[1:] if a.startswith("-") and not a.startswith("--file=")]
src = ([a[7:] for a in sys.argv[1:] if a.startswith("--file=")] or ["mi_rast.hip"])[-1]
with tempfile.TemporaryDirectory() as tmp:
    obj = os.path.join(tmp, "dev.o")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-fno-slp-vectorize", "--cuda-device-only", "--no-gpu-bundle-output", "-Xoffload-linker", "--emit-relocs", "-c",
                           os.path.join(root, "seganygaussians_amd/csrc", src), "-o", obj] + extra)
    elf = bytearray(open(obj, "rb").read())
assert elf[:4] == b"\x7fELF" and elf[4] == 2, "expected the ELF64 code object"
shoff, = struct.unpack_from("<Q", elf, 0x28)
shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, offset, size, link, ..
for rela in (s for s in secs if s[1] == 4):   # SHT_RELA: r_offset is an address inside section sh_info; R_AMDGPU_ABS64 / REL64 / RELATIVE64 are 8 bytes
    target = secs[rela[7]]
    for o in range(rela[4], rela[4] + rela[5], 24):
        r_offset, r_info = struct.unpack_from("<QQ", elf, o)
        at, n = target[4] + r_offset - target[3], 8 if (r_info & 0xFFFFFFFF) in (3, 5, 12) else 4
        elf[at:at + n] = bytes(n)
symtab = next(s for s in secs if s[1] == 2)
strtab = secs[symtab[6]]
syms = {}
for o in range(symtab[4], symtab[4] + symtab[5], 24):
    name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, o)
    if 0 < shndx < shnum and size:
        end = elf.index(b"\0", strtab[4] + name)
        at = secs[shndx][4] + value - secs[shndx][3]
        syms[elf[strtab[4] + name:end].decode()] = bytes(elf[at:at + size])
for k in sorted(syms):
    if k + ".kd" in syms and (not flt or any(f in k for f in flt)):
        print(k, len(syms[k]), hashlib.sha1(syms[k]).hexdigest()[:16], hashlib.sha1(syms[k + ".kd"]).hexdigest()[:16])
