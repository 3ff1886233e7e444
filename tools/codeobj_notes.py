#!/usr/bin/env python3
"""tools/codeobj_notes.py [libacdsp.so] [filter] -- per-kernel resources straight from the code objects embedded in the library.
tools/codeobj_notes.py --diff OLD NEW -- do two builds (libraries or object files) hold the same kernels?

Pure Python (no llvm tools): finds every clang offload bundle in the file, takes its gfx950 code objects, reads the
NT_AMDGPU_METADATA note (msgpack) of each and prints / returns one record per kernel: VGPRs, AGPRs, SGPRs, scratch bytes per lane
(`.private_segment_fixed_size`), spilled VGPRs / SGPRs, static LDS.  `tests/test_abi.py::test_no_kernel_uses_scratch` runs
`kernels()` over the shipped library and fails on scratch outside its allow-list; the same numbers as
`llvm-readelf --notes` on the extracted bundles.

--diff compares kernel by kernel (by mangled name, whichever code object holds it): names present on one side only, differing resource
records, and differing instruction streams (llvm-objdump's disassembly of each kernel symbol, addresses and encodings dropped).  It
prints one line per difference and a summary, and exits non-zero on any difference: the proof that a restructuring of the translation
units left the compiled kernels alone (profiles/tu_split_kernel_diff.txt)."""
import collections
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import msgpack

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _bundles(blob):
    """(triple, bytes) of every entry of every uncompressed offload bundle in the file."""
    pos = 0
    while True:
        pos = blob.find(MAGIC, pos)
        if pos < 0:
            return
        (n,) = struct.unpack_from("<Q", blob, pos + 24)
        q = pos + 32
        if n == 0 or n > 64:            # the magic string inside some unrelated data
            pos += 24
            continue
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode("ascii", "replace")
            q += 24 + tl
            yield triple, blob[pos + off:pos + off + size]
        pos += 24


def _notes(elf):
    """NT_AMDGPU_METADATA (type 32, owner AMDGPU) payloads of a 64-bit little-endian ELF."""
    if elf[:4] != b"\x7fELF":
        return
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    for i in range(shnum):
        sh = shoff + i * shentsize
        sh_type, = struct.unpack_from("<I", elf, sh + 4)
        if sh_type != 7:   # SHT_NOTE
            continue
        off, size = struct.unpack_from("<QQ", elf, sh + 0x18)
        q, end = off, off + size
        while q + 12 <= end:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, q)
            q += 12
            name = elf[q:q + namesz]
            q += (namesz + 3) & ~3
            desc = elf[q:q + descsz]
            q += (descsz + 3) & ~3
            if ntype == 32 and name.startswith(b"AMDGPU"):
                yield desc


def kernels(path):
    """List of dicts: name (mangled), vgpr, agpr, sgpr, scratch, vgpr_spill, sgpr_spill, lds, max_wg."""
    blob = open(path, "rb").read()
    out = []
    for triple, obj in _bundles(blob):
        if "gfx950" not in triple:
            continue
        for desc in _notes(obj):
            md = msgpack.unpackb(desc, raw=False, strict_map_key=False)
            for k in md.get("amdhsa.kernels", []):
                out.append({
                    "name": k.get(".name", "?"),
                    "vgpr": k.get(".vgpr_count", -1), "agpr": k.get(".agpr_count", 0), "sgpr": k.get(".sgpr_count", -1),
                    "scratch": k.get(".private_segment_fixed_size", 0),
                    "vgpr_spill": k.get(".vgpr_spill_count", 0), "sgpr_spill": k.get(".sgpr_spill_count", 0),
                    "lds": k.get(".group_segment_fixed_size", 0), "max_wg": k.get(".max_flat_workgroup_size", 0),
                })
    return out


def instruction_streams(path):
    """{mangled symbol: [instruction text, ...]} of every function in the gfx950 code objects of the file (llvm-objdump)."""
    objdump = "/opt/rocm/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        objdump = shutil.which("llvm-objdump") or objdump
    out = {}
    for triple, obj in _bundles(open(path, "rb").read()):
        if "gfx950" not in triple or obj[:4] != b"\x7fELF":
            continue
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(obj)
            f.flush()
            txt = subprocess.run([objdump, "-d", "--no-leading-addr", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in txt.split("\n"):
            if line.startswith("<") and line.endswith(">:"):
                cur = out.setdefault(line[1:-2], [])
            elif cur is not None and line.startswith(("\t", " ")):
                cur.append(line.split("//")[0].strip())   # (the comment holds the address and the encoding)
    for insns in out.values():
        # objdump's mark for a run of zeros, "...": behind a function's last instruction it is the padding up to whatever stands next in
        # the section, not part of the function; anywhere else it stays and is compared
        while insns and insns[-1] == "...":
            insns.pop()
    return out


RECORD = ("vgpr", "agpr", "sgpr", "scratch", "vgpr_spill", "sgpr_spill", "lds", "max_wg")


def diff(old, new):
    """Prints what differs between the kernels of two builds; returns the number of differences."""
    ko, kn = kernels(old), kernels(new)
    ro, rn = {k["name"]: k for k in ko}, {k["name"]: k for k in kn}
    so, sn = instruction_streams(old), instruction_streams(new)
    every, both = sorted(set(ro) | set(rn)), sorted(set(ro) & set(rn))
    dn = dict(zip(every, demangle(every)))
    n_diff = 0
    for side, ks in (("old", ko), ("new", kn)):
        for name, count in sorted(collections.Counter(k["name"] for k in ks).items()):
            if count > 1:   # the same kernel in several code objects of one build
                print("%d times in %s: %s" % (count, side, dn[name]))
                n_diff += 1
    for name in every:
        if name not in both:
            print("only in %s: %s" % ("old" if name in ro else "new", dn[name]))
            n_diff += 1
    same_rec = same_isa = n_insn = 0
    for name in both:
        rec = ["%s %s -> %s" % (f, ro[name][f], rn[name][f]) for f in RECORD if ro[name][f] != rn[name][f]]
        if rec:
            print("resources differ: %s: %s" % (dn[name], ", ".join(rec)))
        a, b = so.get(name), sn.get(name)
        if a is None or b is None:
            print("instructions differ: %s: no disassembly" % dn[name])
        elif a != b:
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("instructions differ: %s: %d -> %d instructions, first difference at %d" % (dn[name], len(a), len(b), at))
        else:
            same_isa += 1
            n_insn += len(a)
        same_rec += not rec
    n_diff += 2 * len(both) - same_rec - same_isa
    print("# old %s: %d kernels, %d distinct names" % (old, len(ko), len(ro)))
    print("# new %s: %d kernels, %d distinct names" % (new, len(kn), len(rn)))
    print("# %d names on both sides: %d with identical resource records, %d with identical instruction streams (%d instructions)" % (
        len(both), same_rec, same_isa, n_insn))
    print("# %s" % ("no difference" if n_diff == 0 else "%d differences" % n_diff))
    return n_diff


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return [s.replace("void acdsp::", "").split("(")[0] for s in r.stdout.split("\n")[:len(names)]]
    except Exception:
        return list(names)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        if len(sys.argv) != 4:
            sys.exit(__doc__.split("\n")[1])
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ac_dsp_amd", "lib", "libacdsp.so")
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    ks = kernels(lib)
    names = demangle([k["name"] for k in ks])
    bad = 0
    for k, dn in sorted(zip(ks, names), key=lambda t: t[1]):
        if flt and flt not in dn:
            continue
        bad += k["scratch"] > 0
        print("%s %-64s vgpr %3d agpr %3d sgpr %3d scratch %4d spill %3d/%-3d lds %6d" % (
            "!" if k["scratch"] > 0 else " ", dn[:64], k["vgpr"], k["agpr"], k["sgpr"], k["scratch"], k["vgpr_spill"], k["sgpr_spill"], k["lds"]))
    print("# %d kernels, %d with scratch" % (len(ks), bad))
