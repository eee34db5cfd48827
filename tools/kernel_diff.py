#!/usr/bin/env python3
"""usage: tools/kernel_diff.py <old.so> <new.so>

Compares the gfx950 kernels of two builds of liblz4hip.so, kernel by kernel: the claim "every existing kernel disassembles to the
same instructions" as a command.  For both libraries it dumps .hip_fatbin, unbundles every hipv4-amdgcn-amd-amdhsa--gfx950 entry (a
library linked from several translation units holds one code object per unit), disassembles them, keys every function by its mangled
name, drops the instruction addresses, the function-start lines and local labels, and compares per function

  * the instruction text, and
  * for kernels, four fields of the amdhsa metadata note: .vgpr_count, .sgpr_count, .group_segment_fixed_size,
    .private_segment_fixed_size.

It reports the kernels only in old, only in new, identical and different, and the first differing lines of a different one.  A kernel
whose only differences are the literals added to the program counter after s_getpc_b64 (the distance to a global or a constant, which
moves when anything around the kernel does; its own branch offsets are position independent and must match) is listed as "pc-relative
displacement only" and does not fail the comparison.  Exit status: 0 = same kernels, same instructions, same metadata; 1 = anything else.

Needs objcopy and c++filt, and clang-offload-bundler, llvm-objdump and llvm-readelf of the ROCm tree ($ROCM_PATH, default /opt/rocm)."""
import collections
import difflib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def tool(name, *alt):
    for n in (name,) + alt:
        for p in (os.path.join(ROCM, "llvm", "bin", n), shutil.which(n)):
            if p and os.path.exists(p):
                return p
    sys.exit("kernel_diff: %s not found" % name)


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True).stdout


def bundles(fatbin):
    """the offload bundles of a .hip_fatbin section, one per translation unit (the bundler itself reads only the first of a file)"""
    pos = fatbin.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fatbin, pos + len(MAGIC))
        p, end = pos + len(MAGIC) + 8, pos
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", fatbin, p)
            p += 24 + idlen
            end = max(end, pos + off + size)
        yield fatbin[pos:max(end, p)]
        pos = fatbin.find(MAGIC, max(end, p))


def code_objects(lib, tmp):
    tag = os.path.join(tmp, str(len(os.listdir(tmp))))
    subprocess.run([tool("objcopy", "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + tag + ".fatbin", lib, tag + ".copy"],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = []
    for i, b in enumerate(bundles(open(tag + ".fatbin", "rb").read())):
        with open("%s.%d.bundle" % (tag, i), "wb") as f:
            f.write(b)
        if TARGET not in run(tool("clang-offload-bundler"), "--list", "--type=o", "--input=%s.%d.bundle" % (tag, i)).split():
            continue
        co = "%s.%d.co" % (tag, i)
        run(tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=%s.%d.bundle" % (tag, i), "--output=" + co)
        out.append(co)
    if not out:
        sys.exit("kernel_diff: %s holds no %s code object" % (lib, TARGET))
    return out


START = re.compile(r"^[0-9a-f]+ <(.+)>:$")
ADDR = re.compile(r"\s*//\s*([0-9A-Fa-f]+):\s*")          # "// 000000002A20: " in front of the encoding
SYMREF = re.compile(r"\s*<\S+>\s*$")                     # "<function+0x8c>" behind it (a branch target; labels are not compared)


def functions(co):
    """{mangled name: [instruction lines]} of one code object: the instructions inside each function symbol's size (what lies behind
    it is padding).  Labels of inline assembly are not functions: their lines are dropped, and where the disassembler prints one as
    a branch target it is replaced by a placeholder -- its number counts the expansions of the translation unit; the encoding next
    to it holds the offset"""
    size, labels = {}, set()
    for line in run(tool("llvm-readelf"), "--symbols", "--wide", co).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
        elif len(f) >= 8 and f[3] == "NOTYPE":
            labels.add(f[7])
    out, cur, end = {}, None, 0
    for line in run(tool("llvm-objdump"), "-d", "--no-show-raw-insn", co).splitlines():
        m = START.match(line)
        if m:
            if m.group(1) in size:
                cur, end = out.setdefault(m.group(1), []), int(line.split()[0], 16) + size[m.group(1)]
            continue
        a = ADDR.search(line)
        if cur is None or not line.startswith("\t") or not a or int(a.group(1), 16) >= end:
            continue
        text = ADDR.sub("  // ", SYMREF.sub("", line))
        cur.append(" ".join(WORD.sub(lambda w: "<label>" if w.group(0) in labels else w.group(0), text).split()))
    return out


def metadata(co):
    """{kernel name: {field: value}} from the amdhsa.kernels list of the metadata note"""
    out, cur, inside = {}, None, False
    for line in run(tool("llvm-readelf"), "--notes", co).splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line and not line[0].isspace():
            inside, cur = False, None
            continue
        m = re.match(r"^  (- | {2})(\.\w+):\s*(.*)$", line)     # kernel-level keys only: their arguments sit deeper
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3).strip().strip("'\"")
        if m.group(2) == ".name":
            out[cur[".name"]] = cur
    return out


def load(lib, tmp):
    text, meta = collections.defaultdict(list), {}
    objs = code_objects(lib, tmp)
    for co in objs:
        for name, body in functions(co).items():
            text[name].append(body)
        meta.update(metadata(co))
    for name in text:
        text[name].sort()
    return dict(text), meta, len(objs)


WORD = re.compile(r"[A-Za-z_.$][\w.$]*")
NUM = re.compile(r"\b(0x[0-9a-fA-F]+|[0-9A-F]{8}|\d+)\b")


def only_pc_relative(a, b):
    """the two bodies differ only in literals of instructions right behind an s_getpc_b64"""
    if len(a) != len(b):
        return False
    for i, (x, y) in enumerate(zip(a, b)):
        if x == y:
            continue
        if NUM.sub("#", x) != NUM.sub("#", y) or not any("s_getpc_b64" in l for l in a[max(0, i - 4):i]):
            return False
    return True


def family(demangled):
    return re.sub(r"^(void\s+)?(lz4hip::)?", "", re.split(r"[<(]", demangled, 1)[0])


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        old_t, old_m, old_n = load(sys.argv[1], tmp)
        new_t, new_m, new_n = load(sys.argv[2], tmp)
    names = sorted(set(old_t) | set(new_t))
    pretty = dict(zip(names, run(tool("c++filt", "llvm-cxxfilt"), *names).splitlines())) if names else {}
    kern = lambda n: n in old_m or n in new_m
    print("old: %s: %d code object(s), %d kernels, %d other device functions" % (sys.argv[1], old_n, len(old_m), len(set(old_t) - set(old_m))))
    print("new: %s: %d code object(s), %d kernels, %d other device functions" % (sys.argv[2], new_n, len(new_m), len(set(new_t) - set(new_m))))
    for side, m in (("old", old_m), ("new", new_m)):
        fam = collections.Counter(family(pretty[n]) for n in m)
        print("%s kernels by name: %s" % (side, ", ".join("%s %d" % kv for kv in sorted(fam.items(), key=lambda kv: (-kv[1], kv[0])))))
    only_old = [n for n in names if n not in new_t]
    only_new = [n for n in names if n not in old_t]
    same, moved, diff = [], [], []
    for n in names:
        if n not in old_t or n not in new_t:
            continue
        a, b = old_t[n], new_t[n]
        meta_diff = [(f, old_m.get(n, {}).get(f), new_m.get(n, {}).get(f)) for f in FIELDS if old_m.get(n, {}).get(f) != new_m.get(n, {}).get(f)]
        if a == b and not meta_diff:
            same.append(n)
        elif not meta_diff and len(a) == len(b) and all(only_pc_relative(x, y) for x, y in zip(a, b)):
            moved.append(n)
        else:
            diff.append((n, a, b, meta_diff))
    for title, lst in (("only in old", only_old), ("only in new", only_new)):
        print("\n%s: %d" % (title, len(lst)))
        for n in lst:
            print("  %s%s" % (pretty[n], "" if kern(n) else "   (device function)"))
    print("\nidentical (instructions and %s): %d" % (", ".join(FIELDS), len(same)))
    print("\npc-relative displacement only (literals behind s_getpc_b64; everything else identical): %d" % len(moved))
    for n in moved:
        print("  %s" % pretty[n])
        for x, y in zip(old_t[n], new_t[n]):
            for l, r in zip(x, y):
                if l != r:
                    print("      - %s\n      + %s" % (l, r))
    print("\nDIFFERENT: %d" % len(diff))
    for n, a, b, meta_diff in diff:
        print("  %s" % pretty[n])
        for f, o, w in meta_diff:
            print("      %s: %s -> %s" % (f, o, w))
        if len(a) != len(b):
            print("      %d bodies of this name in old, %d in new" % (len(a), len(b)))
        for x, y in zip(a, b):
            if x != y:
                print("      %d -> %d instructions; first differing lines:" % (len(x), len(y)))
                for l in list(difflib.unified_diff(x, y, "old", "new", n=1, lineterm=""))[2:14]:
                    print("        " + l)
    bad = bool(only_old or only_new or diff)
    print("\n%s" % ("NOT THE SAME KERNELS" if bad else "same kernels: %d functions compared, %d identical, %d with pc-relative displacements only"
                    % (len(names), len(same), len(moved))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
